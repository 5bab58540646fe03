"""tests/golden/attention_parent.npz: what ``tg_attention`` computed on an MI355X before segment 0's full key tiles were staged from running source
pointers (csrc/tg_attention.hip, ``issue_full``), as output bit patterns.

    THEATERGEN_HIP_LIB=<library of the commit to pin> python tests/golden/make_attention_parent.py attention

The stored file was recorded with the library of 05ea24b, the last commit whose tile loop derives every request's address anew for every tile.
tests/test_attention_loader_gpu.py replays the cases through the current library and requires every output bit.  Needs the GPU.  Regenerate only when
a change of the attention arithmetic is intended, and say so in that change.

Inputs are not stored: ``make_inputs`` derives them from the case's name by integer arithmetic alone (multiples of 1/64 in [-127/64, 127/64], exact in
bf16 and fp16, so both dtypes and every machine see the same values); the file keeps a SHA-256 of each case's inputs and the test compares it before it
compares outputs.  Stored inputs would triple the file.

The layout is the one the loader can get wrong (``device_args``): K is the right half of a fused [B, len0 + 3, 2 C] buffer, so its row pitch is not
heads * d and its batch stride covers three gap rows; everything in that buffer that is not K is NaN.  V^T rows have pad8(len0) + 8 columns with NaN from
column len0 on.  A source pointer that runs one tile too far, that moves on a lane which reads a constant page, or that uses the wrong pitch, reads NaN
or another batch item's rows.

tests/golden/attention_parent_wide_relpos.npz (``... make_attention_parent.py wide_relpos``): the same for ``tg_attention_wide`` (with its key split) and
``tg_attention_relpos``, recorded with the library of 6663c57, the last commit in which the three forward kernels each carried their own copy of the tile
machinery that csrc/tg_attn_fwd.h holds now.  Same means: inputs (the bias tables too) from the case's name, their SHA-256 stored, K in the fused buffer,
V^T rows with 8 spare NaN columns.  Every output of this file is stored as one SHA-256 per (batch item, block of 128 queries) of its bit patterns: the
outputs themselves (1.9 MB: the grid-64 and the d = 512 cases) would not fit a committed file, and a mismatch still names its blocks.
"""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PATH = os.path.join(ROOT, "tests", "golden", "attention_parent.npz")
PATH_WIDE_RELPOS = os.path.join(ROOT, "tests", "golden", "attention_parent_wide_relpos.npz")
B = 2
W1 = 0.4
GAP_ROWS = 3
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}

# name: heads, d, n_q, len0, len1, causal, mask
CASES = {
    "d40_one_full_tile": (2, 40, 37, 64, 0, False, False),                 # the fast path issues nothing after tile 0
    "d40_two_full_tiles_two_qblocks": (2, 40, 160, 128, 0, False, False),
    "d40_three_full_tiles_seg1": (2, 40, 37, 192, 4, False, False),        # both stage parities, then segment 1
    "d40_two_full_ragged_seg1": (2, 40, 37, 141, 4, False, False),         # a ragged tile with the V^T fix-up, then segment 1
    "d40_ragged_only": (2, 40, 37, 40, 0, False, False),
    "d64_three_full_tiles_seg1": (3, 64, 37, 192, 16, False, False),       # the instance without the bias fold and without the ones row
    "d80_two_full_ragged_seg1": (2, 80, 37, 141, 4, False, False),         # two K panels, 96 V^T rows
    "d160_three_full_tiles": (2, 160, 37, 192, 0, False, False),           # three K panels
    "d40_causal": (2, 40, 70, 192, 0, True, False),                        # the generic loader throughout
    "d64_mask_two_full_ragged": (2, 64, 37, 141, 0, False, True),          # the MASK instance
}


# name: D, heads, n_q, len0, key splits (batch B)
WIDE_CASES = {
    "wide_d256_one_tile": (256, 2, 37, 32, 1),
    "wide_d256_three_tiles_two_qblocks": (256, 1, 160, 96, 1),             # both stages, a partial second query block
    "wide_d512_ragged": (512, 1, 37, 72, 1),                               # two column parts, a ragged last tile
    "wide_d256_split2": (256, 2, 37, 104, 2),                              # key split with combine
    "wide_d512_split3_ragged": (512, 1, 160, 104, 3),                      # splits of 1, 1 and 2 tiles, the last tile ragged
}

# name: grid, d, heads, batch
RELPOS_CASES = {
    "relpos_g14_d64": (14, 64, 2, 2),                                      # four unrolled tiles, the V^T fix-up at key 196, a partial second query block
    "relpos_g14_d80": (14, 80, 2, 2),                                      # the same, plus the ones row
    "relpos_g64_d64": (64, 64, 1, 1),                                      # 64 tiles, Bh one tile ahead
    "relpos_g64_d80": (64, 80, 1, 1),
}
QBLOCK = 128                                                               # stored: one SHA-256 per (batch item, block of QBLOCK queries)


def _values(name, what, shape):
    """fp32 tensor of multiples of 1/64 in [-127/64, 127/64], a function of (name, what, index) in 64-bit integer arithmetic only"""
    n = int(np.prod(shape))
    seed = int.from_bytes(hashlib.sha256(f"{name}/{what}".encode()).digest()[:8], "little")
    x = np.arange(n, dtype=np.uint64) + np.uint64(seed)
    for mul in (0xBF58476D1CE4E5B9, 0x94D049BB133111EB):                 # splitmix64's finaliser
        x ^= x >> np.uint64(30)
        x *= np.uint64(mul)
    x ^= x >> np.uint64(31)
    v = (x % np.uint64(255)).astype(np.int64) - 127
    return torch.from_numpy((v.astype(np.float32) / 64.0).reshape(shape))


def make_inputs(name):
    heads, d, n_q, len0, len1, causal, mask = CASES[name]
    C = heads * d
    inp = {"q": _values(name, "q", (B, n_q, C)), "k0": _values(name, "k0", (B, len0, C)), "v0": _values(name, "v0", (B, len0, C))}
    if len1:
        inp["k1"], inp["v1"] = _values(name, "k1", (B, len1, C)), _values(name, "v1", (B, len1, C))
    if mask:
        inp["mask"] = _values(name, "mask", (B, 1, n_q, len0)) * 2.0          # per batch item and query, shared by the heads
    return inp


def inputs_digest(inp):
    h = hashlib.sha256()
    for k in sorted(inp):
        h.update(k.encode())
        h.update(inp[k].numpy().tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()


def reference(name, inp):
    """fp64 restatement: softmax(scale Q K0^T [+ mask] [causal]) V0 + W1 softmax(scale Q K1^T) V1 per head -> [B, n_q, C] fp64"""
    heads, d, n_q, len0, len1, causal, mask = CASES[name]
    scale = d ** -0.5

    def heads_of(t):
        return t.double().reshape(B, -1, heads, d).permute(0, 2, 1, 3)
    q = heads_of(inp["q"])

    def seg(k, v, bias):
        s = q @ heads_of(k).transpose(-1, -2) * scale
        if bias is not None:
            s = s + bias
        return s.softmax(-1) @ heads_of(v)
    bias = None
    if mask:
        bias = inp["mask"].double()
    if causal:
        bias = torch.full((n_q, len0), float("-inf"), dtype=torch.float64).triu(1)
    o = seg(inp["k0"], inp["v0"], bias)
    if len1:
        o = o + W1 * seg(inp["k1"], inp["v1"], None)
    return o.permute(0, 2, 1, 3).reshape(B, n_q, heads * d)


def device_args(name, inp, dtype, dev="cuda:0"):
    """the case in the layout of the module docstring -> (positional args of ops.attention, keyword args, out tensor)"""
    heads, d, n_q, len0, len1, causal, mask = CASES[name]
    C = heads * d
    nan = float("nan")
    kbuf = torch.full((B, len0 + GAP_ROWS, 2 * C), nan, dtype=dtype)
    kbuf[:, :len0, C:] = inp["k0"].to(dtype)
    ld0 = (len0 + 7) // 8 * 8 + 8
    vt0 = torch.full((B, C, ld0), nan, dtype=dtype)
    vt0[:, :, :len0] = inp["v0"].to(dtype).permute(0, 2, 1)
    kw = dict(causal=causal)
    if len1:
        ld1 = (len1 + 7) // 8 * 8
        vt1 = torch.full((B, C, ld1), nan, dtype=dtype)
        vt1[:, :, :len1] = inp["v1"].to(dtype).permute(0, 2, 1)
        kw.update(k1=inp["k1"].to(dtype).to(dev), k1_ld=C, k1_bs=len1 * C, vt1=vt1.to(dev), vt1_ld=ld1, vt1_bs=C * ld1, len1=len1, w1=W1)
    if mask:
        kw["mask"] = inp["mask"].to(dev).contiguous()
    kdev = kbuf.to(dev)
    out = torch.zeros((B, n_q, C), dtype=dtype, device=dev)
    args = (inp["q"].to(dtype).to(dev), C, n_q * C, kdev[:, :, C:], 2 * C, (len0 + GAP_ROWS) * 2 * C, vt0.to(dev), ld0, C * ld0, len0,
            B, heads, d, n_q, d ** -0.5, out, C, n_q * C)
    return args, kw, out


def run(ops, name, inp, dtype, dev="cuda:0"):
    """one launch -> the output tensor [B, n_q, C] on the device"""
    args, kw, out = device_args(name, inp, dtype, dev)
    ops.attention(*args, **kw)
    torch.cuda.synchronize()
    return out


# ---- tg_attention_wide and tg_attention_relpos ---------------------------------------------------------------------------------------------------------
def _shape2(name):
    """(batch, heads, d, n_q, len0) of a wide or rel-pos case"""
    if name in WIDE_CASES:
        D, heads, n_q, len0, _ = WIDE_CASES[name]
        return B, heads, D, n_q, len0
    grid, d, heads, batch = RELPOS_CASES[name]
    return batch, heads, d, grid * grid, grid * grid


def make_inputs2(name):
    batch, heads, d, n_q, len0 = _shape2(name)
    C = heads * d
    inp = {"q": _values(name, "q", (batch, n_q, C)), "k0": _values(name, "k0", (batch, len0, C)), "v0": _values(name, "v0", (batch, len0, C))}
    if name in RELPOS_CASES:
        grid = RELPOS_CASES[name][0]
        inp["bh"], inp["bw"] = _values(name, "bh", (batch, heads, n_q, grid)), _values(name, "bw", (batch, heads, n_q, grid))
    return inp


def reference2(name, inp):
    """fp64 restatement: softmax(scale Q K^T [+ bh[i, j // G] + bw[i, j % G]]) V per head -> [batch, n_q, C] fp64"""
    batch, heads, d, n_q, len0 = _shape2(name)

    def heads_of(t):
        return t.double().reshape(batch, -1, heads, d).permute(0, 2, 1, 3)
    s = heads_of(inp["q"]) @ heads_of(inp["k0"]).transpose(-1, -2) * d ** -0.5
    if name in RELPOS_CASES:
        grid = RELPOS_CASES[name][0]
        s = (s.reshape(batch, heads, n_q, grid, grid) + inp["bh"].double()[..., :, None] + inp["bw"].double()[..., None, :]).reshape(batch, heads, n_q, len0)
    return (s.softmax(-1) @ heads_of(inp["v0"])).permute(0, 2, 1, 3).reshape(batch, n_q, heads * d)


def run2(ops, name, inp, dtype, dev="cuda:0"):
    """one call of ops.attention_wide / ops.attention_relpos in the layout of the module docstring -> the output tensor [batch, n_q, C] on the device"""
    batch, heads, d, n_q, len0 = _shape2(name)
    C = heads * d
    nan = float("nan")
    kbuf = torch.full((batch, len0 + GAP_ROWS, 2 * C), nan, dtype=dtype)
    kbuf[:, :len0, C:] = inp["k0"].to(dtype)
    ld0 = (len0 + 7) // 8 * 8 + 8
    vt0 = torch.full((batch, C, ld0), nan, dtype=dtype)
    vt0[:, :, :len0] = inp["v0"].to(dtype).permute(0, 2, 1)
    kdev = kbuf.to(dev)
    out = torch.zeros((batch, n_q, C), dtype=dtype, device=dev)
    qkv = (inp["q"].to(dtype).to(dev), C, n_q * C, kdev[:, :, C:], 2 * C, (len0 + GAP_ROWS) * 2 * C, vt0.to(dev), ld0, C * ld0)
    if name in WIDE_CASES:
        ops.attention_wide(*qkv, len0, batch, heads, d, n_q, d ** -0.5, out, C, n_q * C, key_splits=WIDE_CASES[name][4])
    else:
        ops.attention_relpos(*qkv, batch, heads, d, RELPOS_CASES[name][0], d ** -0.5, inp["bh"].to(dev), inp["bw"].to(dev), out, C, n_q * C)
    torch.cuda.synchronize()
    return out


def stored_form(out):
    """what the file keeps of an output [batch, n_q, C]: uint8 [batch, blocks, 32], the SHA-256 of the bit patterns of each block of QBLOCK queries"""
    bits = np.ascontiguousarray(out.view(torch.int16).cpu().numpy())
    return np.stack([np.stack([np.frombuffer(hashlib.sha256(b[i:i + QBLOCK].tobytes()).digest(), dtype=np.uint8) for i in range(0, b.shape[0], QBLOCK)])
                     for b in bits])


def _record(path, cases, inputs, runner, form):
    from theatergen_amd import _lib, ops
    arrays = {}
    for name in cases:
        inp = inputs(name)
        arrays[f"{name}/inputs_sha256"] = inputs_digest(inp)
        for tag, dtype in DTYPES.items():
            out = runner(ops, name, inp, dtype)
            assert torch.isfinite(out.float()).all(), (name, tag)
            arrays[f"{name}/{tag}"] = form(out)
    np.savez_compressed(path, **arrays)
    print(f"{len(cases)} cases, {len(arrays)} arrays, {os.path.getsize(path)} bytes from {_lib.LIB_PATH}")


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    if sys.argv[1:] == ["attention"]:
        _record(PATH, list(CASES), make_inputs, run, lambda out: out.view(torch.int16).cpu().numpy())
    elif sys.argv[1:] == ["wide_relpos"]:
        _record(PATH_WIDE_RELPOS, list(WIDE_CASES) + list(RELPOS_CASES), make_inputs2, run2, stored_form)
    else:
        sys.exit("which file: attention | wide_relpos")
