"""tests/golden/attention_parent.npz: what ``tg_attention`` computed on an MI355X before segment 0's full key tiles were staged from running source
pointers (csrc/tg_attention.hip, ``issue_full``), as output bit patterns.

    THEATERGEN_HIP_LIB=<library of the commit to pin> python tests/golden/make_attention_parent.py

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
"""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PATH = os.path.join(ROOT, "tests", "golden", "attention_parent.npz")
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


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from theatergen_amd import _lib, ops
    arrays = {}
    for name in CASES:
        inp = make_inputs(name)
        arrays[f"{name}/inputs_sha256"] = inputs_digest(inp)
        for tag, dtype in DTYPES.items():
            out = run(ops, name, inp, dtype)
            assert torch.isfinite(out.float()).all(), (name, tag)
            arrays[f"{name}/{tag}"] = out.view(torch.int16).cpu().numpy()
    np.savez_compressed(PATH, **arrays)
    print(f"{len(CASES)} cases, {len(arrays)} arrays, {os.path.getsize(PATH)} bytes from {_lib.LIB_PATH}")
