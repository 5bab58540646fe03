"""CPU: key-split execution of the wide-head flash attention (``tg_attention_wide_split`` and its two host queries; csrc/tg_attention_wide.hip) —
what can be pinned without a device.

  * the header declares the three symbols, ``_lib.SIGNATURES`` binds them with the declared argument lists, the library exports them, ABI 308 stays;
  * ``tg_attention_wide_splits`` is host logic: the planner's invariants over a grid of descriptors, the clamp to the number of 32-key tiles, the
    refusals of ``tg_attention_wide`` as negative codes, the dev knob ``TG_ATTN_WIDE_SPLIT`` read at every call;
  * ``tg_attention_wide_workspace_bytes`` is the header's formula, 0 at ``splits <= 1``;
  * the ``TG_ERR_ARG`` refusals of ``tg_attention_wide_split`` (splits 0, workspace NULL / misaligned / short) come back before any device call:
    this test runs on a machine without a GPU, with fake pointers that are never read;
  * the resource gates: the split instances of ``attention_wide_kernel<`` pass the existing 0-scratch gate, the combine kernel has its own;
  * the VAE switch ``flash_split``: off by default, forwarded by ``AutoencoderKL``, ``TG_VAE_FLASH_SPLIT=1`` means "planner".
"""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TG_ERR_ARG, TG_ERR_UNSUPPORTED = -1, -3
FAKE = 16                                                             # a non-null, 16-byte aligned "pointer": validation never reads it
NEW = ("tg_attention_wide_splits", "tg_attention_wide_workspace_bytes", "tg_attention_wide_split")


def _lib_built():
    from theatergen_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib


def _desc(head_dim=512, heads=1, batch=1, n_q=4096, len0=4096, **over):
    from theatergen_amd import _lib
    d = _lib.AttnDesc()
    inner = heads * head_dim
    d.dtype, d.batch, d.heads, d.head_dim, d.n_q, d.len0 = 0, batch, heads, head_dim, n_q, len0
    d.q = d.k0 = d.vt0 = d.out = FAKE
    d.q_ld, d.q_bs, d.k0_ld, d.k0_bs, d.vt0_ld, d.vt0_bs = inner, n_q * inner, inner, len0 * inner, len0, inner * len0
    d.out_ld, d.out_bs, d.scale = inner, n_q * inner, head_dim ** -0.5
    for f, v in over.items():
        setattr(d, f, v)
    return d


def _blocks(head_dim, heads, batch, n_q):
    return ((n_q + 127) // 128) * heads * batch * (head_dim // 256)


def test_symbols_are_declared_bound_and_exported_at_abi_308():
    _lib = _lib_built()
    header = open(os.path.join(ROOT, "include", "theatergen_hip.h")).read()
    for decl in (r"^int tg_attention_wide_splits\(const tg_attn_desc\* d, int32_t requested\);",
                 r"^int64_t tg_attention_wide_workspace_bytes\(const tg_attn_desc\* d, int32_t splits\);",
                 r"^int tg_attention_wide_split\(const tg_attn_desc\* d, int32_t splits, void\* workspace, int64_t workspace_bytes, void\* stream\);"):
        assert re.search(decl, header, flags=re.M), decl
    P, S = C.POINTER(_lib.AttnDesc), _lib.SIGNATURES
    assert S["tg_attention_wide_splits"] == (_lib.i32, [P, _lib.i32])
    assert S["tg_attention_wide_workspace_bytes"] == (_lib.i64, [P, _lib.i32])
    assert S["tg_attention_wide_split"] == (_lib.i32, [P, _lib.i32, _lib.vp, _lib.i64, _lib.vp])
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    h = _lib.lib()
    for name in NEW:
        assert re.search(rf"\bT {name}$", nm, flags=re.M), f"libtheatergen_hip.so does not export {name}"
        assert getattr(h, name) is not None
    assert re.search(r"#define TG_ABI_VERSION 308\b", header) and _lib.ABI_VERSION == 308 and h.tg_version() == 308


def test_planner_invariants_over_a_grid_of_descriptors(monkeypatch):
    monkeypatch.delenv("TG_ATTN_WIDE_SPLIT", raising=False)
    h = _lib_built().lib()
    sizes = (8, 16, 40, 128, 136, 256, 264, 1000, 1024, 2048, 4096, 4104, 8192, 16384)
    seen_split = 0
    for hd in (256, 512):
        for batch in range(1, 9):
            for heads in (1, 2):
                for n_q in sizes:
                    for len0 in sizes:
                        d = _desc(hd, heads, batch, n_q, len0)
                        S = h.tg_attention_wide_splits(C.byref(d), 0)
                        blocks, nt = _blocks(hd, heads, batch, n_q), (len0 + 31) // 32
                        what = f"d{hd} B{batch} H{heads} n_q{n_q} len{len0}: S = {S}, blocks = {blocks}, nt = {nt}"
                        assert S >= 1, what
                        assert S <= nt, what
                        assert S == 1 or blocks < 256, what
                        assert S == 1 or blocks * S <= 512, what
                        assert S == h.tg_attention_wide_splits(C.byref(d), 0), what                 # the same answer when asked again
                        # ... and a function of the five sizes alone: other pitches, pointers, dtype and scale do not move it
                        e = _desc(hd, heads, batch, n_q, len0, dtype=1, scale=0.5, q=FAKE * 3, q_ld=heads * hd + 8, vt0_ld=len0 + 8, out_ld=heads * hd + 4)
                        assert h.tg_attention_wide_splits(C.byref(e), 0) == S, what
                        seen_split += S > 1
    assert seen_split > 100, "the planner never splits: the grid checks nothing"


def test_planner_picks_at_the_shapes_users_decode(monkeypatch):
    monkeypatch.delenv("TG_ATTN_WIDE_SPLIT", raising=False)
    h = _lib_built().lib()
    for hd in (256, 512):
        assert h.tg_attention_wide_splits(C.byref(_desc(hd, 1, 1, 4096, 4096)), 0) > 1, f"B = 1, N = 4096, d = {hd}: 64 / 32 workgroups on 256 CUs"
    assert h.tg_attention_wide_splits(C.byref(_desc(512, 1, 1, 16384, 16384)), 0) == 1            # 256 workgroups: one full wave already
    for hd in (256, 512):
        assert h.tg_attention_wide_splits(C.byref(_desc(hd, 1, 8, 4096, 4096)), 0) == 1           # 256 / 512 workgroups


def test_requested_is_clamped_to_the_tile_count_and_the_knob_forces(monkeypatch):
    monkeypatch.delenv("TG_ATTN_WIDE_SPLIT", raising=False)
    h = _lib_built().lib()
    for len0, nt in ((8, 1), (32, 1), (40, 2), (200, 7), (4096, 128)):
        d = _desc(256, 1, 2, 40, len0)
        for req in (1, 2, 3, 7, 8, 100, 1000):
            assert h.tg_attention_wide_splits(C.byref(d), req) == min(req, nt), (len0, req)
    assert h.tg_attention_wide_splits(C.byref(_desc()), -1) == TG_ERR_ARG
    # the dev knob: read at every call, only where the planner is asked, clamped like a request
    d = _desc(512, 1, 8, 4096, 4096)
    assert h.tg_attention_wide_splits(C.byref(d), 0) == 1
    monkeypatch.setenv("TG_ATTN_WIDE_SPLIT", "3")
    assert h.tg_attention_wide_splits(C.byref(d), 0) == 3 and h.tg_attention_wide_splits(C.byref(d), 2) == 2
    assert h.tg_attention_wide_splits(C.byref(_desc(256, 1, 1, 40, 40)), 0) == 2
    monkeypatch.setenv("TG_ATTN_WIDE_SPLIT", "1")
    assert h.tg_attention_wide_splits(C.byref(_desc(512, 1, 1, 4096, 4096)), 0) == 1
    monkeypatch.delenv("TG_ATTN_WIDE_SPLIT")
    assert h.tg_attention_wide_splits(C.byref(d), 0) == 1 and h.tg_attention_wide_splits(C.byref(_desc(512, 1, 1, 4096, 4096)), 0) > 1


def test_workspace_bytes_is_the_documented_formula():
    h = _lib_built().lib()
    for hd, heads, batch, n_q, len0 in ((512, 1, 1, 4096, 4096), (256, 2, 3, 136, 200), (256, 1, 2, 8, 72), (512, 1, 2, 40, 40)):
        d = _desc(hd, heads, batch, n_q, len0)
        nt, rows = (len0 + 31) // 32, ((n_q + 127) // 128) * 128
        for splits in (-3, 0, 1):
            assert h.tg_attention_wide_workspace_bytes(C.byref(d), splits) == 0
        for splits in (2, 3, 4, 7, 8, 1000):
            S = min(splits, nt)
            want = S * batch * heads * rows * (hd + 2) * 4 if S > 1 else 0
            assert h.tg_attention_wide_workspace_bytes(C.byref(d), splits) == want, (hd, heads, batch, n_q, len0, splits)
    assert h.tg_attention_wide_workspace_bytes(C.byref(_desc()), 4) == 4 * 4096 * 514 * 4                # 33.7 MB: the figure of the documents
    assert h.tg_attention_wide_workspace_bytes(C.byref(_desc(256, 1, 2, 40, 8)), 4) == 0                 # one tile: one effective split


REFUSALS = [(f"head_dim {hd}", dict(head_dim=hd), TG_ERR_UNSUPPORTED) for hd in (64, 160, 192, 384, 1024)] + [
    ("len1 > 0", dict(len1=8, k1=FAKE, vt1=FAKE, k1_ld=512, vt1_ld=8), TG_ERR_UNSUPPORTED),
    ("causal", dict(causal=1), TG_ERR_UNSUPPORTED),
    ("mask", dict(mask=FAKE), TG_ERR_UNSUPPORTED),
    ("w1_dev", dict(w1_dev=FAKE), TG_ERR_UNSUPPORTED),
    ("bad dtype", dict(dtype=2), TG_ERR_ARG),
    ("batch 0", dict(batch=0), TG_ERR_ARG),
    ("len0 % 8", dict(len0=76), TG_ERR_ARG),
    ("scale 0", dict(scale=0.0), TG_ERR_ARG),
    ("vt0_ld % 8", dict(vt0_ld=76), TG_ERR_ARG),
    ("null q", dict(q=None), TG_ERR_ARG),
]


@pytest.mark.parametrize("what,over,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_what_the_unsplit_entry_refuses_the_new_entries_refuse(what, over, code):
    """the same code from ``tg_attention_wide`` (stream NULL, never reached), ``tg_attention_wide_splits`` and ``tg_attention_wide_split``"""
    _lib = _lib_built()
    h = _lib.lib()
    d = _desc(**dict(dict(n_q=40, len0=72, batch=2), **over))
    assert h.tg_attention_wide(C.byref(d), None) == code
    for req in (0, 1, 2):
        assert h.tg_attention_wide_splits(C.byref(d), req) == code, f"{what}, requested {req}"
    assert b"tg_attention_wide_splits:" in h.tg_last_error()
    assert h.tg_attention_wide_workspace_bytes(C.byref(d), 2) == 0
    assert h.tg_attention_wide_split(C.byref(d), 2, FAKE, 1 << 30, None) == code
    assert b"tg_attention_wide_split:" in h.tg_last_error()
    assert h.tg_attention_wide_splits(None, 0) == TG_ERR_ARG and h.tg_attention_wide_split(None, 2, FAKE, 1 << 30, None) == TG_ERR_ARG


def test_split_entry_refuses_bad_splits_and_workspaces_before_any_device_call():
    """no GPU here and fake pointers: a check that ran after a launch (or after the LDS attribute call) could not return TG_ERR_ARG"""
    _lib = _lib_built()
    h = _lib.lib()
    d = _desc(256, 1, 2, 40, 200)
    need = h.tg_attention_wide_workspace_bytes(C.byref(d), 3)
    assert need == 3 * 2 * 128 * 258 * 4
    cases = {"splits 0": (0, FAKE, need), "splits -2": (-2, FAKE, need), "null workspace": (3, None, need), "misaligned workspace": (3, FAKE + 8, need),
             "short workspace": (3, FAKE, need - 1), "zero-byte workspace": (3, FAKE, 0)}
    for what, (splits, ws, nbytes) in cases.items():
        assert h.tg_gemm(C.byref(_lib.GemmDesc()), None) == -1 and b"tg_gemm" in h.tg_last_error()       # another call's message, to be replaced
        rc = h.tg_attention_wide_split(C.byref(d), splits, ws, nbytes, None)
        assert rc == TG_ERR_ARG, f"{what}: returned {rc}"
        assert b"tg_attention_wide_split:" in h.tg_last_error(), f"{what}: {h.tg_last_error()!r}"
        with pytest.raises(RuntimeError, match="theatergen_hip error"):
            _lib.check(rc)


def test_resource_gates_cover_the_split_instances_and_the_combine_kernel():
    from theatergen_amd import build
    _lib_built()
    if not os.path.exists(os.path.join(build.OBJ, "tg_attention_wide.o.res")):
        build.build(verbose=False)
    assert ("attention_wide_kernel<", 0, 256) in build.HOT_GATES                                  # the existing gate, unchanged
    gates = [g for g in build.HOT_GATES if g[0] == "attention_wide_combine_kernel<"]
    assert len(gates) == 1 and gates[0][1] == 0, gates
    res = build.kernel_resources(verbose=False)
    for T in ("bf16", "f16"):
        for shape in ("256,256", "512,256"):
            for split in ("false", "true"):
                n = f"attention_wide_kernel<{T},{shape},{split}>"
                assert n in res, f"{n} is not in the built object: {sorted(k for k in res if 'attention_wide' in k)}"
                assert res[n].get("scratch", 0) == 0 and res[n].get("vgpr_spill", 0) == 0 and res[n].get("vgprs", 0) <= 256, f"{n}: {res[n]}"
        for D in (256, 512):
            n = f"attention_wide_combine_kernel<{T},{D}>"
            assert n in res and res[n].get("scratch", 0) == 0, f"{n}: {res.get(n)}"
    assert not [b for b in build.check_resources(res) if "attention_wide" in b]


def test_vae_flash_split_switch(monkeypatch):
    import inspect
    from theatergen_amd import ops
    from theatergen_amd.vae import AutoencoderKL, VAEAttention, sd_vae_config
    assert inspect.signature(ops.attention_wide).parameters["key_splits"].default is None
    monkeypatch.delenv("TG_VAE_FLASH_SPLIT", raising=False)
    assert VAEAttention(512).flash_split is None and VAEAttention(512).key_splits() is None       # default off
    assert VAEAttention(512, flash_split=True).key_splits() == 0                                   # the planner
    assert VAEAttention(512, flash_split=4).key_splits() == 4
    assert VAEAttention(512, flash_split=False).key_splits() is None
    monkeypatch.setenv("TG_VAE_FLASH_SPLIT", "1")
    assert VAEAttention(512).key_splits() == 0
    assert VAEAttention(512, flash_split=False).key_splits() is None                               # the attribute wins over the environment
    assert VAEAttention(512, flash_split=2).key_splits() == 2
    assert not VAEAttention(512).flash_route()                                                     # the split switch does not select the flash route
    monkeypatch.setenv("TG_VAE_FLASH_SPLIT", "0")
    assert VAEAttention(512).key_splits() is None
    monkeypatch.delenv("TG_VAE_FLASH_SPLIT")
    vae = AutoencoderKL(sd_vae_config(block_out_channels=(32, 64)), flash=True, flash_split=2)
    for m in (vae.encoder, vae.decoder):
        assert m.mid_block.attentions[0].flash is True and m.mid_block.attentions[0].flash_split == 2
    vae = AutoencoderKL(sd_vae_config(block_out_channels=(32, 64)))
    for m in (vae.encoder, vae.decoder):
        assert m.mid_block.attentions[0].flash_split is None
