"""CPU: the wide-head flash attention (``tg_attention_wide``, head_dim 256 / 512; csrc/tg_attention_wide.hip) — what can be pinned without a device.

  * the header declares the symbol with the EXISTING descriptor, ``_lib.SIGNATURES`` binds it, the library exports it (``nm -D``), and the ABI
    version did not move (the change is additive);
  * ``build.HOT_GATES`` has an entry for ``attention_wide_kernel<`` at 0 scratch bytes that matches kernels of the built object, and they pass it;
  * host validation runs before any launch: every refusal of the header's list returns its documented code and sets ``tg_last_error``
    (fake non-null pointers, never read; stream NULL);
  * the VAE switch: off by default, ``flash=True`` / ``TG_VAE_FLASH=1`` select the route for the channel counts that have a kernel only.
"""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TG_ERR_ARG, TG_ERR_UNSUPPORTED = -1, -3


def _lib_built():
    from theatergen_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib


def test_symbol_is_declared_bound_and_exported_at_abi_308():
    _lib = _lib_built()
    header = open(os.path.join(ROOT, "include", "theatergen_hip.h")).read()
    assert re.search(r"^int tg_attention_wide\(const tg_attn_desc\* d, void\* stream\);", header, flags=re.M), "not declared with the existing descriptor"
    assert "tg_attention_wide" in _lib.SIGNATURES and _lib.SIGNATURES["tg_attention_wide"] == _lib.SIGNATURES["tg_attention"]
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT tg_attention_wide$", nm, flags=re.M), "libtheatergen_hip.so does not export tg_attention_wide"
    assert _lib.lib().tg_attention_wide is not None
    assert re.search(r"#define TG_ABI_VERSION 308\b", header) and _lib.ABI_VERSION == 308 and _lib.lib().tg_version() == 308


def test_resource_gate_covers_the_wide_kernels_at_zero_scratch():
    from theatergen_amd import build
    _lib_built()
    gates = [g for g in build.HOT_GATES if g[0] == "attention_wide_kernel<"]
    assert len(gates) == 1 and gates[0][1] == 0, f"HOT_GATES entry for attention_wide_kernel<: {gates}"
    assert not any(g[0] in "attention_wide_kernel<" for g in build.HOT_GATES[:build.HOT_GATES.index(gates[0])]), "an earlier gate shadows it"
    if not os.path.exists(os.path.join(build.OBJ, "tg_attention_wide.o.res")):
        build.build(verbose=False)
    res = build.kernel_resources(verbose=False)
    mine = {n: r for n, r in res.items() if "attention_wide_kernel<" in n}
    assert {r["file"] for r in mine.values()} == {"tg_attention_wide.hip"}
    for want in ("attention_wide_kernel<bf16,256,", "attention_wide_kernel<f16,256,", "attention_wide_kernel<bf16,512,", "attention_wide_kernel<f16,512,"):
        assert any(n.startswith(want) for n in mine), f"no kernel {want}...> in the built object: {sorted(mine)}"
    for n, r in mine.items():
        assert r.get("scratch", 0) == 0 and r.get("vgpr_spill", 0) == 0, f"{n}: {r}"
    assert not [b for b in build.check_resources(res) if "attention_wide_kernel<" in b]


# ---- host validation -----------------------------------------------------------------------------------------------------------------
FAKE = 16                                                             # a non-null, 16-byte aligned "pointer": validation never reads it


def _desc(head_dim=512, heads=1, n_q=40, len0=72, **over):
    from theatergen_amd import _lib
    d = _lib.AttnDesc()
    inner = heads * head_dim
    d.dtype, d.batch, d.heads, d.head_dim, d.n_q, d.len0 = 0, 2, heads, head_dim, n_q, len0
    d.q = d.k0 = d.vt0 = d.out = FAKE
    d.q_ld, d.q_bs, d.k0_ld, d.k0_bs, d.vt0_ld, d.vt0_bs = inner, n_q * inner, inner, len0 * inner, len0, inner * len0
    d.out_ld, d.out_bs, d.scale = inner, n_q * inner, head_dim ** -0.5
    for f, v in over.items():
        setattr(d, f, v)
    return d


REFUSALS = [(f"head_dim {hd}", dict(head_dim=hd), TG_ERR_UNSUPPORTED) for hd in (64, 160, 192, 248, 384, 520, 1024)] + [
    ("len1 > 0", dict(len1=8, k1=FAKE, vt1=FAKE, k1_ld=512, vt1_ld=8), TG_ERR_UNSUPPORTED),
    ("causal", dict(causal=1), TG_ERR_UNSUPPORTED),
    ("mask", dict(mask=FAKE), TG_ERR_UNSUPPORTED),
    ("w1_dev", dict(w1_dev=FAKE), TG_ERR_UNSUPPORTED),
    ("bad dtype", dict(dtype=2), TG_ERR_ARG),
    ("batch 0", dict(batch=0), TG_ERR_ARG),
    ("n_q 0", dict(n_q=0), TG_ERR_ARG),
    ("len0 0", dict(len0=0), TG_ERR_ARG),
    ("len0 % 8", dict(len0=76), TG_ERR_ARG),
    ("scale 0", dict(scale=0.0), TG_ERR_ARG),
    ("q_ld % 8", dict(q_ld=516), TG_ERR_ARG),
    ("k0_ld % 8", dict(k0_ld=516), TG_ERR_ARG),
    ("vt0_ld % 8", dict(vt0_ld=76), TG_ERR_ARG),
    ("out_ld % 4", dict(out_ld=514), TG_ERR_ARG),
    ("q_bs % 8", dict(q_bs=40 * 512 + 4), TG_ERR_ARG),
    ("k0_bs % 8", dict(k0_bs=72 * 512 + 4), TG_ERR_ARG),
    ("vt0_bs % 8", dict(vt0_bs=512 * 72 + 4), TG_ERR_ARG),
    ("out_bs % 4", dict(out_bs=40 * 512 + 2), TG_ERR_ARG),
] + [(f"null {f}", {f: None}, TG_ERR_ARG) for f in ("q", "k0", "vt0", "out")]


@pytest.mark.parametrize("what,over,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_host_validation_refuses_before_any_launch(what, over, code):
    _lib = _lib_built()
    h = _lib.lib()
    assert h.tg_gemm(C.byref(_lib.GemmDesc()), None) == -1 and b"tg_gemm" in h.tg_last_error()      # another call's message, to be replaced
    rc = h.tg_attention_wide(C.byref(_desc(**over)), None)
    assert rc == code, f"{what}: returned {rc}, documented {code}"
    assert b"tg_attention_wide:" in h.tg_last_error(), f"{what}: tg_last_error is {h.tg_last_error()!r}"
    with pytest.raises(RuntimeError, match="theatergen_hip error"):
        _lib.check(rc)


def test_null_descriptor_and_the_narrow_entry_point():
    _lib = _lib_built()
    h = _lib.lib()
    assert h.tg_attention_wide(None, None) == TG_ERR_ARG
    assert h.tg_attention(C.byref(_desc(head_dim=512)), None) == TG_ERR_ARG and b"tg_attention:" in h.tg_last_error()    # still stops at 160


# ---- python surface ------------------------------------------------------------------------------------------------------------------
def test_vae_switch_is_off_by_default_and_selects_by_channel_count(monkeypatch):
    from theatergen_amd import ops
    from theatergen_amd.vae import AutoencoderKL, VAEAttention, sd_vae_config, tiny_vae_config
    assert callable(ops.attention_wide)
    monkeypatch.delenv("TG_VAE_FLASH", raising=False)
    assert VAEAttention(512).flash is None and not VAEAttention(512).flash_route()
    for c, want in ((32, True), (128, True), (160, True), (192, False), (256, True), (384, False), (512, True), (1024, False)):
        assert VAEAttention(c, flash=True).flash_route() is want, c
        assert VAEAttention(c, flash=False).flash_route() is False
    monkeypatch.setenv("TG_VAE_FLASH", "1")
    assert VAEAttention(512).flash_route() and VAEAttention(128).flash_route() and not VAEAttention(192).flash_route()
    assert not VAEAttention(512, flash=False).flash_route()                    # the attribute wins over the environment
    monkeypatch.setenv("TG_VAE_FLASH", "0")
    assert not VAEAttention(512).flash_route()
    monkeypatch.delenv("TG_VAE_FLASH")
    vae = AutoencoderKL(tiny_vae_config(), flash=True)
    assert vae.encoder.mid_block.attentions[0].flash is True and vae.decoder.mid_block.attentions[0].flash is True
    vae = AutoencoderKL(sd_vae_config(block_out_channels=(32, 64)))
    assert vae.encoder.mid_block.attentions[0].flash is None and vae.decoder.mid_block.attentions[0].flash is None
