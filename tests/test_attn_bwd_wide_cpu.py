"""CPU: the wide-head reverse pass of attention (``tg_attention_bwd_wide`` / ``tg_attention_bwd_cross_wide``, 64 < head_dim <= 160;
csrc/tg_attention_bwd.hip) — what can be pinned without a device.

  * the header declares both symbols, ``_lib.SIGNATURES`` binds them, the library exports them, and the ABI version did not move (the change is
    additive);
  * host validation runs before any launch: every refusal of the header's list returns its documented code and sets ``tg_last_error``
    (fake non-null pointers, never read; stream NULL);
  * the fp32 model of the kernels (tests/test_attn_bwd_contract_cpu.py::model) passes the comparison of tests/attn_bwd_contract.py at the
    shapes and tolerances the GPU tests of the wide kernels use (1.5 x launch_check's per-launch bound, whole tensor and every block), and the
    fault a wide kernel is most likely to have — output columns >= 64 of a head never written — fails it at every wide head dim;
  * ``ops.attention_bwd_wide_supported``'s truth table; the routing switch ``backward.FLASH_BWD_WIDE`` is off by default.
"""
import ctypes as C
import os
import re

import pytest
import torch

from tests import attn_bwd_contract as ab
from tests import launch_check as lc
from tests.test_attn_bwd_contract_cpu import model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.bfloat16, torch.float16]
TG_ERR_ARG, TG_ERR_UNSUPPORTED = -1, -3
WEIGHT = 0.4


def tols(dtype):
    return 1.5 * lc.l2_tol(dtype), 1.5 * lc.rel_tol(dtype)


def test_tolerances_are_the_per_launch_attention_bound():
    assert tols(torch.bfloat16) == pytest.approx((4.5e-3, 1.5e-2)) and tols(torch.float16) == pytest.approx((6e-4, 3.75e-3))


# ---- symbols -------------------------------------------------------------------------------------------------------------------------
def test_wide_symbols_are_declared_bound_and_exported_at_abi_308():
    from theatergen_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "theatergen_hip.h")).read()
    declared = set(re.findall(r"^int\s+(tg_[a-z0-9_]+)\s*\(", header, flags=re.M))
    for name, desc in (("tg_attention_bwd_wide", "tg_attn_bwd_desc"), ("tg_attention_bwd_cross_wide", "tg_attn_bwd_cross_desc")):
        assert name in declared, f"{name} is not declared in the header"
        assert re.search(rf"^int {name}\(const {desc}\* d, void\* stream\);", header, flags=re.M), f"{name}: not the existing descriptor"
        assert name in _lib.SIGNATURES, f"{name} is not bound"
    assert _lib.SIGNATURES["tg_attention_bwd_wide"] == _lib.SIGNATURES["tg_attention_bwd"]
    assert _lib.SIGNATURES["tg_attention_bwd_cross_wide"] == _lib.SIGNATURES["tg_attention_bwd_cross"]
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    h = _lib.lib()
    assert h.tg_attention_bwd_wide is not None and h.tg_attention_bwd_cross_wide is not None
    assert re.search(r"#define TG_ABI_VERSION 308\b", header) and _lib.ABI_VERSION == 308 and h.tg_version() == 308


# ---- host validation -----------------------------------------------------------------------------------------------------------------
FAKE = 16                                                             # a non-null, 16-byte aligned "pointer": validation never reads it
SELF_PTRS = ("q", "k", "v", "dout", "qt", "kt", "doutt", "stats", "dq", "dk", "dv")
CROSS_PTRS = ("q", "dout", "k", "v", "kt", "stats", "dq")


def _self_desc(head_dim=80, n=64, heads=2, **over):
    from theatergen_amd import _lib
    d = _lib.AttnBwdDesc()
    d.dtype, d.batch, d.heads, d.head_dim, d.n = 0, 1, heads, head_dim, n
    for f in SELF_PTRS:
        setattr(d, f, FAKE)
    d.ld, d.bs, d.t_ld, d.t_bs, d.scale = heads * head_dim, n * heads * head_dim, n, heads * head_dim * n, head_dim ** -0.5
    for f, v in over.items():
        setattr(d, f, v)
    return d


def _cross_desc(head_dim=80, n_q=64, n_k=77, heads=2, **over):
    from theatergen_amd import _lib
    d = _lib.AttnBwdCrossDesc()
    inner, lp = heads * head_dim, (n_k + 7) // 8 * 8
    d.dtype, d.batch, d.heads, d.head_dim, d.n_q, d.n_k = 0, 1, heads, head_dim, n_q, n_k
    for f in CROSS_PTRS:
        setattr(d, f, FAKE)
    d.q_ld, d.q_bs, d.k_ld, d.k_bs, d.t_ld, d.t_bs = inner, n_q * inner, inner, n_k * inner, lp, inner * lp
    d.extra, d.extra_ld = FAKE, n_k
    d.scale, d.ds_scale = head_dim ** -0.5, 0.4 * head_dim ** -0.5
    for f, v in over.items():
        setattr(d, f, v)
    return d


def _refusals():
    """(what, descriptor factory, entry point, documented code) — the header's list"""
    out = []
    for hd in (64, 76, 168):
        out.append((f"self head_dim {hd}", lambda hd=hd: _self_desc(head_dim=hd), "tg_attention_bwd_wide", TG_ERR_UNSUPPORTED))
        out.append((f"cross head_dim {hd}", lambda hd=hd: _cross_desc(head_dim=hd), "tg_attention_bwd_cross_wide", TG_ERR_UNSUPPORTED))
    out.append(("self n = 60", lambda: _self_desc(n=60), "tg_attention_bwd_wide", TG_ERR_UNSUPPORTED))
    out.append(("self t_ld < n", lambda: _self_desc(t_ld=56), "tg_attention_bwd_wide", TG_ERR_ARG))
    out.append(("cross t_ld below the padded key count", lambda: _cross_desc(t_ld=72), "tg_attention_bwd_cross_wide", TG_ERR_ARG))
    out.append(("cross extra_ld < n_k", lambda: _cross_desc(extra_ld=76), "tg_attention_bwd_cross_wide", TG_ERR_ARG))
    for f in SELF_PTRS:
        out.append((f"self null {f}", lambda f=f: _self_desc(**{f: None}), "tg_attention_bwd_wide", TG_ERR_ARG))
    for f in CROSS_PTRS:
        out.append((f"cross null {f}", lambda f=f: _cross_desc(**{f: None}), "tg_attention_bwd_cross_wide", TG_ERR_ARG))
    return out


@pytest.mark.parametrize("what,make,entry,code", _refusals(), ids=[r[0] for r in _refusals()])
def test_host_validation_refuses_before_any_launch(what, make, entry, code):
    from theatergen_amd import _lib
    h = _lib.lib()
    assert h.tg_gemm(C.byref(_lib.GemmDesc()), None) == -1 and b"tg_gemm" in h.tg_last_error()      # another call's message, to be replaced
    rc = getattr(h, entry)(C.byref(make()), None)
    assert rc == code, f"{what}: returned {rc}, documented {code}"
    assert entry.encode() + b":" in h.tg_last_error(), f"{what}: tg_last_error is {h.tg_last_error()!r}"
    with pytest.raises(RuntimeError, match="theatergen_hip error"):
        _lib.check(rc)


def test_narrow_entry_points_keep_refusing_wide_heads():
    from theatergen_amd import _lib
    h = _lib.lib()
    assert h.tg_attention_bwd(C.byref(_self_desc(head_dim=80)), None) == TG_ERR_UNSUPPORTED and b"tg_attention_bwd:" in h.tg_last_error()
    assert h.tg_attention_bwd_cross(C.byref(_cross_desc(head_dim=80)), None) == TG_ERR_UNSUPPORTED


# ---- the fp32 model at the wide shapes -----------------------------------------------------------------------------------------------
# (kind, batch, n_q, n_k, heads, head_dim, q multiplier)
MODEL_CASES = [("self", 2, 136, 136, 3, 80, 1.0), ("self", 1, 264, 264, 2, 160, 1.0)] + \
              [("self", 1, 136, 136, 2, d, 1.0) for d in (72, 104, 136)] + \
              [("self", 1, 264, 264, 2, d, m) for d in (80, 160) for m in (4.0, 8.0)] + \
              [("cross", 2, 130, 77, 3, 80, 1.0), ("cross", 1, 264, 264, 2, 160, 4.0)]
_CASES = {}


def case(dtype, c):
    """descriptor + fp64 reference, built once and left unchanged"""
    if (dtype, c) not in _CASES:
        kind, B, nq, nk, H, D, qmul = c
        if kind == "self":
            a = ab.make_self_case(dtype, B, nq, H, D, qmul=qmul)
            ref = ab.self_reference(a)
        else:
            a = ab.make_cross_case(dtype, B, nq, nk, H, D, qmul=qmul, with_extra=True, weight=WEIGHT)
            ref = ab.cross_reference(a)
        _CASES[(dtype, c)] = (a, ref)
    return _CASES[(dtype, c)]


def _verdict(dtype, c, got):
    a, ref = case(dtype, c)
    l2, mx = tols(dtype)
    res = {x: ab.compare(got[x], ref[x], a["heads"], l2, mx) for x in got}
    for x, (ok, m) in res.items():
        print(f"{c} {str(dtype)[6:]} {x}: ok={ok} rel_l2={m['rel_l2']:.2e} max={m['max_rel']:.2e} block={m['block_rel_l2']:.2e}@{m['block_at']} "
              f"block_max={m['block_max_rel']:.2e}")
    return res


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", MODEL_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_fp32_model_passes_at_the_wide_shapes(dtype, c):
    a, _ = case(dtype, c)
    for x, (ok, m) in _verdict(dtype, c, model(a)).items():
        assert ok and m["finite"], f"{c} {x} {dtype}: {m}"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [72, 80, 104, 136, 160])
def test_unwritten_output_columns_past_64_fail_the_comparison(dtype, d):
    """the fault of a wide kernel that keeps the narrow one's two output tiles: columns >= 64 of every head's dK are zero"""
    c = ("self", 1, 136, 136, 2, d, 1.0)
    a, _ = case(dtype, c)
    got = model(a)
    dk = got["dk"].reshape(1, 136, 2, d)
    dk[..., 64:] = 0
    res = _verdict(dtype, c, got)
    assert not res["dk"][0], f"d={d}: zeroed columns passed {res['dk'][1]}"
    assert res["dq"][0] and res["dv"][0]


# ---- python surface ------------------------------------------------------------------------------------------------------------------
def test_wide_supported_truth_table_and_default_switch():
    from theatergen_amd import backward, ops
    for d, n, want in ((72, 64, True), (80, 1024, True), (96, 8, True), (104, 264, True), (160, 64, True), (160, 256, True),
                       (64, 64, False), (40, 1024, False), (8, 8, False), (76, 64, False), (168, 64, False), (320, 64, False),
                       (80, 60, False), (160, 1023, False)):
        assert ops.attention_bwd_wide_supported(d, n) is want, (d, n)
    # the narrow predicate is unchanged: the two never overlap
    for d in range(8, 200, 4):
        assert not (ops.attention_bwd_supported(d, 64) and ops.attention_bwd_wide_supported(d, 64))
    assert ops.attention_bwd_supported(64, 64) and not ops.attention_bwd_supported(80, 1024)
    if "TG_FLASH_BWD_WIDE" not in os.environ:
        assert backward.FLASH_BWD_WIDE is False
    assert callable(ops.attention_bwd_wide) and callable(ops.attention_bwd_cross_wide)
