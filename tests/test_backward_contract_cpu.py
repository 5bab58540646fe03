"""CPU: pins tests/backward_contract.py (the fp64 restatements the GPU edge tests of csrc/tg_backward.hip compare against) and shows that the
comparison has teeth at the tolerances those tests use.

  * each restatement is fp64 autograd of F.group_norm (+ F.silu), F.layer_norm, a * F.gelu(g), softmax and 4 * avg_pool2d (1e-12);
  * the Python ``gnb_slabs`` and kernel choice give, for every GPU case, the slab counts and paths worked out by hand from the C rules;
  * the fp32 models of the kernels pass, on every GPU case and in both dtypes, the very ``judge`` the GPU test applies;
  * the same models with one fault injected fail it on at least one GPU case.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import backward_contract as bc

DTYPES = [torch.bfloat16, torch.float16]
BF16 = torch.bfloat16
CASES = bc.all_cases()


def _name(dtype):
    return str(dtype).replace("torch.", "")


@functools.lru_cache(maxsize=None)
def case(cid, dtype):
    """launch + fp64 reference + magnitude + the R = 64 allowance, built once per (case, dtype) and left unchanged"""
    entry, kw = CASES[cid]
    a = bc.make_case(entry, dtype, **kw)
    return a, bc.reference(a), bc.reference(a, magnitude=True), bc.extra_tolerance(a)


def verdict(cid, dtype, fault=None):
    a, ref, mag, ex = case(cid, dtype)
    return bc.judge(a, bc.model(a, fault), ref, mag, ex)


def test_tolerances_are_the_per_launch_attention_bound():
    assert bc.tols(torch.bfloat16) == pytest.approx((4.5e-3, 1.5e-2)) and bc.tols(torch.float16) == pytest.approx((6e-4, 3.75e-3))
    # one rounding of an fp32 value lies under the rel-L2 bound of a block of any size
    assert bc.unit_roundoff(torch.bfloat16) == 2.0 ** -8 < 4.5e-3 and bc.unit_roundoff(torch.float16) == 2.0 ** -11 < 6e-4


# ---- the restatements are autograd's formulas --------------------------------------------------------------------------------------------
def _close(got, ref, what):
    err = float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)
    assert err <= 1e-12, f"{what}: {err:.2e} of the peak"


@pytest.mark.parametrize("shape", [(2, 37, 320, 32, True), (1, 33, 320, 32, False), (2, 9, 24, 3, True), (1, 100, 36, 4, True)])
def test_groupnorm_restatement_is_fp64_autograd(shape):
    """C = 320 with 32 groups: 10-channel groups straddle the 8-channel chunks"""
    B, hw, Cc, G, silu = shape
    a = bc.make_case("groupnorm", torch.float16, B=B, hw=hw, C=Cc, groups=G, silu=silu, R=0.5)
    ext = {r.name: r.view().double() for r in bc.read_extents(a)}
    x = ext["x"].permute(0, 2, 1).clone().requires_grad_(True)                 # [B, C, hw]
    y = F.group_norm(x, G, ext["gamma"], ext["beta"], bc._f32(a["eps"]))
    y = F.silu(y) if silu else y
    want = torch.autograd.grad(y, x, ext["dy"].permute(0, 2, 1))[0].permute(0, 2, 1)
    _close(bc.reference(a)["dx"], want, f"groupnorm {shape}")


@pytest.mark.parametrize("rows,Cc,gamma", [(3, 36, True), (4, 320, True), (5, 320, False), (2, 8, True)])
def test_layernorm_restatement_is_fp64_autograd(rows, Cc, gamma):
    a = bc.make_case("layernorm", torch.bfloat16, rows=rows, C=Cc, gamma=gamma, R=1.0)
    ext = {r.name: r.view().double() for r in bc.read_extents(a)}
    x = ext["x"].clone().requires_grad_(True)
    want = torch.autograd.grad(F.layer_norm(x, (Cc,), ext.get("gamma"), None, bc._f32(a["eps"])), x, ext["dy"])[0]
    _close(bc.reference(a)["dx"], want, f"layernorm {(rows, Cc, gamma)}")


def test_layernorm_of_one_channel_is_exactly_zero():
    a = bc.make_case("layernorm", torch.float16, rows=3, C=1)
    assert float(bc.reference(a)["dx"].abs().max()) == 0.0 and float(bc.reference(a, magnitude=True)["dx"].abs().min()) > 0.0


@pytest.mark.parametrize("kw", [dict(rows=7, inner=33), dict(rows=1, inner=65, gate_sweep=True)])
def test_geglu_restatement_is_fp64_autograd(kw):
    a = bc.make_case("geglu", torch.float16, **kw)
    ext = {r.name: r.view().double() for r in bc.read_extents(a)}
    h = ext["h"].clone().requires_grad_(True)
    av, gt = h.chunk(2, dim=-1)
    want = torch.autograd.grad(av * F.gelu(gt), h, ext["dg"])[0]
    _close(bc.reference(a)["dh"], want, f"geglu {kw}")


@pytest.mark.parametrize("kw", [dict(rows=5, L=77, ld_out=96, probs_fp32=True, extra=True, probs_out=True),
                                dict(rows=70, L=8, ld_out=8, probs_fp32=False, extra=False, probs_out=False),
                                dict(rows=5, L=1, ld_out=24, probs_fp32=True, extra=True, probs_out=True)])
def test_softmax_restatement_is_fp64_autograd(kw):
    """P is an operand: any row of probabilities is softmax(log P + c), and d softmax / d scores at those scores is the row Jacobian"""
    a = bc.make_case("softmax", torch.bfloat16, **kw)
    ext = {r.name: r.view().double() for r in bc.read_extents(a)}
    L = kw["L"]
    P = ext["probs"] / ext["probs"].sum(-1, keepdim=True)                       # storage-dtype probabilities do not sum to one: autograd's
    s = torch.log(P).clone().requires_grad_(True)                               # softmax does, so it is compared on the normalised rows
    up = ext["dprobs"] + (ext["extra"] if "extra" in ext else 0.0)
    want = bc._f32(a["scale"]) * torch.autograd.grad(torch.softmax(s, -1), s, up)[0]
    got = bc.reference(dict(a, probs=P.contiguous(), ld_probs=L))
    if L == 1:
        assert float(got["dscores"].abs().max()) == 0.0 and float(want.abs().max()) <= 1e-15, "one key: dS cancels to zero"
    else:
        _close(got["dscores"][:, :L], want, f"softmax {kw}")
    assert kw["ld_out"] > L and float(got["dscores"][:, L:].abs().max()) == 0.0 or kw["ld_out"] == L
    if kw["probs_out"]:
        assert torch.equal(bc.reference(a)["probs_out"][:, :L], ext["probs"]) and float(bc.reference(a)["probs_out"][:, L:].abs().max()) == 0.0


def test_sumpool_restatement_is_fp64_autograd():
    a = bc.make_case("sumpool", torch.float16, B=2, h=3, w=5, C=7)
    du = bc.read_extents(a)[0].view().double()
    want = 4 * F.avg_pool2d(du.permute(0, 3, 1, 2), 2)
    _close(bc.reference(a)["out"], want.permute(0, 2, 3, 1), "sumpool2x2")
    # and it is the adjoint of the nearest x2 upsample
    x = torch.randn(2, 7, 3, 5, dtype=torch.float64, requires_grad=True)
    adj = torch.autograd.grad(F.interpolate(x, scale_factor=2, mode="nearest"), x, du.permute(0, 3, 1, 2))[0]
    _close(bc.reference(a)["out"], adj.permute(0, 2, 3, 1), "sumpool2x2 as the adjoint of the upsample")


def test_reference_reads_through_the_pitches_and_past_no_storage():
    """pad columns and guard rows hold NaN: a restatement that walked a wrong pitch returns NaN; one that reads past a storage raises"""
    for cid in ("softmax r5-L77-ld96-p32-ex-po", "gn-fallback 2x64x320g32-xshift4", "ln 3x36", "pool 2x3x5x7", "geglu 130x256"):
        a, ref, mag, _ = case(cid, BF16)
        assert all(bool(torch.isfinite(v).all()) for v in list(ref.values()) + list(mag.values())), cid
        for r in bc.read_extents(a):
            st = r.t.untyped_storage().nbytes() // r.t.element_size()
            assert r.view().numel() < st, f"{cid}: {r.name} has no guard"
    a = dict(case("softmax r5-L77-ld96-p32-ex-po", BF16)[0])
    a["rows"] = 8                                                               # three rows more than the buffers hold (two guard rows)
    with pytest.raises(RuntimeError):
        bc.reference(a)


# ---- slab count and kernel choice ------------------------------------------------------------------------------------------------------
def test_gnb_slabs_restates_the_c_rule():
    assert [bc.gnb_slabs(1, hw) for hw in (1, 31, 32, 33, 64, 65, 4096, 4097, 9216)] == [1, 1, 1, 2, 2, 3, 128, 128, 128]
    assert [bc.gnb_slabs(b, 1387) for b in (1, 2, 3, 4, 64, 65, 127, 128, 130)] == [44, 44, 42, 32, 2, 1, 1, 1, 1]
    # hw = 1387 at B = 3: 42 slabs of 34 rows, the last one starts past the map
    a, *_ = case("gn-slab 3x1387x64g32", BF16)
    S, rows_per, TC, TR = bc.gn_slab_geometry(a)
    assert (S, rows_per, TC, TR) == (42, 34, 8, 32) and (S - 1) * rows_per == 1394 >= 1387 > (S - 2) * rows_per
    ids, grid = bc.blocks(a)
    assert grid == (3, 42, 32) and int(ids.max()) == (2 * 42 + 40) * 32 + 31, "no element belongs to the empty slab"


def test_scratch_bytes_agree_with_the_library():
    import os
    from theatergen_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    L = _lib.lib()
    for cid, (entry, kw) in CASES.items():
        if entry == "groupnorm":
            assert L.tg_groupnorm_bwd_scratch_bytes(kw["B"], kw["hw"], kw["groups"]) == 4 * bc.gn_scratch_floats(kw["B"], kw["hw"], kw["groups"]), cid


SLAB_GEOMETRY = {                                                               # (nslab, rows per slab, TC, TR) by hand from the C rules
    "1x1x64g32": (1, 1, 8, 32), "1x31x320g32": (1, 31, 40, 6), "1x33x320g32": (2, 17, 40, 6), "3x1387x64g32": (42, 34, 8, 32),
    "130x40x64g32": (1, 40, 8, 32), "1x144x2560g32": (5, 29, 256, 1), "1x40x2056g8": (2, 20, 256, 1), "1x40x4096g32": (2, 20, 256, 1),
    "2x100x24g3": (4, 25, 3, 85), "1x300x8g2-nosilu": (10, 30, 1, 256), "1x64x512g256": (2, 32, 64, 4), "2x577x640g32-const": (19, 31, 80, 3),
}


@pytest.mark.parametrize("dtype", DTYPES)
def test_path_choice_of_every_gpu_case(dtype):
    assert set(SLAB_GEOMETRY) == set(bc.GN_SLAB_CASES)
    for k in bc.GN_SLAB_CASES:
        a, *_ = case(f"gn-slab {k}", dtype)
        assert bc.gn_path(a) == "slab" and bc.gn_slab_geometry(a) == SLAB_GEOMETRY[k], (k, bc.gn_fallback_reasons(a), bc.gn_slab_geometry(a))
        assert [r.name for r in bc.written_region(a)] == ["dx", "partials"]
        assert bc.written_region(a)[1].view().numel() == a["partials"].numel(), "the scratch is exactly tg_groupnorm_bwd_scratch_bytes"
    for k, (_, why) in bc.GN_FALLBACK_CASES.items():
        a, *_ = case(f"gn-fallback {k}", dtype)
        assert bc.gn_fallback_reasons(a) == [why], (k, bc.gn_fallback_reasons(a))
        assert [r.name for r in bc.written_region(a)] == ["dx"]
    for k, (_, kw) in bc.GN_OFFSET_CASES.items():
        a, *_ = case(f"gn-offset {k}", dtype)
        assert bc.gn_path(a) == ("slab" if kw["scratch"] else "fallback"), k


def test_one_pass_variance_loses_what_the_issue_says():
    """relative rstd error of the slab path's E[x^2] - mean^2 on x = R + N(0, 1): at most 1e-7 at R = 0, 4e-5 up to R = 16, 6.6e-4 at R = 64
    (above the fp16 single-launch rel-L2 bound of 4e-4); the allowance of the R = 64 slab cases is twice the model's own figure"""
    errs = {}
    for R in (0, 4, 16, 64):
        a = bc.make_case("groupnorm", torch.float16, B=1, hw=1024, C=320, groups=32, R=float(R))
        errs[R] = bc.gn_onepass_rstd_error(a)
        assert bc.extra_tolerance(a) == (2 * errs[R] if R == 64 else 0.0)
    print(errs)
    assert errs[0] <= 1e-7 and errs[4] <= 4e-5 and errs[16] <= 4e-5 and errs[64] <= 6.6e-4
    a = bc.make_case("groupnorm", torch.float16, B=1, hw=1024, C=320, groups=32, R=64.0, scratch=False)
    assert bc.extra_tolerance(a) == 0.0, "the centred fallback gets the normal bound"


# ---- a correct implementation passes ---------------------------------------------------------------------------------------------------
FAMILIES = sorted({cid.split(" ")[0] for cid in CASES})


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", FAMILIES)
def test_fp32_model_passes_every_gpu_case(family, dtype):
    bad = []
    for cid in CASES:
        if cid.split(" ")[0] != family:
            continue
        fails, metrics = verdict(cid, dtype)
        for name, m in metrics.items():
            if family != "softmax":
                print(f"{cid} {_name(dtype)} {name}: rel_l2={m['rel_l2']:.2e} max={m['max_rel']:.2e} block={m['block_rel_l2']:.2e}@{m['block_at']} "
                      f"block_max={m['block_max_rel']:.2e} tol={m['l2_tol']:.2e}")
        bad += [f"{cid}: {f}" for f in fails]
    assert not bad, "\n".join(bad)


# ---- injected faults -------------------------------------------------------------------------------------------------------------------
# fault -> a GPU case (bf16, the looser dtype) at which it must FAIL
FAULT_CASES = {
    "phase0_drops_last_row": "gn-slab 1x33x320g32",
    "fold_drops_last_slab": "gn-slab 1x33x320g32",                   # 16 of 33 rows missing from every sum
    "group_of_chunk_head": "gn-slab 1x31x320g32",
    "no_silu_grad": "gn-slab 1x144x2560g32",
    "no_gamma": "ln 4x320",
    "m2_wrong_count": "gn-slab 1x40x4096g32",
    "softmax_pads_unwritten": "softmax r5-L77-ld96-p32-ex-po",
    "softmax_sum_without_extra": "softmax r70-L264-ld264-pst-ex-nopo",
    "grid_stride_tail_dropped": "geglu 1030x1024",
    "pool_second_tap_twice": "pool 2x3x5x7",
}


def test_every_fault_of_the_issue_is_listed():
    assert set(FAULT_CASES) == set(bc.FAULTS) and len(bc.FAULTS) == 10


@pytest.mark.parametrize("fault", sorted(FAULT_CASES))
def test_injected_fault_fails(fault):
    fails, metrics = verdict(FAULT_CASES[fault], BF16, fault)
    print(fault, metrics)
    assert fails, f"{fault} passed on {FAULT_CASES[fault]}: {metrics}"
    assert not verdict(FAULT_CASES[fault], BF16)[0]


def test_fold_over_one_slab_too_few_fails_wherever_the_last_slab_holds_rows():
    """hw = 1387 at B = 3 is the one case whose last slab is empty: a fold over nslab - 1 slabs is right there by accident, and wrong on
    every other multi-slab case"""
    assert not verdict("gn-slab 3x1387x64g32", BF16, "fold_drops_last_slab")[0]
    for k, geo in SLAB_GEOMETRY.items():
        if k != "3x1387x64g32":
            assert verdict(f"gn-slab {k}", BF16, "fold_drops_last_slab")[0], k


def test_more_faults_fail_where_only_one_case_sees_them():
    assert verdict("gn-slab 2x577x640g32-const", BF16, "group_of_chunk_head")[0]
    assert verdict("gn-slab 2x100x24g3", BF16, "no_gamma")[0] and verdict("gn-fallback 1x100x36g4", BF16, "no_silu_grad")[0]
    assert verdict("pool 1x33x33x1024", BF16, "grid_stride_tail_dropped")[0]
    # 8-channel groups on chunk boundaries: taking the group of the chunk's first channel is right there
    assert not verdict("gn-slab 2x100x24g3", BF16, "group_of_chunk_head")[0]
    # the tail of the grid-stride trip is one block among 1030 rows: the whole-tensor figure alone would pass it
    fails, metrics = verdict("geglu 1030x1024", BF16, "grid_stride_tail_dropped")
    assert metrics["dh"]["block_rel_l2"] > 0.7 and metrics["dh"]["block_at"][0] >= 1024


def test_a_fault_confined_to_one_slab_and_group_shows_in_the_block_figure():
    """2 % of the peak added to one (item, slab, group) of 3 x 42 x 32: the whole-tensor figures pass, the block's do not"""
    a, ref, mag, ex = case("gn-slab 3x1387x64g32", BF16)
    out = {k: v.clone() for k, v in bc.model(a).items()}
    ids, grid = bc.blocks(a)
    target = (1 * 42 + 17) * 32 + 9
    out["dx"][ids == target] += (0.02 * float(ref["dx"].abs().max()))
    fails, metrics = bc.judge(a, out, ref, mag, ex)
    m = metrics["dx"]
    l2, mx = bc.tols(BF16)
    assert fails and m["block_at"] == [1, 17, 9] and m["rel_l2"] <= l2 and m["block_rel_l2"] > l2
