"""CPU: the conditions the bounds of tests/test_attn_fwd_edges_gpu.py rest on, and the teeth of its cases (tests/attn_fwd_contract.py).

Conditions, for every case of ``attn_fwd_contract.CASES`` and both dtypes:
  * the reference is finite and the schedule-faithful fp32 model is finite;
  * a second legitimate implementation — ``model(strict_max=True)``: a strict per-row running max, no FOLD rounding — lies inside the bound
    derived from the model (1.5x whole-tensor rel-L2, 1.5x worst block, 2x max-rel).  Cases that run FOLD are compared with the strict model
    that KEEPS FOLD's rounded query (``fold_rounding=True``): dropping the rounding that dominates FOLD's error would make the condition empty;
  * cases with N(0, 1)-scaled scores: the model meets the absolute figure of the suite, 1.5x launch_check's l2_tol / rel_tol, whole tensor
    and worst block.
Teeth: every fault of ``FAULT_CASE`` leaves the bound on its named case at bf16, the looser dtype; the cases a fault passes by accident are
asserted where the accident is exact (the faulted model is bit-equal) and tabled in profiles/attn_fwd_contract_findings.md.
``fold_ref_not_reset`` has NO catching case, and that is a property of the kernel, not a hole in the cases: segment 1 subtracts its own
maximum, so a stale FOLD reference r cancels; what is left is the fp32 rounding of ``score + r``, |r| 2^-24 exp2 units, visible at bf16 only from
|r| ~ 2^17 on — where FOLD's storage-dtype reference (off by up to |r| 2^-9) has long left exp2's range.  The test asserts the harmlessness.
"""
import pytest
import torch

from tests import attn_fwd_contract as af
from tests import launch_check as lc

DTYPES = [torch.bfloat16, torch.float16]
BF16 = torch.bfloat16

_cache = {}


def facts(name, dtype):
    """(descriptor, reference, model metrics), computed once per case and dtype and left unchanged"""
    key = (name, dtype)
    if key not in _cache:
        a = af.build(name, dtype)
        ref = af.reference(a)
        _cache[key] = (a, ref, af.compare(af.model(a), ref, a["heads"]))
    return _cache[key]


def _id(dtype):
    return str(dtype).replace("torch.", "")


# ---- the conditions -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("group", sorted({n.split(" ")[0] for n in af.CASES}))
def test_model_conditions(group, dtype):
    l2, mx = 1.5 * lc.l2_tol(dtype), 1.5 * lc.rel_tol(dtype)
    for name in [n for n in af.CASES if n.split(" ")[0] == group]:
        a, ref, mm = facts(name, dtype)
        assert bool(torch.isfinite(ref).all()) and mm["finite"], f"{name}: {mm}"
        fold = af.instance(a)[3]
        ms = af.compare(af.model(a, strict_max=True, fold_rounding=fold), ref, a["heads"])
        assert af.within(ms, af.bounds(mm)), f"{name} {dtype}: the strict-max model {ms} leaves the bound of the lazy model {mm}"
        if af.CASES[name]["kind"] == "normal":
            assert max(mm["rel_l2"], mm["block_rel_l2"]) <= l2 and mm["max_rel"] <= mx, f"{name} {dtype}: the model {mm} misses the absolute figure"


def test_instances():
    got = {af.instance(dict(head_dim=c["kw"]["d"], mask=c["kw"].get("mask"))) for n, c in af.CASES.items() if n.startswith("inst ")}
    assert got == af.ALL_INSTANCES and len(af.ALL_INSTANCES) == 17
    assert af.instance(dict(head_dim=40, mask=None)) == (48, 64, True, True, False)
    assert af.instance(dict(head_dim=40, mask=1)) == (48, 64, True, False, True) and af.instance(dict(head_dim=48, mask=None))[3] is False


def test_block_merge_rule():
    assert af.block_ranges(136) == [(0, 128), (128, 136)] and af.block_ranges(135) == [(0, 135)]
    assert af.block_ranges(129) == [(0, 129)] and af.block_ranges(257) == [(0, 128), (128, 257)] and af.block_ranges(1) == [(0, 1)]


def test_softmax_range_cases_enter_the_states_they_are_named_for():
    for dtype in DTYPES:
        for cls in ("fold", "ones", "plain", "mask"):
            seen = {}
            for what in ("late +7.5", "late +8.5", "late +200", "tile0 +200"):
                af.model(af.build(f"range {cls} {what}", dtype), info=seen.setdefault(what, {}))
            assert seen["late +7.5"]["rescales"] == 0 and 128 < seen["late +7.5"]["p_max"] <= 256, (cls, seen)      # P up to 2^7.5 = 181
            assert seen["late +8.5"]["rescales"] == 1 and seen["late +200"]["rescales"] == 1 and seen["tile0 +200"]["rescales"] == 0, (cls, seen)


def test_mask_rules_before_the_fix():
    """the MASK instance without the reference-0 and far-reference rules: NaN on exactly the rows whose first tile is all -inf (or finfo.min
    / scale = -inf) and on the rows masked with -1e30 throughout; with the rules every row is finite"""
    for name, rows in (("mask inf_tile0 d64", "tile0"), ("mask fmin d64", "tile0"), ("mask big_row d64", "third"), ("mask inf_part d64", None)):
        a, ref, mm = facts(name, BF16)
        pre = torch.isnan(af.model(a, inf_fix=False)).any(-1)
        want = torch.zeros_like(pre)
        if rows == "tile0":
            want[:] = True
            want[:, 4::5] = False
        elif rows == "third":
            want[:, ::3] = True
        assert torch.equal(pre, want), name
        assert mm["finite"]


# ---- teeth ---------------------------------------------------------------------------------------------------------------------------
FAULT_CASE = {
    "vt_tail": "inst d64 nomask", "drop_last_key": "len0 9 d64", "extra_key": "len0 9 d64", "causal_strict": "causal 77 d64",
    "causal_no_qblk": "causal 200 d64", "mask_qs_ignored": "mask layout 7 d64", "mask_hs_ignored": "mask layout 7 d64",
    "mask_bs_ignored": "mask layout 7 d64", "mask_no_inv_scale": "mask layout 7 d64", "mask_on_seg1": "inst d64 mask",
    "seg1_l0": "inst d64 nomask", "w1_on_seg0": "inst d64 nomask", "w1_dev0": "ps count 2 d64", "head_dpad": "inst d8 nomask",
    "qblk_rows": "inst d64 nomask", "no_rescale": "range plain late +200",
}
# cases a fault passes EXACTLY (the faulted model is the model): the state the fault lives in is not entered
ACCIDENTS = {
    "vt_tail": "len0 128 d64", "causal_no_qblk": "causal 77 d64", "mask_qs_ignored": "mask layout 6 d64", "mask_hs_ignored": "mask layout 5 d64",
    "mask_bs_ignored": "mask layout 3 d64", "mask_no_inv_scale": "mask zero d64", "mask_on_seg1": "mask layout 7 d64", "seg1_l0": "len1 0 d64",
    "w1_dev0": "ps count 1 d64", "head_dpad": "inst d64 nomask", "qblk_rows": "nq 128 d64", "no_rescale": "range plain late +7.5",
}


def test_every_fault_is_named():
    assert set(FAULT_CASE) | {"fold_ref_not_reset"} == set(af.FAULTS) and set(ACCIDENTS) <= set(FAULT_CASE)


@pytest.mark.parametrize("fault", sorted(FAULT_CASE))
def test_fault_fails_on_its_named_case(fault):
    name = FAULT_CASE[fault]
    a, ref, mm = facts(name, BF16)
    mf = af.compare(af.model(a, fault=fault), ref, a["heads"])
    assert not af.within(mf, af.bounds(mm)), f"{fault} passes {name}: {mf} inside the bound of {mm}"


@pytest.mark.parametrize("fault", sorted(ACCIDENTS))
def test_fault_passes_where_its_state_is_not_entered(fault):
    a, ref, mm = facts(ACCIDENTS[fault], BF16)
    assert torch.equal(af.model(a, fault=fault), af.model(a)), f"{fault} on {ACCIDENTS[fault]}"


def test_a_stale_fold_reference_in_segment_1_is_harmless():
    for name in ("inst d40 nomask", "range fold reference 2^12", "range fold x8"):
        for dtype in DTYPES:
            a, ref, mm = facts(name, dtype)
            assert af.instance(a)[3] and a["len1"] > 0
            mf = af.compare(af.model(a, fault="fold_ref_not_reset"), ref, a["heads"])
            assert af.within(mf, af.bounds(mm)) and mf["rel_l2"] <= 1.02 * mm["rel_l2"], (name, mf, mm)


def test_one_block_scaled_by_1_02_passes_the_whole_tensor_figure_and_fails_the_block_figure():
    """4 items x 4 heads x 8 query blocks = 128 units: one of them 2 % off moves the whole-tensor rel-L2 by 0.02 / sqrt(128) = 1.8e-3 in
    quadrature, inside 1.5x the model's 2.3e-3; in its own block it is 0.02, six times the block bound"""
    a = af.make_case(BF16, 4, 1024, 64, 4, 8, plain=True)
    ref = af.reference(a)
    out = af.model(a)
    mm = af.compare(out, ref, 4)
    bad = out.clone()
    bad[2, 384:512, 8:16] *= 1.02
    mb = af.compare(bad, ref, 4)
    bound = af.bounds(mm)
    assert mb["rel_l2"] <= bound[0], (mb, bound)
    assert mb["block_rel_l2"] > bound[1] and mb["block_at"] == [2, 1, 3] and not af.within(mb, bound), (mb, bound)


# ---- tg_attn_probs -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("d", [8, 40, 160])
def test_probs_model_sits_under_the_operation_count_bound(d, dtype):
    for length in (1, 63, 64, 65, 255, 256):
        for b0, tokens in ((0, None), (1, None), (1, [0, length - 1, length // 2, length - 1, min(1, length - 1)])):
            a = af.probs_case(dtype, 2, b0, 2, d, 5, length, tokens=tokens)
            ref, bound = af.probs_reference(a), af.probs_bound(a)
            assert tuple(ref.shape) == tuple(a["probs"].shape) == (2 - b0, 2, 5, length if tokens is None else 5)
            err = (af.probs_model(a) - ref).abs()
            assert bool((err <= bound).all()), f"len {length} d {d}: model / bound = {float((err / bound).max()):.3f}"
            # the bound has teeth: a worst-case count, linear in head_dim, yet under 1e-3 of p at head dim 160: a probability 1 % off fails by 10x
            assert float((bound / ref.clamp_min(1e-30))[ref > 1e-6].max()) < 1e-3
            if tokens is not None:
                full = af.probs_reference(dict(a, tokens=None, n_tokens=0))
                assert torch.equal(ref, full[..., tokens]) and torch.equal(ref[..., 1], ref[..., 3])


def test_probs_reference_skips_the_items_below_b0():
    a = af.probs_case(BF16, 3, 0, 2, 8, 5, 63)
    full = af.probs_reference(a)
    assert torch.equal(af.probs_reference(dict(a, b0=2)), full[2:])
