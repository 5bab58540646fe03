"""GPU: hand-made edge launches of the five entries of csrc/tg_backward.hip (``tg_groupnorm_bwd`` on both of its kernels, ``tg_layernorm_bwd``,
``tg_geglu_bwd``, ``tg_softmax_bwd_rows``, ``tg_sumpool2x2``) against the fp64 restatement of their C-ABI contracts (tests/backward_contract.py).

The entries are called through ``theatergen_amd._lib`` directly, so the scratch, the alignment and the pitches are set by hand.  Every case, in
bf16 and fp16,
  * checks that every read and written region lies inside its storage and that no written element is read;
  * fills the output storages (guard rows and pad columns included) and the scratch with a sentinel byte first and checks that every byte
    outside the written region kept it;
  * compares with the restatement, whole tensor AND every block — (item, slab, group) on the slab path, (item, group) on the fallback, a row
    for LayerNorm / softmax / GEGLU, a pixel for the pool; GEGLU and the pool also element by element (``backward_contract.element_bound``);
  * replays once into NaN-filled outputs and NaN-filled scratch: same bits, no NaN (every element written, from the inputs alone).
Every element of an input buffer that the contract does not read holds NaN (pad columns of probs / dprobs / extra, guard rows), so a read
outside the contract shows in the outputs.

Tolerances (not tuned on the kernels): 1.5 x launch_check's per-launch bound — rel-L2 4.5e-3 (bf16) / 6e-4 (fp16), max error 1.5e-2 / 3.75e-3 of
the peak — for the whole tensor and for every block.  The fp32 models of the kernels pass every case here at these bounds, and every injected
fault fails (test_backward_contract_cpu.py).  The slab path at |mean| / std = 64 alone gets an allowance: twice the relative rstd error its
one-pass variance shows in the CPU model on the same operands.  Measured figures: profiles/backward_contract_findings.md.
"""
import pytest
import torch

from tests import backward_contract as bc
from tests import gemm_contract as gc
from tests import launch_check as lc
from tests import parity_metrics as pm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
SENTINEL = 0xA5
ALL_CASES = bc.all_cases()


def _name(dtype):
    return str(dtype).replace("torch.", "")


def launch(a):
    from theatergen_amd import _lib, ops
    L, p, e = _lib.lib(), ops._ptr, a["entry"]
    dt = ops._dt(torch.empty(0, dtype=bc.storage_dtype(a)))
    if e == "groupnorm":
        rc = L.tg_groupnorm_bwd(dt, p(a["x"]), p(a["dy"]), a["batch"], a["hw"], a["C"], a["groups"], a["eps"], p(a["gamma"]), p(a["beta"]), a["silu"],
                                p(a["dx"]), p(a["partials"]), ops._stream())
    elif e == "layernorm":
        rc = L.tg_layernorm_bwd(dt, p(a["x"]), p(a["dy"]), a["rows"], a["C"], a["eps"], p(a["gamma"]), p(a["dx"]), ops._stream())
    elif e == "geglu":
        rc = L.tg_geglu_bwd(dt, p(a["h"]), p(a["dg"]), a["rows"], a["inner"], p(a["dh"]), ops._stream())
    elif e == "softmax":
        rc = L.tg_softmax_bwd_rows(dt, p(a["probs"]), a["probs_fp32"], a["ld_probs"], p(a["dprobs"]), a["ld_dprobs"], p(a["extra"]), a["ld_extra"],
                                   a["rows"], a["length"], a["scale"], p(a["dscores"]), p(a["probs_out"]), a["ld_out"], ops._stream())
    else:
        rc = L.tg_sumpool2x2(dt, p(a["du"]), a["batch"], a["h"], a["w"], a["C"], p(a["out"]), ops._stream())
    torch.cuda.synchronize()
    return rc


def kernel_rstd_error(a):
    """largest relative error of the rstd the slab kernels formed, recomputed from the slab sums they left in the scratch"""
    B, hw, Cc, G = a["batch"], a["hw"], a["C"], a["groups"]
    part = [w for w in bc.written_region(a) if w.name == "partials"][0].view().double()
    inv_n = 1.0 / (float(hw) * (Cc // G))
    mean = part[..., 0].sum(1) * inv_n
    var = (part[..., 1].sum(1) * inv_n - mean * mean).clamp_min(0.0)
    rstd = (1.0 / torch.sqrt(var + bc._f32(a["eps"]))).float().double()
    want = bc.gn_group_stats(a)[1]
    return float(((rstd - want) / want).abs().max())


def run_case(cid, dtype, quiet=False):
    """the checks of this file on one launch -> {output: metrics}"""
    entry, kw = ALL_CASES[cid]
    a = bc.make_case(entry, dtype, device=DEV, **kw)
    what = f"backward edge {cid} {_name(dtype)}"
    reads, writes = bc.read_extents(a), bc.written_region(a)
    lc.LaunchChecker._check_reads(reads + writes, what)
    ref, mag = bc.reference(a), bc.reference(a, magnitude=True)
    masks = lc.LaunchChecker._write_masks(writes)
    lc.LaunchChecker._check_overlap(masks, reads, what)
    for t, _ in masks.values():
        lc._bytes(t).fill_(SENTINEL)
    snaps = lc.LaunchChecker._snapshot(masks)
    assert launch(a) == 0, what
    lc.LaunchChecker._check_outside(masks, snaps, what)
    first = {w.name: w.view().clone() for w in writes}
    fails, metrics = bc.judge(a, first, ref, mag)
    extra = {}
    if entry == "groupnorm" and bc.gn_path(a) == "slab":
        assert bool(torch.isfinite(first["partials"]).all()), f"{what}: non-finite slab sums"
        if a["R"] > 0:
            extra = {"kernel_rstd_err": kernel_rstd_error(a), "model_rstd_err": bc.gn_onepass_rstd_error(a)}
    for name, m in metrics.items():
        pm.record(f"{what} {name}", m, **extra)
        if not quiet or fails:
            print(f"{what} {name}: rel_l2={m['rel_l2']:.3e} max={m['max_rel']:.3e} block={m['block_rel_l2']:.3e}@{m['block_at']} "
                  f"block_max={m['block_max_rel']:.3e} {extra}")
    l2, mx = bc.tols(dtype)
    assert not fails, f"{what}: {fails} (tolerances rel-L2 {l2:.1e}, max {mx:.1e}, whole tensor and every block)"
    # replay: NaN everywhere the launch may write
    for t, _ in masks.values():
        gc._storage_tensor(t).fill_(float("nan"))
    assert launch(a) == 0, what
    for w in writes:
        again = w.view()
        assert not bool(torch.isnan(again).any()), f"{what}: {w.name} of the replay keeps NaN (an element was not written, or read stale memory)"
        bits = torch.int32 if w.t.dtype == torch.float32 else torch.int16
        assert torch.equal(again.contiguous().view(bits), first[w.name].contiguous().view(bits)), \
            f"{what}: {w.name} of the replay into NaN-filled buffers differs from the first launch"
    return metrics


# ---- tg_groupnorm_bwd ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("key", list(bc.GN_SLAB_CASES))
def test_groupnorm_slab_path(dtype, key):
    """one-row and ragged slabs, an empty last slab (3 x 1387), the batch cap (130 items: one slab), one and two chunk slots (2056, 2560, 4096),
    an idle thread row (24 channels), 256 thread rows (8 channels), 256 folding threads, and a constant group (zero variance, the clamp)"""
    entry, kw = bc.GN_SLAB_CASES[key]
    a = bc.make_case(entry, dtype, device=DEV, **kw)
    assert bc.gn_path(a) == "slab", bc.gn_fallback_reasons(a)
    if kw.get("const") is not None:
        it, grp, val = kw["const"]
        x = bc.read_extents(a)[0].view().reshape(kw["B"], kw["hw"], kw["groups"], -1)
        assert bool((x[it, :, grp] == val).all()) and float(x[it, :, grp + 1].float().std()) > 0.5
    run_case(f"gn-slab {key}", dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("key", list(bc.GN_FALLBACK_CASES))
def test_groupnorm_fallback_kernel(dtype, key):
    """each of the five conditions of tg_groupnorm_bwd that keep the one-workgroup-per-(item, group) kernel, one at a time"""
    (entry, kw), why = bc.GN_FALLBACK_CASES[key]
    a = bc.make_case(entry, dtype, device=DEV, **kw)
    assert bc.gn_fallback_reasons(a) == [why], bc.gn_fallback_reasons(a)
    run_case(f"gn-fallback {key}", dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("key", list(bc.GN_OFFSET_CASES))
def test_groupnorm_offset_operands(dtype, key):
    """x = R + N(0, 1): the slab path's one-pass variance at the normal bounds for R = 4 and 16, with the model's allowance at R = 64; the
    centred fallback kernel on the same operands at the normal bounds throughout"""
    entry, kw = bc.GN_OFFSET_CASES[key]
    a = bc.make_case(entry, dtype, device=DEV, **kw)
    assert bc.gn_path(a) == ("slab" if kw["scratch"] else "fallback")
    ex = bc.extra_tolerance(a)
    assert (ex > 0.0) == (kw["R"] == 64.0 and kw["scratch"]) and ex <= 2 * 6.6e-4
    x = bc.read_extents(a)[0].view().double()
    assert abs(float(x.mean()) - kw["R"]) < 0.05 and abs(float(x.std()) - 1.0) < 0.05
    run_case(f"gn-offset {key}", dtype)


# ---- tg_layernorm_bwd ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("key", list(bc.LN_CASES))
def test_layernorm(dtype, key):
    """fewer channels than lanes (8, 36), exactly 64, 320 and 1280, 4096, one channel (zero variance, dx = 0), gamma NULL, x = 16 + N(0, 1);
    row counts that leave waves of the last workgroup without a row"""
    m = run_case(f"ln {key}", dtype)["dx"]
    if key == "3x1":
        assert m["rel_l2"] == 0.0, "one channel: x - mean and gy - mean(gy) are exactly zero"


# ---- tg_geglu_bwd, tg_sumpool2x2 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("key", list(bc.GEGLU_CASES))
def test_geglu(dtype, key):
    """one element, the shape of the existing test, 1030 x 1024 = 1 054 720 elements (6 144 in the grid-stride trip), gates -8 .. 8"""
    entry, kw = bc.GEGLU_CASES[key]
    assert (kw["rows"] * kw["inner"] > bc.GRID_CAP_ELEMS) == (key == "1030x1024")
    assert run_case(f"geglu {key}", dtype)["dh"]["worst_over_element_bound"] <= 1.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("key", list(bc.POOL_CASES))
def test_sumpool2x2(dtype, key):
    """one element, odd sizes, 33 x 33 x 1024 = 1 115 136 elements (66 560 in the grid-stride trip)"""
    entry, kw = bc.POOL_CASES[key]
    assert (kw["B"] * kw["h"] * kw["w"] * kw["C"] > bc.GRID_CAP_ELEMS) == (key == "1x33x33x1024")
    assert run_case(f"pool {key}", dtype)["out"]["worst_over_element_bound"] <= 1.0


# ---- tg_softmax_bwd_rows ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", bc.SM_LENGTHS)
def test_softmax_rows(dtype, L):
    """rows 1 / 5 / 70 x ld_out roundup8(L) and + 16 x probs fp32 (pitch L + 5) or storage dtype x extra NULL or pitch L + 3 x probs_out NULL or
    not: 48 launches per length.  Pad columns of both outputs exactly zero (``judge``); the NaN in the input pads reaches no output."""
    cases = bc.softmax_cases(L)
    assert len(cases) == 48
    for key, (_, kw) in cases.items():
        m = run_case(f"softmax {key}", dtype, quiet=True)
        assert set(m) == ({"dscores", "probs_out"} if kw["probs_out"] else {"dscores"}) and all(v["finite"] for v in m.values())
        if L == 1:
            assert m["dscores"]["rel_l2"] == 0.0, "one key: P (dP - P dP) cancels to zero exactly"
