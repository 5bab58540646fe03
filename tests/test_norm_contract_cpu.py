"""CPU: pins tests/norm_contract.py (the fp64 restatements, plans and fp32 models the GPU edge test of csrc/tg_norm.hip and csrc/tg_layernorm_add.hip
compares against) and shows that the comparison has teeth at the bounds that test uses.

  * the restatements are torch's fp64 group_norm (+ silu) / layer_norm; they read through the pitches of the call and past no storage;
  * ``plan`` gives, for the named GPU cases, the geometry worked out by hand from the C gates, agrees with ``tg_groupnorm_scratch_bytes``, and every case
    passes the restated host checks; every refusal row of the GPU test returns TG_ERR_ARG from the library itself (a refusal needs no GPU);
  * the fp32 models pass every GPU case in both dtypes through the very ``judge`` the GPU test applies, fp32 outputs inside the derived bounds;
  * each fault of ``norm_contract.FAULTS``, injected into the model, fails it on a named GPU case in bf16; where one passes by accident that is asserted too;
  * 2 % of the peak confined to one block passes the whole-tensor figures and fails the block figure;
  * the one-pass variance of the two-launch path by |mean| / std, model against fp64 and against the floor.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import norm_contract as nc
from tests.gemm_contract import _storage_tensor

DNAMES = list(nc.DTYPES)


def verdict(cid, dname, fault=None):
    a, ref, mod, fig, bnd, elem = nc.case_data(cid, dname)
    return nc.judge(a, mod if fault is None else nc.model(a, fault), ref, bnd, elem, cid)


# ---- the restatements ---------------------------------------------------------------------------------------------------------------------
def _close(got, want, what):
    err = float((got - want).abs().max()) / max(float(want.abs().max()), 1e-300)
    assert err <= 1e-12, f"{what}: {err:.2e} of the peak"


@pytest.mark.parametrize("cid", ["gn-two 1x9x24+16g4", "gn-two 1x40x8g2-nobeta", "gn-two 2x264x320g32-bare", "gn-small 3x250x64g8-nogamma", "gn-small 1x64x40+24g4",
                                 "gn-two 1x300x64g32-eps"])
def test_groupnorm_restatement_is_torch_fp64(cid):
    a = nc.make_case(cid, torch.float16)
    ext = nc._ext(a)
    x = nc._x(ext, a).double().permute(0, 2, 1)
    g, b = (ext[k].double() if k in ext else None for k in ("gamma", "beta"))
    y = F.group_norm(x, a["groups"], g, b, nc._f32(a["eps"]))
    _close(nc.reference(a)["out"], (F.silu(y) if a["silu"] else y).permute(0, 2, 1), cid)


def test_coefficients_applied_are_the_normalised_tensor():
    a = nc.make_case("gn-two coef-2x264x24+16g4", torch.bfloat16)
    ext = nc._ext(a)
    cf = nc.reference(a)["coef"]
    x = nc._x(ext, a).double()
    y = F.group_norm(x.permute(0, 2, 1), a["groups"], None, ext["beta"].double(), nc._f32(a["eps"])).permute(0, 2, 1)
    _close(x * cf[:, 0][:, None] + cf[:, 1][:, None], y, "x a + d")


@pytest.mark.parametrize("cid", ["ln 33x200-nogamma-nobeta-pitch", "ln 17x328-nobeta-pitch", "ln 33x72-nogamma", "ln 9x1280", "ln-add 9x648-m16-pitch"])
def test_layernorm_restatement_is_torch_fp64(cid):
    a = nc.make_case(cid, torch.bfloat16)
    ext = nc._ext(a)
    x = ext["x"].double() + (ext["res"].double() if "res" in ext else 0.0)
    g, b = (ext[k].double() if k in ext else None for k in ("gamma", "beta"))
    _close(nc.reference(a)["out"], F.layer_norm(x, (a["C"],), g, b, nc._f32(a["eps"])), cid)
    if "res" in ext:
        return
    st = nc.reference(dict(a, entry="layernorm_stats"))["stats"]
    _close((x * st[:, :1] + st[:, 1:]) * (g if g is not None else 1.0) + (b if b is not None else 0.0), nc.reference(a)["out"], cid + " through stats")


def test_partials_restatement_takes_the_statistics_from_the_partials():
    a = nc.make_case("gn-partials n7-b2-apply", torch.float16)
    st = nc.gn_stats64(a)
    b = dict(a, entry="groupnorm", c0=320, c1=0, x1=None, x0=a["x"])
    want = nc.gn_stats64(b)                                                     # the same x: each 64-pixel sum is rounded once to fp32
    assert float(((st["mean"] - want["mean"]).abs() / want["m1"]).max()) <= 2 * nc.U and float(((st["var"] - want["var"]).abs() / want["m2"]).max()) <= 4 * nc.U


def test_reference_reads_through_the_pitches_and_past_no_storage():
    for cid in ("ln 17x328-nobeta-pitch", "ln-add 9x648-m16-pitch", "gn-two 1x9x24+16g4", "gn-partials n7-b2-apply", "gn-two 2x64x512g32-gshift"):
        a, ref, *_ = nc.case_data(cid, "bf16")
        assert all(bool(torch.isfinite(v).all()) for v in ref.values()), cid
        # everything the contract does not read is NaN
        for r in nc.read_extents(a):
            flat = _storage_tensor(r.t)
            assert r.view().numel() < flat.numel(), f"{cid}: {r.name} has no guard"
            mask = torch.zeros(flat.numel(), dtype=torch.bool)
            mask.as_strided(r.sizes, r.strides, r.storage_byte_offset() // r.esize).fill_(True)
            assert bool(torch.isnan(flat[~mask]).all()) and bool(torch.isfinite(flat[mask]).all()), (cid, r.name)
    a = dict(nc.case_data("ln 17x328-nobeta-pitch", "bf16")[0])
    a["rows"] = 20                                                              # three rows more than the buffer holds (two guard rows)
    with pytest.raises(RuntimeError):
        nc.reference(a)


# ---- plans --------------------------------------------------------------------------------------------------------------------------------
TWO = lambda n, per, cx, ry, slots, lds, **k: dict(path="two-launch", gn_nblk=n, per=per, cx=cx, ry=ry, slots=slots, lds_bytes=lds, **k)
SMALL = lambda gpb, nc_, npy, maxp, MAXP: dict(path="small", gpb=gpb, nc=nc_, npy=npy, maxp=maxp, MAXP=MAXP)
PLANS = {                                                                       # by hand from gn_small_plan / gn_nblk / groupnorm_impl
    "gn-two 1x300x320g32": TWO(37, 9, 40, 6, 1, 15360, why="hw > 256"),
    "gn-two 16x300x64g32": TWO(32, 10, 8, 32, 1, 16384),
    "gn-two 3x1387x64g32": TWO(170, 9, 8, 32, 1, 16384, why="hw > 256"),
    "gn-two 1x9x24+16g4": TWO(1, 9, 5, 51, 1, 16320, npart=1),
    "gn-two 1x264x8g1-nogamma": TWO(33, 8, 1, 256, 1, 16384, why="hw > 256"),
    "gn-two 1x40x8g2-nobeta": TWO(5, 8, 1, 256, 1, 16384, why="channels per group not a multiple of 8"),
    "gn-two 1x264x2056g8": TWO(33, 8, 256, 1, 2, 16448),
    "gn-two 1x257x8192g32": TWO(32, 9, 256, 1, 4, 65536),
    "gn-two 1x675x1024g32": TWO(84, 9, 128, 2, 1, 16384),
    "gn-two 1x64x512g256": TWO(8, 8, 64, 4, 1, 16384, stat_trips=8, why="channels per group not a multiple of 8"),
    "gn-two 1x264x320g40": TWO(33, 8, 40, 6, 1, 15360, stat_trips=2),
    "gn-two 2x577x640g32-const": TWO(72, 9, 80, 3, 1, 15360),
    "gn-two 2x64x512g32-gshift": TWO(8, 8, 64, 4, 1, 16384, why="gamma / beta not 16-byte aligned"),
    "gn-two 1x64x272g34": TWO(8, 8, 34, 7, 1, 15232, why="groups per block > 16"),
    "gn-two 1x256x512g2": TWO(32, 8, 64, 4, 1, 16384, why="pixels per lane > 24"),
    "gn-two 1x16x2056g1": TWO(2, 8, 256, 1, 2, 16448, why="chunk columns > 256"),
    "gn-offset 1024x320-R64": TWO(128, 8, 40, 6, 1, 15360),
    "gn-offset 288x2560-R64": TWO(36, 8, 256, 1, 2, 20480),
    "gn-small 2x64x512g32": SMALL(4, 8, 32, 2, 3),
    "gn-small 1x160x128g4": SMALL(2, 8, 32, 5, 6),
    "gn-small 1x256x320g4": SMALL(1, 10, 25, 11, 12),
    "gn-small 1x256x1024g8": SMALL(1, 16, 16, 16, 24),
    "gn-small 3x250x64g8-nogamma": SMALL(8, 8, 32, 8, 12),
    "gn-small 1x100x80g10": SMALL(10, 10, 25, 4, 6),
    "gn-small 1x7x8g1": SMALL(1, 1, 256, 1, 3),
    "gn-small 2x1x64g8": SMALL(8, 8, 32, 1, 3),
    "gn-small 1x64x40+24g4": SMALL(4, 8, 32, 2, 3),
    "gn-small coef-2x64x512g32": SMALL(4, 8, 32, 2, 3),
    "gn-partials n7-b2-apply": dict(path="partials-apply", gn_nblk=50, per=8, npart=7),
    "gn-partials n70-apply": dict(path="partials-apply", gn_nblk=512, per=9, npart=70),
    "gn-partials n1-coef": dict(path="partials-coef", gn_nblk=5, npart=1),
    "gn-partials n9-coef": dict(path="partials-coef", gn_nblk=65, npart=9),
}
LN_INSTANCES = {8: (8, 1), 64: (8, 1), 72: (8, 5), 200: (8, 5), 320: (8, 5), 328: (16, 5), 640: (16, 5), 648: (32, 5), 1280: (32, 5), 1288: (64, 4),
                2048: (64, 4), 2056: (64, 8), 4096: (64, 8)}


@pytest.mark.parametrize("dname", DNAMES)
def test_plan_of_the_named_cases(dname):
    for cid, want in PLANS.items():
        pl = nc.plan(nc.case_data(cid, dname)[0])
        assert {k: pl.get(k) for k in want} == want, (cid, pl)
    two = [cid for cid in nc.ALL if cid.startswith(("gn-two", "gn-offset"))]
    assert all(nc.plan(nc.case_data(cid, dname)[0])["path"] == "two-launch" for cid in two)
    assert all(nc.plan(nc.case_data(cid, dname)[0])["path"] == "small" for cid in nc.ALL if cid.startswith("gn-small"))
    assert {nc.plan(nc.case_data(cid, dname)[0])["MAXP"] for cid in nc.ALL if cid.startswith("gn-small")} == {3, 6, 12, 24}
    assert {nc.plan(nc.case_data(cid, dname)[0])["gpb"] for cid in nc.ALL if cid.startswith("gn-small")} >= {1, 2, 4, 8, 10}
    refusals = {nc.plan(nc.case_data(cid, dname)[0]).get("why") for cid in two}
    assert refusals >= {"hw > 256", "channels per group not a multiple of 8", "groups per block > 16", "chunk columns > 256", "pixels per lane > 24",
                        "gamma / beta not 16-byte aligned"}
    for fam, add in (("ln", False), ("ln-stats", False), ("ln-add", True)):
        seen = set()
        for k in nc.CASES[fam]:
            a = nc.case_data(f"{fam} {k}", dname)[0]
            pl = nc.plan(a)
            assert (pl["LPR"], pl["MAXC"]) == LN_INSTANCES[a["C"]], (fam, k)
            seen.add((pl["LPR"], pl["MAXC"], a["rows"] > pl["rows_per_block"]))
        assert {s[:2] for s in seen} == set(LN_INSTANCES[c] for c in LN_INSTANCES if not add or c <= 1280), fam
        assert all((l, m, True) in seen for l, m, _ in seen), f"{fam}: every instance runs with one row more than a block holds"
    # from_partials: the producer's block count is never the apply pass's
    for k in nc.GN_PARTIALS:
        a = nc.case_data(f"gn-partials {k}", dname)[0]
        assert a["nblk"] != nc.gn_nblk(a["batch"], a["hw"]) and a["hw"] % 64


def test_slab_shapes_enter_the_trip_the_remainder_and_the_empty_slab():
    """per-thread-row pixel counts of the two-launch cases: 4-pixel trips, remainders, both in one row, idle rows, empty slabs"""
    seen = set()
    for cid in nc.ALL:
        if not cid.startswith(("gn-two", "gn-offset", "gn-partials")):
            continue
        a = nc.case_data(cid, "bf16")[0]
        pl = nc.plan(a)
        for blk in range(pl.get("gn_nblk", 0)):
            n = min((blk + 1) * pl["per"], a["hw"]) - blk * pl["per"]
            if n <= 0:
                seen.add("empty slab")
                continue
            for ty in range(pl["ry"]):
                k = max((n - ty + pl["ry"] - 1) // pl["ry"], 0)
                seen.add("idle row" if k == 0 else "trip + remainder" if k >= 4 and k % 4 else "trips only" if k >= 4 else "remainder only")
    assert seen == {"empty slab", "idle row", "trip + remainder", "trips only", "remainder only"}


def _lib():
    import os
    from theatergen_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.lib()


def test_scratch_bytes_and_host_checks_agree_with_the_library():
    L = _lib()
    for cid, k in nc.ALL.items():
        a = nc.case_data(cid, "bf16")[0]
        assert nc.host_check_failures(a) == [], (cid, nc.host_check_failures(a))
        if k["entry"] in ("groupnorm", "groupnorm_coef"):
            assert L.tg_groupnorm_scratch_bytes(k["B"], k["hw"], k["groups"]) == 4 * nc.gn_scratch_floats(k["B"], k["hw"], k["groups"]) == 4 * a["partials"].numel(), cid
    for B, hw in ((1, 1), (1, 7), (1, 8), (1, 4095), (1, 4096), (1, 5000), (2, 4096), (3, 1387), (512, 64), (513, 64), (600, 9)):
        assert L.tg_groupnorm_scratch_bytes(B, hw, 32) == 4 * nc.gn_scratch_floats(B, hw, 32), (B, hw)


def test_every_refusal_row_is_refused_by_the_library_and_by_the_restated_checks():
    """a refusal returns before any HIP call: the table of the GPU test runs here on made-up, never dereferenced addresses"""
    from tests import test_norm_edges_gpu as edges
    L = _lib()
    for entry in edges.BASE:
        base = edges.base_call(entry, lambda nbytes: 0x7f0000000000)
        assert nc.host_check_failures(edges.as_launch(entry, base)) == [], entry
    for entry, label, change in edges.REFUSALS:
        call = edges.base_call(entry, lambda nbytes: 0x7f0000000000)
        call.update(change(call) if callable(change) else change)
        assert nc.host_check_failures(edges.as_launch(entry, call)), f"{entry} {label}: the restated checks accept it"
        assert edges.run_call(L, entry, call, stream=None) == edges.ERR_CODES.get(label, edges.ERR_ARG), f"{entry} {label}"


# ---- a correct implementation passes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", DNAMES)
@pytest.mark.parametrize("family", list(nc.CASES))
def test_fp32_model_passes_every_gpu_case(family, dname):
    bad = []
    for k in nc.CASES[family]:
        cid = f"{family} {k}"
        fails, fig = verdict(cid, dname)
        a, ref, mod, mfig, bnd, elem = nc.case_data(cid, dname)
        for name, f in fig.items():
            tail = f"worst element / bound {f[5]:.3f}" if len(f) > 5 else f"floor {floor_of(cid, dname):.3e}"
            print(f"{cid} {dname} {name}: rel-L2 {f[0]:.3e} block {f[1]:.3e}@{f[4]} max-rel {f[2]:.3e} chain {nc.plan(a)['chain']} {tail}")
            if len(f) > 5:
                assert f[5] <= 0.9, f"{cid}: the model should sit well inside a worst-case bound"
        bad += fails
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("dname", DNAMES)
def test_the_bounds_are_tighter_than_the_tolerance_of_the_existing_tests(dname):
    """test_groupnorm / test_layernorm allow rel-L2 3e-3 / 4e-4 and max-rel 1e-2 / 2.5e-3 against fp32 torch: every bound here is below that"""
    l2, mx = nc.old_tolerance(nc.DTYPES[dname])
    for cid in nc.ALL:
        bnd = nc.case_data(cid, dname)[4]
        for name, b in bnd.items():
            if name == "out":
                assert b[0] <= l2 and b[2] <= mx, (cid, b)


@functools.lru_cache(maxsize=None)
def floor_of(cid, dname):
    a, ref, *_ = nc.case_data(cid, dname)
    return nc.figures(a, {"out": ref["out"].to(nc.DTYPES[dname])}, ref)["out"][0]


@pytest.mark.parametrize("dname", DNAMES)
def test_two_pass_paths_sit_on_the_floor_when_the_mean_dwarfs_the_deviation(dname):
    """LayerNorm, layernorm_add and the small GroupNorm path at mean 8 / std 0.125 and mean 16 / std 0.0625: the model's rel-L2 is the floor's (the fp64
    result rounded once) within 5 %.  No allowance anywhere."""
    for cid in ("ln 17x320-m8-pitch", "ln 9x1280-m16", "ln-add 17x320-m8", "ln-add 9x648-m16-pitch", "gn-small 1x256x320g4-m8", "gn-small 2x250x64g8-m16"):
        a, ref, mod, fig, bnd, _ = nc.case_data(cid, dname)
        assert nc.extra_tolerance(a) == 0.0
        assert fig["out"][0] <= 1.05 * floor_of(cid, dname), (cid, fig["out"][0], floor_of(cid, dname))


def onepass_table(dname, shape=(1024, 320)):
    """R -> (model rel-L2, fp64-rounded-once floor, model's worst relative rstd error) of the two-launch path on x = 16 + N(0, (16 / R)^2)"""
    rows = {}
    for R in (4, 16, 64, 256):
        cid = f"gn-offset {shape[0]}x{shape[1]}-R{R}"
        if cid in nc.ALL:
            a, ref, mod, fig, _, _ = nc.case_data(cid, dname)
        else:                                                                    # R = 256 is no GPU case: outside the contract (header)
            a = nc.make_case(cid, nc.DTYPES[dname], spec=nc._gn(1, shape[0], shape[1], 32, mean=16.0, std=16.0 / R, R=float(R)), seed=977)
            ref = nc.reference(a)
            fig = nc.figures(a, nc.model(a), ref)
        floor = nc.figures(a, {"out": ref["out"].to(nc.DTYPES[dname])}, ref)["out"][0]
        rows[R] = (fig["out"][0], floor, nc.onepass_rstd_error(a))
    return rows


@pytest.mark.parametrize("shape", [(1024, 320), (288, 2560)])
def test_one_pass_variance_by_mean_over_deviation(shape):
    """What the header states for the two-launch path.  Up to R = 64 the model's rel-L2 stays within 1.1 x the floor in both dtypes (fp16 1 x 1024 x 320:
    1.05 x, rstd error 9e-5; 1 x 288 x 2560: rstd error 4e-4 in bf16), so the R = 64 GPU cases take NO allowance; at R = 256 it is 4.8 x the floor in
    fp16 (1.0e-3) and 2.4 x in bf16 on the wide shape: outside the contract.  bf16 at 10 channels per group: 16 + N(0, s^2) rounds to multiples of
    2^-3, every sum is exact in fp32 and nothing shows at any R."""
    for dname in DNAMES:
        t = onepass_table(dname, shape)
        for R, (l2, floor, rstd) in t.items():
            print(f"one-pass {shape[0]}x{shape[1]} {dname} R={R}: model rel-L2 {l2:.3e} floor {floor:.3e} ratio {l2 / floor:.3f} rstd error {rstd:.2e}")
        for R in (4, 16, 64):
            assert t[R][0] <= 1.1 * t[R][1], (dname, R, t[R])
            a = nc.case_data(f"gn-offset {shape[0]}x{shape[1]}-R{R}", dname)[0]
            _, ref, mod, fig, bnd, _ = nc.case_data(f"gn-offset {shape[0]}x{shape[1]}-R{R}", dname)
            assert bnd["out"][0] == 1.5 * fig["out"][0], "no allowance: the model does not leave the floor"
        assert t[4][2] <= 1e-5 and t[16][2] <= 5e-5 and t[64][2] <= 1e-3
        if dname == "fp16" or shape[1] == 2560:
            assert t[256][0] > 2.0 * t[256][1], "R = 256 leaves the floor"
        else:
            assert max(v[2] for v in t.values()) <= 1e-6, "bf16 at 10 channels per group: every sum is exact in fp32"


# ---- injected faults ------------------------------------------------------------------------------------------------------------------------
# fault -> (a GPU case at which the faulted model must FAIL in bf16, a GPU case that enters the faulted code and passes by accident, or None)
FAULT_CASES = {
    "partial_drops_last_pixel": ("gn-two 1x300x320g32", None),
    "apply_skips_remainder": ("gn-two 1x675x1024g32", "gn-two 1x264x2056g8"),           # per 8 at ry 1: two full trips, no remainder
    "prefetch_on_second_slot": ("gn-two 1x264x2056g8", None),
    "fold_npart_minus_1": ("gn-two 1x264x320g40", "gn-two 3x1387x64g32"),               # the last slab is empty
    "from_partials_wrong_nblk": ("gn-partials n7-b2-apply", "gn-partials n9-apply"),    # one item: the item stride is never used
    "group_of_chunk_head": ("gn-two 1x300x320g32", "gn-two 1x264x320g40"),              # 8-channel groups lie on the chunks
    "x1_with_c0_pitch": ("gn-two 1x9x24+16g4", None),
    "count_c0": ("gn-two 1x9x24+16g4", "gn-two 1x300x320g32"),                          # one source: c0 is C
    "eps_outside_sqrt": ("gn-two 1x300x64g32-eps", "gn-two 1x300x320g32"),              # std 1: eps moves rstd by 5e-6 either way
    "beta_dropped_without_gamma": ("gn-two 1x264x8g1-nogamma", "gn-two 2x264x320g32-bare"),
    "small_ragged_lane_included": ("gn-small 3x250x64g8-nogamma", "gn-small 2x64x512g32"),          # 2 x 32 pixel lanes hold 64 pixels: none is ragged
    "ln_drops_ragged_chunk": ("ln 33x200-nogamma-nobeta-pitch", "ln 33x320"),           # 40 chunks on 8 lanes: no ragged trip
    "stats_wrong_sign": ("ln-stats 33x320", None),
}


def test_every_fault_of_the_issue_is_listed():
    assert set(FAULT_CASES) == set(nc.FAULTS) and len(nc.FAULTS) == 13


@pytest.mark.parametrize("fault", sorted(FAULT_CASES))
def test_injected_fault_fails(fault):
    hit, accident = FAULT_CASES[fault]
    fails, fig = verdict(hit, "bf16", fault)
    print(fault, hit, fig)
    assert fails, f"{fault} passed on {hit}: {fig}"
    assert not verdict(hit, "bf16")[0]
    if accident is not None:
        assert not verdict(accident, "bf16", fault)[0], f"{fault} on {accident}"


def test_more_faults_fail_where_only_one_case_sees_them():
    assert verdict("ln 33x72-nogamma", "bf16", "beta_dropped_without_gamma")[0]
    assert verdict("gn-small 1x64x40+24g4", "bf16", "x1_with_c0_pitch")[0]
    assert verdict("gn-two 1x257x8192g32", "bf16", "prefetch_on_second_slot")[0]
    assert verdict("gn-two 2x577x640g32-const", "bf16", "group_of_chunk_head")[0]
    assert verdict("gn-partials n9-coef", "bf16", "fold_npart_minus_1")[0]
    assert verdict("gn-two coef-2x264x24+16g4", "bf16", "count_c0")[0]
    assert verdict("gn-small 2x250x64g8-m16", "bf16", "small_ragged_lane_included")[0]
    # every multi-slab two-launch case whose last slab holds pixels sees a fold that stops one short
    for cid in nc.ALL:
        if cid.startswith("gn-two"):
            a = nc.case_data(cid, "bf16")[0]
            pl = nc.plan(a)
            if pl["path"] == "two-launch":
                assert bool(verdict(cid, "bf16", "fold_npart_minus_1")[0]) == ((pl["gn_nblk"] - 1) * pl["per"] < a["hw"]), cid


def test_a_fault_confined_to_one_block_shows_in_the_block_figure():
    """2 % of the peak added to one (item, slab, group) of 3 x 170 x 32, and to one (item, group) of 3 x 8 on the small path: the whole-tensor rel-L2
    passes, the block's does not"""
    for cid, target in (("gn-two 3x1387x64g32", (1, 17, 9)),):
        a, ref, mod, fig, bnd, _ = nc.case_data(cid, "bf16")
        ids, grid = nc.blocks(a)
        flat = 0
        for i, n in zip(target, grid):
            flat = flat * n + i
        out = {"out": mod["out"].clone()}
        out["out"][ids == flat] += 0.02 * float(ref["out"].abs().max())
        fails, f = nc.judge(a, out, ref, bnd, None, cid)
        assert fails and f["out"][4] == list(target) and f["out"][0] <= bnd["out"][0] and f["out"][1] > bnd["out"][1], (cid, f, bnd)
        if len(grid) == 3:
            assert f["out"][2] > bnd["out"][2]
