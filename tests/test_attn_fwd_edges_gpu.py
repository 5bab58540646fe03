"""GPU: hand-made edge descriptors of ``tg_attention`` / ``tg_attention_ps`` / ``tg_attn_probs`` (csrc/tg_attention.hip: one kernel template, 17
instances, and the probability export) against the fp64 restatement of their C-ABI contract (tests/attn_fwd_contract.py).

The descriptors are filled through ``theatergen_amd._lib`` directly, so head dims below the instance's padded one, mask strides, pitches and
pointers the ``ops`` wrappers never produce are reachable.  The cases are ``attn_fwd_contract.CASES``, the ones whose model conditions
tests/test_attn_fwd_contract_cpu.py asserts on the CPU.  Every case
  * compares the output with the restatement: whole-tensor rel-L2, the worst (batch item, head, 128-query block) and max|err| / max|ref|;
  * fills the output storage (pad columns, gap rows) with a sentinel byte first and checks that every byte outside the written region kept it;
  * replays once into a NaN-filled output: same bits, no NaN.
Every input element the contract does not read holds NaN: pad columns of pitched rows, gap rows, the left half of the fused buffer K is the
right half of, V^T columns from ``len`` on, the mask outside the rows (and row pitch) read, the floats around ``w1_dev``.

Bounds (the norm rule, nothing tuned on the kernel): 1.5x the whole-tensor rel-L2 and 1.5x the worst block of the schedule-faithful fp32
model, 2x its max-rel, all from the case's own operands; cases with N(0, 1)-scaled scores also meet 1.5x launch_check's l2_tol / rel_tol,
whole tensor and worst block.  ``tg_attn_probs`` (fp32) is held element by element to the operation-count bound of the contract module.
Measured figures: profiles/attn_fwd_contract_findings.md.
"""
import ctypes as C

import pytest
import torch

from tests import attn_fwd_contract as af
from tests import gemm_contract as gc
from tests import launch_check as lc
from tests import parity_metrics as pm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
SENTINEL = 0xA5
TG_ERR_ARG = -1


def _name(dtype):
    return str(dtype).replace("torch.", "")


def descriptor(a):
    from theatergen_amd import _lib, ops
    p = ops._ptr
    d = _lib.AttnDesc()
    d.dtype = ops._dt(a["q"])
    for f in ("batch", "heads", "head_dim", "n_q", "len0", "len1", "causal", "q_ld", "q_bs", "k0_ld", "k0_bs", "vt0_ld", "vt0_bs", "k1_ld", "k1_bs",
              "vt1_ld", "vt1_bs", "out_ld", "out_bs", "mask_bs", "mask_hs", "mask_qs", "scale", "w1"):
        setattr(d, f, a[f])
    for f in ("q", "k0", "vt0", "k1", "vt1", "out", "w1_dev", "mask"):
        setattr(d, f, p(a[f]))
    return d


def call(a, d):
    """tg_attention_ps where the descriptor dict carries a count, else tg_attention"""
    from theatergen_amd import _lib, ops
    L = _lib.lib()
    rc = (L.tg_attention(C.byref(d), ops._stream()) if a["ip_scale_count"] is None else
          L.tg_attention_ps(C.byref(d), int(a["ip_scale_count"]), ops._stream()))
    torch.cuda.synchronize()
    return rc


def launch(a):
    return call(a, descriptor(a))


def abs_tols(dtype):
    return 1.5 * lc.l2_tol(dtype), 1.5 * lc.rel_tol(dtype)


def run_case(a, what, kind="normal"):
    """the checks of this file on one descriptor -> (device metrics, model metrics, the output's values)"""
    reads, writes = af.read_extents(a), af.written_region(a)
    lc.LaunchChecker._check_reads(reads + writes, what)
    dtype = a["q"].dtype
    ref = af.reference(a)
    assert bool(torch.isfinite(ref).all()), f"{what}: the reference is not finite (the case is outside the contract)"
    mm = af.compare(af.model(a), ref, a["heads"])
    fl = af.compare(ref.to(dtype).to(torch.float64), ref, a["heads"])                 # the floor: fp64 rounded once
    bound = af.bounds(mm)
    masks = lc.LaunchChecker._write_masks(writes)
    lc.LaunchChecker._check_overlap(masks, reads, what)
    for t, _ in masks.values():
        lc._bytes(t).fill_(SENTINEL)
    snaps = lc.LaunchChecker._snapshot(masks)
    assert launch(a) == 0, what
    lc.LaunchChecker._check_outside(masks, snaps, what)
    first = writes[0].view().clone()
    m = af.compare(first, ref, a["heads"])
    ratio = max(m[k] / b if b > 0 else (0.0 if m[k] == 0 else float("inf")) for k, b in zip(("rel_l2", "block_rel_l2", "max_rel"), bound))
    pm.record(f"attn_fwd edge {what}", m, model=mm, floor=fl["rel_l2"], instance=list(af.instance(a)), bound_ratio=ratio)
    print(f"ATTN_FWD|{what}|{kind}|{af.instance(a)}|dev {m['rel_l2']:.3e} {m['block_rel_l2']:.3e} {m['max_rel']:.3e}|model {mm['rel_l2']:.3e} "
          f"{mm['block_rel_l2']:.3e} {mm['max_rel']:.3e}|floor {fl['rel_l2']:.3e}|dev/bound {ratio:.3f}")
    assert af.within(m, bound), f"{what}: device {m} outside the bound {bound} of the fp32 model {mm}"
    if kind == "normal":
        l2, mx = abs_tols(dtype)
        assert max(m["rel_l2"], m["block_rel_l2"]) <= l2 and m["max_rel"] <= mx, f"{what}: device {m} above the absolute figure ({l2:.1e}, {mx:.1e})"
    for t, _ in masks.values():
        gc._storage_tensor(t).fill_(float("nan"))
    assert launch(a) == 0, what
    again = writes[0].view()
    assert not bool(torch.isnan(again).any()), f"{what}: the replay keeps NaN (an element was not written, or stale memory was read)"
    assert torch.equal(again.contiguous().view(torch.int16), first.contiguous().view(torch.int16)), f"{what}: the replay's bits differ"
    return m, mm, first


def run_named(name, dtype):
    return run_case(af.build(name, dtype, DEV), f"{name} {_name(dtype)}", af.CASES[name]["kind"])


def _names(*prefixes):
    return [n for n in af.CASES if n.startswith(prefixes)]


# ---- every instance ------------------------------------------------------------------------------------------------------------------
def test_the_cases_reach_all_17_instances():
    got = {af.instance(dict(head_dim=c["kw"]["d"], mask=c["kw"].get("mask"))) for n, c in af.CASES.items() if n.startswith("inst ")}
    assert got == af.ALL_INSTANCES and len(got) == 17
    below = {c["kw"]["d"] for n, c in af.CASES.items() if n.startswith("inst ")} - {16, 32, 48, 64, 80, 96, 128, 160}
    assert below == {8, 24, 40, 56, 72, 88, 104, 136}            # head_dim < DPAD: the d < HD predicates of Q, K, V^T and the store


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("name", _names("inst "))
def test_every_instance(name, dtype):
    """n_q 136 (two query blocks, the second of 8 rows), len0 141 (two full tiles and a ragged one with the V^T fix-up), len1 4"""
    run_named(name, dtype)


# ---- key and query counts, causal, mask layouts and values ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("name", _names("len0 ", "len1 ", "nq "))
def test_key_and_query_counts(name, dtype):
    run_named(name, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("name", _names("causal "))
def test_causal(name, dtype):
    """n_q = len0 = 200: tiles 2 and 3 are hidden from every row of block 0; n_q 70 < len0 192: tiles 2 and 3 are hidden from every row;
    segment 1 is not causal; causal and mask both apply"""
    run_named(name, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("name", _names("mask layout "))
def test_mask_layouts(name, dtype):
    """the eight combinations of zero and non-zero mask_bs / mask_hs / mask_qs and a row pitch of len0 + 11; every (item, head, row) of the
    mask holds values of its own, the storage around and between the rows read holds NaN"""
    run_named(name, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("name", [n for n in _names("mask ") if not n.startswith("mask layout")])
def test_mask_values(name, dtype):
    """-10000; -1e30 on some keys; -1e30 on every key of a row (uniform); -inf on part of a tile; -inf on the whole first tile with visible
    keys after it; finfo.min at scale 0.125 (mask / scale overflows to -inf).  The all-zero mask: bit-equal to the unmasked launch where that
    is not the FOLD instance (head dim 64), judged at the bound at head dim 40."""
    m, mm, first = run_named(name, dtype)
    if name.startswith("mask zero"):
        kw = dict(af.CASES[name]["kw"], mask=None)
        b = af.make_case(dtype, device=DEV, **kw)
        assert launch(b) == 0
        same = torch.equal(af.written_region(b)[0].view().contiguous().view(torch.int16), first.contiguous().view(torch.int16))
        print(f"ATTN_FWD_ZEROMASK|{name} {_name(dtype)}|bit-equal to the unmasked launch: {same}")
        if not af.instance(b)[3]:
            assert same, f"{name}: the zero-mask launch differs from the unmasked one"
    if "big_row" in name:
        a = af.build(name, dtype, DEV)
        ref = af.reference(a).reshape(a["batch"], a["n_q"], a["heads"], -1)
        vmean = torch.stack([af.read_extents(a)[2].view()[b].double().reshape(a["heads"], -1, a["len0"]).mean(-1) for b in range(a["batch"])])
        assert float((ref[:, 0] - vmean).abs().max()) < 1e-12                  # row 0 of the reference IS the uniform average of V


# ---- softmax range -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("name", _names("range "))
def test_softmax_range(name, dtype):
    """per instance class (FOLD, ONES, plain, MASK): a key 7.5 exp2 units above the reference in the last tile (no rescale, P up to 181), one
    8.5 above (rescale), one 200 above (a skipped rescale overflows), a spike in tile 0 (everything after it underflows), operands x 8"""
    a = af.build(name, dtype, DEV)
    info = {}
    af.model(a, info=info)
    if "late +7.5" in name:
        assert info["rescales"] == 0 and 128 < info["p_max"] <= 256, info
    if "late +8.5" in name or "late +200" in name:
        assert info["rescales"] == 1, info
    if "tile0 +200" in name:
        assert info["rescales"] == 0, info
    run_case(a, f"{name} {_name(dtype)}", "peaked")


# ---- FOLD against the zero-mask instance on the same head-dim-40 operands ------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("d", [40, 64])
@pytest.mark.parametrize("qmul", af.FOLD_QMULS)
def test_fold_against_the_zero_mask_instance(qmul, d, dtype):
    """Q x 1, 2, 4, 8: the unmasked launch (FOLD at head dim 40) and the zero-mask launch (<48, 64, ONES, MASK>: no FOLD) of the same operands,
    each against fp64, the floor and its model; head dim 64 (no FOLD on either side) for scale"""
    res = {}
    for side in ("nomask", "zeromask"):
        name = f"qx{qmul:g} d{d} {side}"
        res[side] = run_named(name, dtype)
    (mf, mmf, of), (mz, mmz, oz) = res["nomask"], res["zeromask"]
    print(f"ATTN_FWD_FOLD|d{d} qx{qmul:g} {_name(dtype)}|unmasked dev {mf['rel_l2']:.3e} blk {mf['block_rel_l2']:.3e} model {mmf['rel_l2']:.3e}|"
          f"zero-mask dev {mz['rel_l2']:.3e} blk {mz['block_rel_l2']:.3e} model {mmz['rel_l2']:.3e}|bit-equal {torch.equal(of, oz)}")
    if d == 64:
        assert torch.equal(of.view(torch.int16), oz.view(torch.int16))


# ---- tg_attention_ps -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("name", _names("ps "))
def test_per_item_ip_scale(name, dtype):
    """counts 0, 1 and batch; with one float per item, item b is bit-equal to a scalar launch (tg_attention) with w1_dev[b]; the launch
    constant w1 = 9 must never be read"""
    m, mm, first = run_named(name, dtype)
    kw = af.CASES[name]["kw"]
    if kw["ip_scale_count"] == kw["B"]:
        B, nq = kw["B"], kw["n_q"]
        for b in range(B):
            s = af.make_case(dtype, device=DEV, **dict(kw, w1_dev=[kw["w1_dev"][b]], ip_scale_count=None))
            assert launch(s) == 0
            one = af.written_region(s)[0].view()[b]
            assert torch.equal(one.contiguous().view(torch.int16), first[b].contiguous().view(torch.int16)), f"{name}: item {b} differs"
        assert nq > 0


# ---- tg_attn_probs -------------------------------------------------------------------------------------------------------------------
def probs_launch(a, **edit):
    from theatergen_amd import _lib, ops
    p = ops._ptr
    v = dict(dtype=ops._dt(a["q"]), batch=a["batch"], b0=a["b0"], heads=a["heads"], head_dim=a["head_dim"], n_q=a["n_q"], q=p(a["q"]),
             q_ld=a["q_ld"], q_bs=a["q_bs"], k=p(a["k"]), k_ld=a["k_ld"], k_bs=a["k_bs"], len=a["len"], scale=a["scale"], tokens=p(a["tokens"]),
             n_tokens=a["n_tokens"], probs=p(a["probs"]))
    v.update(edit)
    rc = _lib.lib().tg_attn_probs(v["dtype"], v["batch"], v["b0"], v["heads"], v["head_dim"], v["n_q"], v["q"], v["q_ld"], v["q_bs"], v["k"],
                                  v["k_ld"], v["k_bs"], v["len"], v["scale"], v["tokens"], v["n_tokens"], v["probs"], ops._stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("d", [8, 40, 160])
@pytest.mark.parametrize("length", [1, 63, 64, 65, 255, 256])
def test_attn_probs(length, d, dtype):
    """n_q 1, 5, 8 (one partial, one full plus a partial, two full workgroups of 4 rows) x b0 0, 1 of batch 2 x all columns, one token, five
    tokens with a repeated index; pitched q / k with NaN pads and gap rows; element by element against the operation-count bound"""
    worst = 0.0
    for n_q in (1, 5, 8):
        for b0 in (0, 1):
            for tokens in (None, [length // 2], [0, length - 1, length // 2, length - 1, min(1, length - 1)]):
                a = af.probs_case(dtype, 2, b0, 2, d, n_q, length, tokens=tokens, device=DEV)
                what = f"probs len={length} d={d} nq={n_q} b0={b0} tokens={tokens} {_name(dtype)}"
                reads, writes = af.probs_read_extents(a), af.probs_written_region(a)
                lc.LaunchChecker._check_reads(reads + writes, what)
                ref, bound = af.probs_reference(a), af.probs_bound(a)
                model_err = (af.probs_model(a) - ref).abs()
                assert bool((model_err <= bound).all()), f"{what}: the fp32 model leaves the bound"
                masks = lc.LaunchChecker._write_masks(writes)
                for t, _ in masks.values():
                    lc._bytes(t).fill_(SENTINEL)
                snaps = lc.LaunchChecker._snapshot(masks)
                assert probs_launch(a) == 0, what
                lc.LaunchChecker._check_outside(masks, snaps, what)
                first = a["probs"].clone()
                err = (first.double() - ref).abs()
                r = float((err / bound).max())
                worst = max(worst, r)
                assert r <= 1.0, f"{what}: |err| / bound = {r:.3f} at {int(torch.argmax(err / bound))}"
                if tokens is None:
                    assert float((first.double().sum(-1) - 1.0).abs().max()) < 1e-5, what
                gc._storage_tensor(a["probs"]).fill_(float("nan"))
                assert probs_launch(a) == 0, what
                assert torch.equal(a["probs"].view(torch.int32), first.view(torch.int32)), f"{what}: the replay's bits differ"
    print(f"ATTN_FWD_PROBS|len={length} d={d} {_name(dtype)}|worst |err| / bound {worst:.3f}")


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def _refused(a, what, edit=None, count=None):
    """host validation returns TG_ERR_ARG with a message and no output byte changes (the checks run before any launch)"""
    from theatergen_amd import _lib
    masks = lc.LaunchChecker._write_masks(af.written_region(a))
    for t, _ in masks.values():
        lc._bytes(t).fill_(SENTINEL)
    d = descriptor(a)
    if edit is not None:
        edit(d)
    rc = call(a if count is None else dict(a, ip_scale_count=count), d)
    assert rc == TG_ERR_ARG, f"{what}: returned {rc}, documented {TG_ERR_ARG}"
    assert _lib.lib().tg_last_error(), f"{what}: no error message"
    for t, _ in masks.values():
        assert bool((lc._bytes(t) == SENTINEL).all()), f"{what}: a refused descriptor wrote to its outputs"


def _set(**kv):
    def edit(d):
        for k, v in kv.items():
            setattr(d, k, v)
    return edit


def _bump(field, nbytes):
    return lambda d: setattr(d, field, getattr(d, field) + nbytes)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_attention_refusals_return_tg_err_arg_and_write_nothing(dtype):
    def mk(**kw):
        return af.make_case(dtype, 2, 40, 77, 2, 64, **dict(dict(len1=4, device=DEV), **kw))
    for what, edit in (
            ("bad dtype", _set(dtype=7)), ("batch 0", _set(batch=0)), ("heads 0", _set(heads=0)), ("n_q 0", _set(n_q=0)), ("len0 0", _set(len0=0)),
            ("head_dim 0", _set(head_dim=0)), ("head_dim 12", _set(head_dim=12)), ("head_dim 168", _set(head_dim=168)),
            ("null q", _set(q=None)), ("null k0", _set(k0=None)), ("null vt0", _set(vt0=None)), ("null out", _set(out=None)),
            ("q_ld % 8", _set(q_ld=140)), ("k0_ld % 8", _set(k0_ld=268)), ("vt0_ld % 8", _set(vt0_ld=92)), ("out_ld % 4", _set(out_ld=134)),
            ("len1 -1", _set(len1=-1)), ("len1 65", _set(len1=65)), ("null k1", _set(k1=None)), ("null vt1", _set(vt1=None)),
            ("k1_ld % 8", _set(k1_ld=140)), ("vt1_ld % 8", _set(vt1_ld=12)),
            ("scale 0", _set(scale=0.0)), ("scale < 0", _set(scale=-0.125)), ("scale NaN", _set(scale=float("nan"))),
            ("q + 2 bytes", _bump("q", 2)), ("q + 8 bytes", _bump("q", 8)), ("k0 + 8 bytes", _bump("k0", 8)), ("vt0 + 2 bytes", _bump("vt0", 2)),
            ("out + 4 bytes", _bump("out", 4)), ("k1 + 8 bytes", _bump("k1", 8)), ("vt1 + 4 bytes", _bump("vt1", 4)),
            ("vt0_ld < len0", _set(vt0_ld=72)), ("vt1_ld < len1", _set(vt1_ld=0)),
            ("q_bs % 8", _bump("q_bs", 4)), ("k0_bs % 8", _bump("k0_bs", 4)), ("vt0_bs % 8", _bump("vt0_bs", 4)), ("out_bs % 4", _bump("out_bs", 2)),
            ("k1_bs % 8", _bump("k1_bs", 4)), ("vt1_bs % 8", _bump("vt1_bs", 4))):
        _refused(mk(), f"{what} {_name(dtype)}", edit)
    _refused(mk(mask="zero"), "mask + 2 bytes", _bump("mask", 2))
    _refused(mk(mask="zero"), "mask with scale 0", _set(scale=0.0))
    _refused(mk(w1_dev=[0.4, 0.5]), "ip_scale_count 3 of batch 2", count=3)
    _refused(mk(w1_dev=[0.4, 0.5]), "ip_scale_count -1", count=-1)
    _refused(mk(), "ip_scale_count = batch without w1_dev", count=2)
    from theatergen_amd import _lib, ops
    assert _lib.lib().tg_attention(None, ops._stream()) == TG_ERR_ARG and _lib.lib().tg_last_error()
    # with one batch item the batch strides move nothing and are not checked
    one = af.make_case(dtype, 1, 40, 77, 2, 64, len1=4, device=DEV)
    d = descriptor(one)
    d.q_bs, d.k0_bs, d.vt0_bs, d.out_bs = d.q_bs + 4, d.k0_bs + 4, d.vt0_bs + 4, d.out_bs + 2
    assert call(one, d) == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_attn_probs_refusals_return_tg_err_arg_and_write_nothing(dtype):
    from theatergen_amd import _lib
    for what, edit in (("bad dtype", dict(dtype=7)), ("null q", dict(q=None)), ("null k", dict(k=None)), ("null probs", dict(probs=None)),
                       ("batch <= b0", dict(b0=2)), ("b0 < 0", dict(b0=-1)), ("heads 0", dict(heads=0)), ("n_q 0", dict(n_q=0)),
                       ("len 0", dict(len=0)), ("len 257", dict(len=257)), ("head_dim 0", dict(head_dim=0)), ("head_dim 12", dict(head_dim=12)),
                       ("q_ld % 8", dict(q_ld=20)), ("k_ld % 8", dict(k_ld=28)), ("tokens with n_tokens 0", dict(n_tokens=0))):
        a = af.probs_case(dtype, 2, 0, 2, 8, 5, 63, tokens=[1, 2], device=DEV)
        lc._bytes(a["probs"]).fill_(SENTINEL)
        rc = probs_launch(a, **edit)
        assert rc == TG_ERR_ARG, f"probs {what}: returned {rc}"
        assert _lib.lib().tg_last_error(), f"probs {what}: no error message"
        assert bool((lc._bytes(a["probs"]) == SENTINEL).all()), f"probs {what}: a refused call wrote"
