"""GPU: the guidance reductions (csrc/tg_guidance.hip) at their edges, against the fp64 restatement of their C-ABI contract
(tests/guidance_contract.py), in every launch form: one launch per term (``ops.guidance_*``), the plan form (``ops.GuidanceBatch`` ->
``tg_guidance_plan_run`` + fold, with ``flush()``'s collision rule), the pointer-table form (``tg_guidance_batch``, filled through ctypes)
and, for the two boxes whose k the host clamps, the host path (``guidance.add_ca_loss_per_attn_map_to_loss``).

Every case
  * uses the tolerance the contract derives from operation counts (never tuned here; the measured error / bound ratios are recorded in
    parity_metrics.jsonl and quoted in profiles/guidance_contract_findings.md);
  * pre-fills ``out[0]`` (0.75) and every gradient buffer with a non-trivial pattern: the results are ``+=``;
  * requires the gradient columns of every other token to keep their bits;
  * holds NaN in the attention columns of every other token and requires a NaN-free result: they were not read.
The cases and their fp64 references are built once in tests/guidance_contract.py; the fp32 model of tests/test_guidance_contract_cpu.py
passes every one of them at the same tolerances, and each fault injected there fails.  No case provokes a fault: the two out-of-range
requests (hw = 72 x 72 for the LDS-resident select) are refused by host checks before anything is launched.
"""
import ctypes as C

import pytest
import torch

from tests import guidance_contract as gct
from tests import parity_metrics as pm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TG_ERR_ARG = -1
KIND_ID = {"topk": 0, "ratio": 1, "ref": 2}
ALL = sorted(gct.cases())
ONE_LAUNCH = [n for n in ALL if not gct.cases()[n].get("collides")]           # items of one launch never share a (grad, token) column
HOST = [n for n in ALL if "host" in gct.cases()[n]]


class Buffers:
    """a case on the device: maps, masks, reference columns, and freshly pre-filled out / gradient buffers"""

    def __init__(self, case):
        self.case = case
        self.maps = [m.to(DEV) for m in case["maps"]]
        on_dev = {}                                # terms that share a mask tensor share it on the device too (one pointer slot)
        self.masks = [on_dev.setdefault(id(t["mask"]), t["mask"].to(DEV)) for t in case["terms"]]
        self.refs = [t["ref"].to(DEV) if t["kind"] == "ref" else None for t in case["terms"]]
        self.refill()

    def refill(self):
        self.grads_before = [gct.grad_prefill(m.shape) for m in self.case["maps"]]
        self.grads = [g.to(DEV) for g in self.grads_before]
        self.out = torch.full((1,), gct.OUT_PREFILL, dtype=torch.float32, device=DEV)

    def result(self):
        torch.cuda.synchronize()
        return float(self.out.cpu()[0]), [g.cpu() for g in self.grads]


def launch_terms(b):
    from theatergen_amd import ops
    for t, mask, ref in zip(b.case["terms"], b.masks, b.refs):
        a, g = b.maps[t["map"]], b.grads[t["map"]]
        if t["kind"] == "topk":
            ops.guidance_topk(a, t["token"], mask, t["k_fg"], t["k_bg"], t["fg_w"], t["bg_w"], t["scale"], b.out, g)
        elif t["kind"] == "ratio":
            ops.guidance_ratio(a, t["token"], mask, t["scale"], b.out, g)
        else:
            ops.guidance_ref(a, t["token"], ref, mask, t["eps"], t["scale"], b.out, g)


def launch_plan(b):
    from theatergen_amd import ops
    batch = ops.GuidanceBatch(torch.device(DEV))
    for t, mask, ref in zip(b.case["terms"], b.masks, b.refs):
        batch.add(KIND_ID[t["kind"]], b.maps[t["map"]], t["token"], mask, t["scale"], b.grads[t["map"]], ref=ref, k_fg=t.get("k_fg", 0),
                  k_bg=t.get("k_bg", 0), fg_w=t.get("fg_w", 0.0), bg_w=t.get("bg_w", 0.0), eps=t.get("eps", 0.0))
    batch.flush(b.out)


def item_table(b):
    """the ``tg_guidance_item`` table of a case on the device -> (table, n_items, max_hw_topk, max_heads)"""
    from theatergen_amd import _lib
    terms = b.case["terms"]
    arr = (_lib.GuidanceItem * len(terms))()
    for it, t, mask, ref in zip(arr, terms, b.masks, b.refs):
        a = b.maps[t["map"]]
        it.attn, it.grad, it.mask, it.ref = a.data_ptr(), b.grads[t["map"]].data_ptr(), mask.data_ptr(), ref.data_ptr() if ref is not None else None
        it.heads, it.hw, it.n_tok, it.token = a.shape[0], a.shape[1], a.shape[2], t["token"]
        it.kind, it.k_fg, it.k_bg = KIND_ID[t["kind"]], t.get("k_fg", 0), t.get("k_bg", 0)
        it.fg_w, it.bg_w, it.scale, it.eps = t.get("fg_w", 0.0), t.get("bg_w", 0.0), t["scale"], t.get("eps", 0.0)
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
    max_hw = max([b.maps[t["map"]].shape[1] for t in terms if t["kind"] == "topk"] + [0])
    return table, len(terms), max_hw, max(b.maps[t["map"]].shape[0] for t in terms)


def launch_batch(b):
    from theatergen_amd import _lib, ops
    table, n, max_hw, max_heads = item_table(b)
    partials = torch.full((n,), float("nan"), dtype=torch.float32, device=DEV)
    _lib.check(_lib.lib().tg_guidance_batch(table.data_ptr(), n, max_hw, max_heads, partials.data_ptr(), b.out.data_ptr(), ops._stream()))
    torch.cuda.synchronize()                   # `table` and `partials` stay alive until the launch has finished


def launch_host(b, batched):
    """the host path of a one-box, one-token top-k term: the host builds the mask and clamps k"""
    from theatergen_amd import guidance as G
    from theatergen_amd import ops
    (t,), h = b.case["terms"], b.case["host"]
    a = b.maps[0]
    H = int(a.shape[1] ** 0.5)
    assert torch.equal(G._box_mask(h["box"], H, H, a.device)[0].reshape(-1), t["mask"]), "the host's box mask is not the case's"
    batch = ops.GuidanceBatch(a.device) if batched else None
    G.add_ca_loss_per_attn_map_to_loss(b.out, a, 1, [h["box"]], [[t["token"]]], use_ratio_based_loss=False, fg_top_p=h["top_p"],
                                       bg_top_p=h["top_p"], fg_weight=h["fg_w"], bg_weight=h["bg_w"], grad=b.grads[0], scale=t["scale"], batch=batch)
    if batched:
        assert [(i["k_fg"], i["k_bg"]) for i in batch.items] == [(t["k_fg"], t["k_bg"])], "the host's k is not the reference's"
        batch.flush(b.out)


FORMS = {"term": launch_terms, "plan": launch_plan, "batch": launch_batch, "host": lambda b: launch_host(b, False),
         "host_plan": lambda b: launch_host(b, True)}


def run_and_check(name, form):
    case = gct.cases()[name]
    b = Buffers(case)
    FORMS[form](b)
    out, grads = b.result()
    m = gct.check_case(case, gct.case_refs(name), gct.OUT_PREFILL, out, b.grads_before, grads)
    pm.record(f"guidance_edges/{name}/{form}", m)
    print(f"guidance {name} [{form}]: loss error / bound {m['loss_ratio']:.3f}, gradient error / bound {m['grad_ratio']:.3f}")
    return out, grads


def same_bits(x, y):
    return x[0] == y[0] and all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(x[1], y[1]))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_straddling_ties_inputs_straddle(seed):
    gct.straddle_preconditions(gct.case_refs(f"straddling_ties_s{seed}")[0])


@pytest.mark.parametrize("name", ALL)
def test_per_term_launches(name):
    run_and_check(name, "term")


@pytest.mark.parametrize("name", ALL)
def test_plan_form_and_flush(name):
    run_and_check(name, "plan")


@pytest.mark.parametrize("name", ONE_LAUNCH)
def test_pointer_table_form(name):
    run_and_check(name, "batch")


@pytest.mark.parametrize("name", HOST)
@pytest.mark.parametrize("form", ["host", "host_plan"])
def test_host_path_clamps_k(name, form):
    t = gct.cases()[name]["terms"][0]
    assert 1 in (t["k_fg"], t["k_bg"]) and t["mask"].sum() in (0, t["mask"].numel())
    run_and_check(name, form)


@pytest.mark.parametrize("name", ONE_LAUNCH)
def test_launch_forms_give_the_same_bits(name):
    """'the same sequence of additions the per-item launches perform (bit-identical loss)': plan form and pointer-table form against the
    same terms issued one launch each, in the same order — out[0] and every gradient element"""
    res = {}
    for form in ("term", "plan", "batch"):
        b = Buffers(gct.cases()[name])
        FORMS[form](b)
        res[form] = b.result()
    assert same_bits(res["plan"], res["term"]), (name, res["plan"][0], res["term"][0])
    assert same_bits(res["batch"], res["term"]), (name, res["batch"][0], res["term"][0])


@pytest.mark.parametrize("form", ["term", "plan", "batch"])
def test_loss_without_a_gradient_buffer_is_the_same_bits(form):
    """grad = NULL (``compute_ca_lossv3(return_grads=False)``): the same out[0], and nothing else to write to"""
    with_grad = Buffers(gct.cases()["plan_mixed"])
    FORMS[form](with_grad)
    b = Buffers(gct.cases()["plan_mixed"])
    b.grads = [None] * len(b.grads)
    if form == "term":
        launch_terms(b)
    elif form == "plan":
        launch_plan(b)
    else:
        b.grads = [torch.empty(0, device=DEV)] * len(b.grads)          # data_ptr() == 0: the table's NULL
        launch_batch(b)
    torch.cuda.synchronize()
    assert float(b.out.cpu()[0]) == with_grad.result()[0]


def test_flush_defers_colliding_terms(monkeypatch):
    """three terms on one (gradient, token) column: three launches, in item order within each"""
    from theatergen_amd import ops
    seen = []
    real = ops.GuidanceBatch._launch
    monkeypatch.setattr(ops.GuidanceBatch, "_launch", lambda self, now, loss: (seen.append([i["kind"] for i in now]), real(self, now, loss))[1])
    run_and_check("flush_collision", "plan")
    assert seen == [[0, 1], [0], [2]], seen


def test_fold_takes_more_than_256_items_in_one_launch(monkeypatch):
    from theatergen_amd import ops
    seen = []
    real = ops.GuidanceBatch._launch
    monkeypatch.setattr(ops.GuidanceBatch, "_launch", lambda self, now, loss: (seen.append(len(now)), real(self, now, loss))[1])
    run_and_check("items_over_256", "plan")
    assert seen == [300], seen


@pytest.mark.parametrize("name,form", [("straddling_ties_s0", "term"), ("ties_at_zero", "plan"), ("plan_mixed", "plan"), ("plan_mixed", "batch"),
                                       ("flush_collision", "plan")])
def test_replay_gives_the_same_bits(name, form):
    b = Buffers(gct.cases()[name])
    FORMS[form](b)
    first = b.result()
    b.refill()
    FORMS[form](b)
    assert same_bits(b.result(), first)


def test_map_too_large_for_the_select_is_refused_by_all_three_entries():
    """hw = 72 x 72: 4 waves x 2 x 5184 floats = 165888 bytes > 160 KB.  TG_ERR_ARG from the host checks, nothing launched, out and grad
    untouched"""
    from theatergen_amd import _lib, ops
    L = _lib.lib()
    heads, hw = 4, 72 * 72
    g = torch.Generator().manual_seed(72)
    case = dict(name="lds_refused", maps=[gct.nan_map({"n_tok": 2, 1: gct._prob_cols(heads, hw, g)})],
                terms=[gct._term("topk", 0, 1, gct.box_mask(72, 72, 10, 40, 10, 40), 0.25, k_fg=10, k_bg=10, fg_w=1.0, bg_w=4.0)])
    b = Buffers(case)
    t = case["terms"][0]
    rcs = {"topk": L.tg_guidance_topk(b.maps[0].data_ptr(), heads, hw, 2, 1, b.masks[0].data_ptr(), 10, 10, 1.0, 4.0, 0.25, b.out.data_ptr(),
                                      b.grads[0].data_ptr(), ops._stream())}
    assert b"too large" in L.tg_last_error()
    table, n, max_hw, max_heads = item_table(b)
    partials = torch.zeros(n, dtype=torch.float32, device=DEV)
    rcs["batch"] = L.tg_guidance_batch(table.data_ptr(), n, max_hw, max_heads, partials.data_ptr(), b.out.data_ptr(), ops._stream())
    arr = (_lib.GuidancePItem * 1)()
    p = arr[0]
    p.attn_slot, p.grad_slot, p.mask_slot, p.ref_slot, p.heads, p.hw, p.n_tok, p.token = 0, 1, 2, -1, heads, hw, 2, 1
    p.kind, p.k_fg, p.k_bg, p.fg_w, p.bg_w, p.scale = 0, 10, 10, 1.0, 4.0, t["scale"]
    ptable = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
    slots = (C.c_void_p * 3)(b.maps[0].data_ptr(), b.grads[0].data_ptr(), b.masks[0].data_ptr())
    head_terms = torch.zeros(heads, dtype=torch.float32, device=DEV)
    rcs["plan"] = L.tg_guidance_plan_run(ptable.data_ptr(), 1, hw, heads, slots, 3, head_terms.data_ptr(), b.out.data_ptr(), ops._stream())
    assert b"too large" in L.tg_last_error()
    assert rcs == {"topk": TG_ERR_ARG, "batch": TG_ERR_ARG, "plan": TG_ERR_ARG}, rcs
    out, grads = b.result()
    assert out == gct.OUT_PREFILL and torch.equal(grads[0], b.grads_before[0])
    with pytest.raises(RuntimeError, match="too large"):
        launch_plan(b)
