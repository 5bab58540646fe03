"""CPU: pins tests/guidance_contract.py (the fp64 restatement the GPU edge tests of the guidance reductions compare against) and shows that
the comparison has teeth at the tolerances it derives.

  * on tie-free inputs the contract IS oracle/guidance_loss.compute_ca_lossv3 and its autograd in fp64 (all three kinds, a two-box object,
    several token positions);
  * a plain fp32 model of the kernel's algorithm (31-step radix select on the bit pattern, ties broken in index order, lane-serial sums
    and a 6-step butterfly, heads and items added serially) passes the contract on every GPU case at the derived tolerances: the
    reference alone fits them (the ratios are printed; profiles/guidance_contract_findings.md quotes them);
  * the same model breaking ties from the other end passes too (the contract describes a set), and with one output fault injected it fails.
"""
import numpy as np
import pytest
import torch

from tests import guidance_contract as gct

F = np.float32
CASES = sorted(gct.cases())


# ---- fp32 model of the kernel's algorithm, with fault switches ------------------------------------------------------------------------
def wave_sum32(v):
    """a wave's sum of v[0..n): lane l adds v[l], v[l + 64], ... serially, then a 6-step butterfly"""
    n = len(v)
    pad = np.zeros((n + 63) // 64 * 64, dtype=F)
    pad[:n] = v
    acc = np.zeros(64, dtype=F)
    for row in pad.reshape(-1, 64):
        acc = acc + row
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[lanes ^ o]
    return F(acc[0])


def _select32(x, k, fault):
    bits = x.view(np.uint32)
    cand = 0
    for bit in range(30, -1, -1):
        trial = cand | (1 << bit)
        if int((bits >= trial).sum()) >= k:
            cand = trial
    if fault == "thr_bit_up":
        cand += 1
    if fault == "thr_bit_down":
        cand -= 1
    thr = np.array([cand], dtype=np.uint32).view(F)[0]
    gt = x > thr
    return thr, gt, wave_sum32(np.where(gt, x, F(0)))


def _topk_head(a, m, t, gcol, fault):
    scale, fg_w, bg_w = F(t["scale"]), F(t["fg_w"]), F(t["bg_w"])
    sels, means = [], []
    for x, k, own in ((a * m, t["k_fg"], m == 1), (a * (F(1) - m), t["k_bg"], m == 0)):
        thr, gt, s = _select32(x, k, fault)
        need = k - int(gt.sum())
        means.append(s / F(k) if fault == "mean_drops_need" else (s + F(need) * thr) / F(k))
        eq = x == thr
        lim = need + (1 if fault == "tie_extra" else -1 if fault == "tie_fewer" else 0)
        if fault == "ties_from_the_end":
            rank = (np.cumsum(eq[::-1]) - eq[::-1])[::-1]
        else:
            rank = np.cumsum(eq) - eq                       # equal elements before this one, in index order
        sel = gt | (eq & (rank < lim))
        if fault == "tie_for_greater" and (gt & own).any() and (eq & own & ~sel).any():
            sel[np.argmax(gt & own)] = False
            sel[np.argmax(eq & own & ~sel)] = True
        sels.append(sel)
    g = (F(0) - np.where(sels[0], scale * fg_w * m / F(t["k_fg"]), F(0))) + np.where(sels[1], scale * bg_w * (F(1) - m) / F(t["k_bg"]), F(0))
    gcol[g != 0] += g[g != 0]
    return fg_w * (F(1) - means[0]) + bg_w * means[1]


def _ratio_head(a, m, t, heads, gcol):
    sm, sa = wave_sum32(a * m), wave_sum32(a)
    r = sm / sa
    c = F(t["scale"]) / F(heads) * F(-2) * (F(1) - r) / (sa * sa)
    gcol += c * (m * sa - sm)
    return (F(1) - r) * (F(1) - r)


def _ref_head(a, rc, m, t, heads, gcol):
    eps = F(t["eps"])
    ci, ri = F(1) / (wave_sum32(a * m) + eps), F(1) / (wave_sum32(rc * m) + eps)
    cm = a * m * ci
    d = cm - rc * m * ri
    sg = np.sign(d).astype(F)
    sc = wave_sum32(sg * cm)
    gcol += F(t["scale"]) / F(heads) * ci * m * (sg - sc)
    return wave_sum32(np.abs(d))


def model(case, fault=None):
    """-> (out after, [gradient buffers after]): the terms in order, into the pre-filled buffers"""
    out = F(gct.OUT_PREFILL)
    grads = [gct.grad_prefill(m.shape).numpy().copy() for m in case["maps"]]
    for t in case["terms"]:
        attn = case["maps"][t["map"]].numpy()
        heads, hw, n_tok = attn.shape
        tok = t["token"]
        a_all, m = attn[:, :, tok].astype(F), t["mask"].numpy().astype(F).reshape(-1)
        wtok = (tok + 1) % n_tok if fault == "neighbour_column" and n_tok > 1 else tok
        s = F(0)
        for h in range(heads):
            if fault == "head_skipped" and h == 1:
                continue
            gcol = grads[t["map"]][h, :, wtok].copy()
            if t["kind"] == "topk":
                hl = _topk_head(a_all[h], m, t, gcol, fault)
            elif t["kind"] == "ratio":
                hl = _ratio_head(a_all[h], m, t, heads, gcol)
            else:
                hl = _ref_head(a_all[h], t["ref"].numpy().astype(F).reshape(heads, hw)[h], m, t, heads, gcol)
            grads[t["map"]][h, :, wtok] = gcol
            s = s + hl
        divide = (t["kind"] != "topk") != (fault == "fold_divisor")
        out = out + (F(t["scale"]) * s / F(heads) if divide else F(t["scale"]) * s)
    return float(out), [torch.from_numpy(g) for g in grads]


def run_model(name, fault=None):
    case = gct.cases()[name]
    out, grads = model(case, fault)
    before = [gct.grad_prefill(m.shape) for m in case["maps"]]
    return gct.check_case(case, gct.case_refs(name), gct.OUT_PREFILL, out, before, grads)


# ---- the contract against the oracle ------------------------------------------------------------------------------------------------------
KEYS = ("mid", "up")
BOXES = [[(0.1, 0.15, 0.55, 0.6), (0.5, 0.4, 0.95, 0.9)], (0.3, 0.05, 0.8, 0.5)]          # object 0 has two boxes
POSITIONS = [[1, 2], [4]]


def _oracle_inputs():
    g = torch.Generator().manual_seed(11)
    maps = {}
    for k, (heads, H) in zip(KEYS, ((5, 8), (10, 12))):
        a = torch.rand(1, heads, H * H, 6, generator=g) + 0.05
        maps[k] = a / a.sum(-1, keepdim=True)
    refs = []
    for boxes in (BOXES[0], [BOXES[1]]):
        per_box = []
        for _ in boxes:
            per_box.append([{k: (torch.rand(1, v.shape[1], v.shape[2], 1, generator=g) + 0.05) / 6 for k, v in maps.items()}])
        refs.append(per_box if len(boxes) > 1 else per_box[0])
    return maps, refs


def _contract_terms(maps, refs, kw, with_ref):
    """the terms of one compute_ca_lossv3 call, built the way the header and the reference describe them"""
    from oracle import guidance_loss as og
    norm = 1.0 / (len(BOXES) * len(KEYS))
    terms = []
    for m, key in enumerate(KEYS):
        H = int(maps[key].shape[2] ** 0.5)
        for obj, pos in zip(BOXES, POSITIONS):
            mask = og._box_mask(obj, H, H).reshape(-1)
            for p in pos:
                if kw["use_ratio_based_loss"]:
                    terms.append(gct._term("ratio", m, p, mask, norm / len(pos)))
                else:
                    k_fg, k_bg = gct._k(mask, kw["fg_top_p"])
                    terms.append(gct._term("topk", m, p, mask, norm / len(pos), k_fg=k_fg, k_bg=k_bg, fg_w=kw["fg_weight"], bg_w=kw["bg_weight"]))
    if with_ref:
        for obj, pos, rf in zip(BOXES, POSITIONS, refs):
            boxes, rfs = (obj, rf) if isinstance(obj, list) else ([obj], [rf])
            for bx, r in zip(boxes, rfs):
                for m, key in enumerate(KEYS):
                    H = int(maps[key].shape[2] ** 0.5)
                    for p in pos:
                        terms.append(gct._term("ref", m, p, og._box_mask(bx, H, H).reshape(-1), norm * 2.0 / (len(boxes) * len(pos)),
                                               ref=r[0][key][0, :, :, 0].contiguous(), eps=1e-5))
    return terms


@pytest.mark.parametrize("form", ["topk", "ratio", "topk+ref"])
def test_contract_is_the_oracle_and_its_autograd(form):
    from oracle import guidance_loss as og
    maps, refs = _oracle_inputs()
    kw = dict(use_ratio_based_loss=True) if form == "ratio" else dict(use_ratio_based_loss=False, fg_top_p=0.2, bg_top_p=0.2, fg_weight=1.0,
                                                                      bg_weight=4.0)
    with_ref = form.endswith("ref")
    saved = {k: v.double().requires_grad_(True) for k, v in maps.items()}
    refs64 = [[[{k: v.double() for k, v in r[0].items()}] for r in o] if isinstance(o[0], list) else [{k: v.double() for k, v in o[0].items()}]
              for o in refs]
    extra = dict(ref_ca_saved_attns=refs64, index=0, ref_ca_loss_weight=2.0, ref_ca_last_token_only=False) if with_ref else {}
    want = og.compute_ca_lossv3(saved, BOXES, POSITIONS, list(KEYS), **extra, **kw)
    want_grads = torch.autograd.grad(want, [saved[k] for k in KEYS])
    terms = _contract_terms(maps, refs, kw, with_ref)
    got, grads = 0.0, [np.zeros(maps[k].shape[1:]) for k in KEYS]
    for t in terms:
        r = gct.reference(t, maps[KEYS[t["map"]]][0])
        assert r["grad"] is not None and len(r["head_terms"]) == maps[KEYS[t["map"]]].shape[1]
        got += r["term"]
        grads[t["map"]][:, :, t["token"]] += r["grad"]
    # scales are fp32 in the contract (the header's `float`), fp64 in the oracle: 2^-24 relative per term
    assert abs(got - want.item()) <= 2.0 ** -23 * abs(want.item()), (got, want.item())
    for g, w in zip(grads, want_grads):
        w = w[0].numpy()
        assert np.abs(g - w).max() <= 2.0 ** -23 * np.abs(w).max()
        assert np.array_equal(g != 0, w != 0)


# ---- the fp32 model fits the derived tolerances on every GPU case ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_fp32_model_passes_the_contract(name):
    m = run_model(name)
    print(f"fp32 model {name}: loss error / bound {m['loss_ratio']:.3f}, gradient error / bound {m['grad_ratio']:.3f}")
    assert m["loss_ratio"] <= 1.0 and m["grad_ratio"] <= 1.0


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_straddling_ties_preconditions(seed):
    gct.straddle_preconditions(gct.case_refs(f"straddling_ties_s{seed}")[0])


def test_ties_under_a_strictly_greater_set():
    r = gct.case_refs("ties_under_greater_s3")[0]
    gct.straddle_preconditions(r)
    assert all(s["greater"].sum() >= 2 for s in r["fg"] + r["bg"])


def test_zero_ties_and_clamped_k_are_what_the_cases_claim():
    r = gct.case_refs("ties_at_zero")[0]
    assert all(s["thr"] == 0 and s["need"] >= 2 and s["shown"].sum() > s["need"] and s["free"].any() for s in r["fg"] + r["bg"])
    e, w = gct.case_refs("empty_box")[0], gct.case_refs("whole_image_box")[0]
    assert all(s["thr"] == 0 and not s["greater"].any() and s["free"].all() for s in e["fg"] + w["bg"])
    v = gct.case_refs("values_around_2")[0]
    assert all(s["thr"] > 2 for s in v["fg"] + v["bg"]) and gct.column(gct.cases()["values_around_2"]["maps"][0], 2).min() < 1
    d = gct.case_refs("denormals")[0]
    assert all(0 < s["thr"] < np.finfo(np.float32).tiny and s["greater"].sum() == 3 for s in d["fg"])


def test_any_tie_break_is_admissible():
    for name in ("straddling_ties_s0", "ties_at_zero", "empty_box"):
        run_model(name, "ties_from_the_end")


FAULTS = [("tie_extra", "straddling_ties_s0"), ("tie_fewer", "straddling_ties_s0"), ("tie_for_greater", "ties_under_greater_s3"), ("tie_extra", "ties_under_greater_s3"),
          ("thr_bit_up", "straddling_ties_s0"), ("thr_bit_down", "straddling_ties_s2"), ("mean_drops_need", "straddling_ties_s0"),
          ("head_skipped", "straddling_ties_s0"), ("head_skipped", "heads_3"), ("fold_divisor", "straddling_ties_s0"),
          ("fold_divisor", "heads_5"), ("neighbour_column", "straddling_ties_s0"), ("neighbour_column", "hw_63"),
          ("tie_fewer", "denormals"), ("mean_drops_need", "k_is_1")]


@pytest.mark.parametrize("fault,name", FAULTS)
def test_injected_fault_is_rejected(fault, name):
    run_model(name)
    with pytest.raises(AssertionError):
        run_model(name, fault)
