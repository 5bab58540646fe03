"""The C-ABI contract of ``tg_guidance_topk`` / ``tg_guidance_ratio`` / ``tg_guidance_ref`` (include/theatergen_hip.h) restated in fp64, for
checking single launches of the box-guidance reductions in any of their launch forms (per-term, ``tg_guidance_batch``,
``tg_guidance_plan_run`` + fold).  Written from the header and the reference formulas (oracle/guidance_loss.py), not from the kernel.

A TERM is a dict: ``kind`` ("topk" | "ratio" | "ref"), ``map`` (index of its attention map in the case; every map has one gradient buffer of
its shape), ``token``, ``mask`` fp32 [hw] (binary), ``scale`` and, by kind, ``k_fg k_bg fg_w bg_w`` / ``ref`` fp32 [heads, hw], ``eps``.
The float parameters are the header's ``float``: the contract is stated on their fp32 values.  With A = attn[:, :, token] (fp64 of the fp32 bits):

    topk   head_h = fg_w (1 - mean top_{k_fg}(A_h M)) + bg_w mean top_{k_bg}(A_h (1 - M))          term = scale sum_h head_h
    ratio  head_h = (1 - r_h)^2,  r_h = sum(A_h M) / sum(A_h)                                      term = scale mean_h head_h
    ref    head_h = sum_i |cm_i - rm_i|,  cm = A_h M / (sum(A_h M) + eps), rm likewise from ref    term = scale mean_h head_h
    out[0] += term;   grad[:, :, token] += d term / d A;   nothing else of grad is written, nothing else of attn is read.

``reference(term, attn)`` returns the term, the per-head terms, the dense fp64 gradient (ratio, ref) and the error bounds below.

TOP-K GRADIENT.  With ties the sub-gradient is a set.  Per head and per side (fg on x = A M, bg on x = A (1 - M)) the contract gives
``thr`` (the k-th largest of x), ``greater`` = {x > thr} (must be selected), ``less`` = {x < thr} (must not), ``tie`` = {x == thr} and
``need`` = k - |greater|; a selected element i receives ``value_i`` = -scale fg_w M_i / k_fg (fg) or +scale bg_w (1 - M_i) / k_bg (bg).
Masks are binary, so the fg contribution lands on M = 1 and the bg contribution on M = 0: each pixel is owned by one side.  A tied pixel whose
``value`` is 0 (it is owned by the other side) is FREE: selecting it changes nothing, so of the ``need`` selections between
max(0, need - |free|) and min(need, |tie \\ free|) fall on the tied pixels that show.  ``check_topk_column`` accepts a produced column exactly
when greater pixels moved by ``value``, less pixels kept their bits, every visible tie did one or the other, and their count is in that range.

TOLERANCES, from operation counts (u = 2^-24; nothing here was tuned on the kernel).  S = ceil(hw / 64), H = heads.
  * A head term is built from sums of at most hw non-negative fp32 products (A M is exact for a binary M): a lane adds its S elements
    serially, a 6-step wave reduction follows: relative error (S + 6) u of each sum, first order.  At most ten scalar roundings follow
    (the ref form's two extra roundings per element, the divide, 1 - x, the weights): CONST = 16 covers both.  The error of a head
    term is therefore <= (S + CONST) u mag_h, where mag_h is the head term with every subtraction replaced by an addition:
        topk   |fg_w| (1 + mean_f) + |bg_w| mean_b
        ratio  4 r (1 - r) + (1 - r)^2          (d (1 - r)^2 = 2 (1 - r) dr and dr <= 2 (S + 7) u r: numerator and denominator)
        ref    2 sum_i (cm_i + rm_i)            (each |d_i| is off by (S + 10) u (cm_i + rm_i); the sum adds (S + 6) u sum |d_i|)
  * Heads are added serially (H - 1 additions, each u of a partial sum <= sum_h mag_h), the scale and the 1 / H follow:
        |term error| <= SAFE (S + H + CONST) u |scale| [/ H] sum_h mag_h           SAFE = 2 for the second-order terms and the choice of
    fused or separate multiply-adds.  Terms, then the pre-filled out[0] = p, are added serially: n additions of at most u (|p| + sum_j |term_j|):
        |out error| <= sum_j bound_j + SAFE n u (|p| + sum_j |term_j|).
  * Ratio gradient g_i = c (M_i sa - sm), c = -2 scale (1 - r) / (H sa^2).  sa, sm carry (S + 6) u each, so M_i sa - sm (it cancels)
    is off by (2 S + 14) u sa, and 1 - r by (2 S + 14) u r.  With K = 2 |scale| / H = |c| sa^2 / (1 - r):
        |g_i error| <= K / sa^2 [ (2S+14) u r |M_i sa - sm| + (1 - r) (2S+14) u sa ] + 8 u |g_i| <= (2 S + 22) u K / sa
    an ABSOLUTE bound per head, = (2 S + 22) u |c| sa / (1 - r): it scales with |c| sa.  x SAFE.
  * Ref gradient g_i = c M_i (sign(d_i) - sc), c = scale ci / H, sc = sum_j sign(d_j) cm_j (|sc| <= 1).  cm_j carries (S + 10) u, the sum
    (S + 6) u more: sc is off by (2 S + 16) u; c by (S + 10) u; |sign - sc| <= 2:
        |g_i error| <= (4 S + 41) u |c|   on M_i = 1 (x SAFE), exactly 0 on M_i = 0.
    sign(d) must be the same in fp32 and fp64: the INPUTS must keep |d_i| >= MARGIN (cm_i + rm_i) with MARGIN = 4 (S + CONST) u (four times
    the fp32 error of d_i) wherever M_i = 1, unless cm_i = rm_i = 0 exactly.  ``reference`` asserts it: a precondition on the test's
    inputs, not on the kernel.  The one exception is a term marked ``exact_zero`` (ref equal to the column, or an empty mask): there d = 0
    identically, every product is the same on both sides in any precision, and term and gradient must be exactly 0 (bounds 0).
  * A top-k gradient element is one or two multiplies and one divide: 4 u |value|.  Every ``+=`` into a pre-filled element p adds one
    rounding: SAFE u (|p| + |g|), for all three kinds.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
SAFE = 2.0
CONST = 16
TOPK_GRAD_ULPS = 4.0
KINDS = ("topk", "ratio", "ref")          # the header's kind 0, 1, 2


def _f32(x):
    return float(np.float32(x))


def _np64(t):
    return t.detach().cpu().numpy().astype(np.float64) if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)


def steps(hw):
    return (hw + 63) // 64


def column(attn, token):
    return _np64(attn[:, :, token])


# ---- the three forms -----------------------------------------------------------------------------------------------------------------
def _side(x, k, value):
    """one head, one side: x fp64 [hw] >= 0; value fp64 [hw]: what a selected element receives"""
    thr = np.partition(x, len(x) - k)[len(x) - k]
    greater, less, tie = x > thr, x < thr, x == thr
    need = int(k - greater.sum())
    assert 1 <= need <= int(tie.sum())
    free = tie & (value == 0)
    shown = tie & ~free
    lo, hi = max(0, need - int(free.sum())), min(need, int(shown.sum()))
    return dict(thr=float(thr), greater=greater, less=less, tie=tie, free=free, shown=shown, need=need, lo=lo, hi=hi, value=value,
                mean=float((x[greater].sum() + need * thr) / k))


def _topk(t, A):
    H, hw = A.shape
    M = _np64(t["mask"]).reshape(-1)
    assert M.shape == (hw,) and np.all((M == 0) | (M == 1)), "the contract is stated for binary masks"
    k_fg, k_bg, fg_w, bg_w, scale = int(t["k_fg"]), int(t["k_bg"]), _f32(t["fg_w"]), _f32(t["bg_w"]), _f32(t["scale"])
    assert 1 <= k_fg <= hw and 1 <= k_bg <= hw
    vf, vb = -scale * fg_w * M / k_fg, scale * bg_w * (1 - M) / k_bg
    fg = [_side(A[h] * M, k_fg, vf) for h in range(H)]
    bg = [_side(A[h] * (1 - M), k_bg, vb) for h in range(H)]
    heads = np.array([fg_w * (1 - f["mean"]) + bg_w * b["mean"] for f, b in zip(fg, bg)])
    mag = np.array([abs(fg_w) * (1 + f["mean"]) + abs(bg_w) * b["mean"] for f, b in zip(fg, bg)])
    grad = np.zeros_like(A)                      # dense only when no head leaves a choice
    for h in range(H):
        for s in (fg[h], bg[h]):
            if s["lo"] != s["hi"] or s["lo"] not in (0, int(s["shown"].sum())):
                grad = None
                break
            sel = s["greater"] | (s["shown"] if s["lo"] > 0 else np.zeros(hw, dtype=bool))
            grad[h] += np.where(sel, s["value"], 0.0)
        if grad is None:
            break
    gb = TOPK_GRAD_ULPS * U * (np.abs(vf) + np.abs(vb))[None, :].repeat(H, 0)
    return dict(term=scale * heads.sum(), head_terms=heads, bound=SAFE * (steps(hw) + H + CONST) * U * abs(scale) * mag.sum(),
                grad=grad, grad_bound=gb, fg=fg, bg=bg, mask=M)


def _ratio(t, A):
    H, hw = A.shape
    M = _np64(t["mask"]).reshape(-1)
    scale = _f32(t["scale"])
    sa, sm = A.sum(1), (A * M).sum(1)
    r = sm / sa
    heads = (1 - r) ** 2
    mag = 4 * r * (1 - r) + (1 - r) ** 2
    c = scale / H * (-2.0) * (1 - r) / (sa * sa)
    grad = c[:, None] * (M[None, :] * sa[:, None] - sm[:, None])
    gb = SAFE * (2 * steps(hw) + 22) * U * (2 * abs(scale) / H) / sa
    return dict(term=scale * heads.sum() / H, head_terms=heads, bound=SAFE * (steps(hw) + H + CONST) * U * abs(scale) / H * mag.sum(),
                grad=grad, grad_bound=gb[:, None].repeat(hw, 1))


def sign_margin(hw):
    return 4 * (steps(hw) + CONST) * U


def _ref(t, A):
    H, hw = A.shape
    M = _np64(t["mask"]).reshape(-1)
    R = _np64(t["ref"]).reshape(H, hw)
    scale, eps = _f32(t["scale"]), _f32(t["eps"])
    ci, ri = 1.0 / ((A * M).sum(1) + eps), 1.0 / ((R * M).sum(1) + eps)
    cm, rm = A * M * ci[:, None], R * M * ri[:, None]
    d = cm - rm
    if t.get("exact_zero"):
        assert not d.any(), "exact_zero: ref must equal the column wherever the mask is 1"
        z = np.zeros_like(A)
        return dict(term=0.0, head_terms=np.zeros(H), bound=0.0, grad=z, grad_bound=z, exact_zero=True)
    ok = (np.abs(d) >= sign_margin(hw) * (cm + rm)) | ((cm == 0) & (rm == 0))
    assert ok.all(), f"ref inputs: |d| within {sign_margin(hw):.2e} (cm + rm) of zero at {int((~ok).sum())} pixels: sign(d) is not pinned"
    sg = np.sign(d)
    sc = (sg * cm).sum(1)
    c = scale / H * ci
    grad = c[:, None] * M[None, :] * (sg - sc[:, None])
    heads = np.abs(d).sum(1)
    mag = 2 * (cm + rm).sum(1)
    gb = SAFE * (4 * steps(hw) + 41) * U * np.abs(c)[:, None] * M[None, :]
    return dict(term=scale * heads.sum() / H, head_terms=heads, bound=SAFE * (steps(hw) + H + CONST) * U * abs(scale) / H * mag.sum(),
                grad=grad, grad_bound=gb)


def reference(t, attn):
    """fp64 restatement of one term over its attention map ``attn`` fp32 [heads, hw, n_tok]"""
    A = column(attn, t["token"])
    assert np.isfinite(A).all() and (A >= 0).all(), "the term's own column must be finite and non-negative"
    r = {"topk": _topk, "ratio": _ratio, "ref": _ref}[t["kind"]](t, A)
    r["kind"] = t["kind"]
    return r


# ---- the checkers ----------------------------------------------------------------------------------------------------------------------
def _add_tol(before, g):
    return SAFE * U * (np.abs(before) + np.abs(g))


def check_topk_column(ref, before, after):
    """``before`` / ``after``: the term's gradient column [heads, hw] (fp32 values) around ONE top-k term.  -> (violations, worst err / bound)"""
    before, after = _np64(before), _np64(after)
    bad, worst = [], 0.0
    M = ref["mask"]
    for h in range(before.shape[0]):
        for name, s, own in (("fg", ref["fg"][h], M == 1), ("bg", ref["bg"][h], M == 0)):
            v = s["value"]
            tol = TOPK_GRAD_ULPS * U * np.abs(v) + _add_tol(before[h], v)
            err = np.abs(after[h] - (before[h] + v))
            moved, kept = err <= tol, after[h] == before[h]
            shows = own & (v != 0)
            for what, where, good in (("greater not selected", s["greater"] & shows, moved), ("less selected", s["less"] & shows, kept),
                                      ("tie neither selected nor left", s["tie"] & shows, moved | kept),
                                      ("written where the contribution is zero", own & (v == 0), kept)):
                n = int((where & ~good).sum())
                if n:
                    bad.append(f"head {h} {name}: {what} at {n} pixels (first {int(np.argmax(where & ~good))})")
            sel = s["greater"] & shows & moved
            if sel.any():
                worst = max(worst, float((err[sel] / tol[sel]).max()))
            n_sel = int((s["tie"] & shows & moved & ~kept).sum())
            if not s["lo"] <= n_sel <= s["hi"]:
                bad.append(f"head {h} {name}: {n_sel} visible ties selected, the contract admits {s['lo']}..{s['hi']} (need {s['need']}, "
                           f"{int(s['free'].sum())} free)")
    return bad, worst


def check_dense_column(refs, before, after):
    """one gradient column that one or more terms with a dense gradient add to -> (violations, worst err / bound)"""
    before, after = _np64(before), _np64(after)
    g = sum(r["grad"] for r in refs)
    if all(r.get("exact_zero") for r in refs):
        same = after == before
        return ([] if same.all() else [f"exact-zero term changed {int((~same).sum())} gradient elements"]), 0.0
    tol = sum(r["grad_bound"] for r in refs) + len(refs) * _add_tol(before, sum(np.abs(r["grad"]) for r in refs))
    err = np.abs(after - (before + g))
    ratio = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0))
    bad = []
    if ratio.max() > 1.0:
        at = np.unravel_index(np.argmax(ratio), ratio.shape)
        bad.append(f"gradient off by {ratio.max():.2f} x the bound at (head, pixel) {tuple(int(i) for i in at)}: {after[at]!r} vs "
                   f"{(before + g)[at]!r}")
    return bad, float(ratio.max())


def out_bound(refs, prefill):
    return sum(r["bound"] for r in refs) + SAFE * len(refs) * U * (abs(prefill) + sum(abs(r["term"]) for r in refs))


def check_case(case, refs, out_before, out_after, grads_before, grads_after):
    """The whole contract on one case.  ``refs[j] = reference(case.terms[j], ...)``; ``out_*`` floats (fp32 values); ``grads_*``: one fp32
    tensor per map.  Asserts; returns {"loss_ratio", "grad_ratio"}: the worst error over its bound."""
    bad = []
    want = float(out_before) + sum(r["term"] for r in refs)
    tol = out_bound(refs, float(out_before))
    err = abs(float(out_after) - want)
    if not math.isfinite(float(out_after)):
        bad.append(f"out[0] = {out_after}")
    if all(r.get("exact_zero") for r in refs):
        if float(out_after) != float(out_before):
            bad.append(f"out[0] moved from {out_before!r} to {out_after!r} by exactly-zero terms")
        loss_ratio = 0.0
    else:
        loss_ratio = err / tol
        if not loss_ratio <= 1.0:
            bad.append(f"out[0] = {float(out_after)!r}, contract {want!r}: error {err:.3e} is {loss_ratio:.2f} x the bound {tol:.3e}")
    grad_ratio = 0.0
    for m, (gb, ga) in enumerate(zip(grads_before, grads_after)):
        gb, ga = gb.detach().cpu(), ga.detach().cpu()
        if not torch.isfinite(ga).all():
            bad.append(f"map {m}: non-finite gradient (a column of another token was read?)")
        cols = {}
        for t, r in zip(case["terms"], refs):
            if t["map"] == m:
                cols.setdefault(int(t["token"]), []).append(r)
        others = [c for c in range(gb.shape[2]) if c not in cols]
        if not torch.equal(ga[:, :, others].view(torch.int32), gb[:, :, others].view(torch.int32)):
            bad.append(f"map {m}: gradient columns of other tokens changed")
        for tok, rs in cols.items():
            if len(rs) == 1 and rs[0]["kind"] == "topk":
                b, w = check_topk_column(rs[0], gb[:, :, tok], ga[:, :, tok])
            else:
                assert all(r["grad"] is not None for r in rs), "terms that share a column must leave no tie to choose"
                b, w = check_dense_column(rs, gb[:, :, tok], ga[:, :, tok])
            bad += [f"map {m} token {tok}: {x}" for x in b]
            grad_ratio = max(grad_ratio, w)
    assert not bad, f"{case['name']}: " + "; ".join(bad[:6]) + (f" (+{len(bad) - 6} more)" if len(bad) > 6 else "")
    return {"loss_ratio": loss_ratio, "grad_ratio": grad_ratio}


# ---- the cases (built on the CPU from fixed seeds: the same bits wherever they run) --------------------------------------------------------
OUT_PREFILL = 0.75


def grad_prefill(shape):
    """a non-trivial, exactly representable pattern in [0.25, 1]: shows a ``=`` in place of ``+=``"""
    n = int(np.prod(shape))
    return (0.25 + (torch.arange(n, dtype=torch.float32) % 7) * 0.125).reshape(shape)


def nan_map(cols):
    """attn [heads, hw, n_tok]: ``cols`` {token: fp32 [heads, hw]}; every other column is NaN"""
    n_tok = cols.pop("n_tok")
    first = next(iter(cols.values()))
    a = torch.full((first.shape[0], first.shape[1], n_tok), float("nan"), dtype=torch.float32)
    for tok, c in cols.items():
        a[:, :, tok] = c
    return a.contiguous()


def _gen(*key):
    return torch.Generator().manual_seed(int(sum((i + 1) * 1009 * int(v) for i, v in enumerate(key))) + 5)


def _rand_mask(hw, g):
    if hw == 1:
        return torch.ones(1)
    m = (torch.rand(hw, generator=g) < 0.35).float()
    one = int(torch.randint(0, hw, (1,), generator=g))                  # at least one pixel inside and one outside
    m[one] = 1.0
    m[(one + 1 + int(torch.randint(0, hw - 1, (1,), generator=g))) % hw] = 0.0
    return m


def _prob_cols(heads, hw, g):
    """tie-free positive columns, scaled like softmax rows over 77 tokens"""
    return (torch.rand(heads, hw, generator=g) * 0.9 + 0.05) / 40.0


def _term(kind, m, token, mask, scale, **kw):
    return dict(kind=kind, map=m, token=int(token), mask=mask.contiguous(), scale=float(scale), **kw)


def _k(mask, p=0.2):
    """k of the reference (utils/guidance.py:136-137): fp32 product, truncated, at least 1"""
    n = mask.sum()
    return max(1, int((n * p).long())), max(1, int(((1 - mask).sum() * p).long()))


def trio(name, heads, hw, n_tok, tokens, seed=0, k=None, mul=1.0):
    """one top-k, one ratio and one ref term, each on a map of its own [heads, hw, n_tok] at ``tokens[j]``; ``mul`` scales the maps (the
    header asks for fp32 maps, not for probabilities: x 160 puts values on both sides of 2.0, bit 30 of the pattern the select walks)"""
    maps, terms = [], []
    for j, kind in enumerate(KINDS):
        g = _gen(heads, hw, n_tok, seed, j)
        maps.append(nan_map({"n_tok": n_tok, tokens[j]: _prob_cols(heads, hw, g) * mul}))
        mask = _rand_mask(hw, g)
        if kind == "topk":
            k_fg, k_bg = k if k is not None else _k(mask)
            terms.append(_term(kind, j, tokens[j], mask, 0.25, k_fg=k_fg, k_bg=k_bg, fg_w=1.0, bg_w=4.0))
        elif kind == "ratio":
            terms.append(_term(kind, j, tokens[j], mask, 0.125))
        else:
            terms.append(_term(kind, j, tokens[j], mask, 0.5, ref=_prob_cols(heads, hw, g).contiguous(), eps=1e-5))
    return dict(name=name, maps=maps, terms=terms)


def box_mask(H, W, y0, y1, x0, x1):
    m = torch.zeros(H, W)
    m[y0:y1, x0:x1] = 1
    return m.reshape(-1)


def straddling_ties(seed, top_p=0.2):
    """three value levels on a 12 x 12 map, 10 heads: every (head, side) has 0 < thr, need >= 2, more visible ties than need, spread over
    at least two 64-lane chunks (asserted by the tests).  top_p = 0.2 (k = 9 / 19) puts the threshold on the top level: everything selected
    is a tie; top_p = 0.5 (k = 24 / 48) puts it on the middle level: the ties sit under a non-empty strictly-greater set."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(1, 4, (10, 144), generator=g).float() / 8
    mask = box_mask(12, 12, 3, 9, 2, 10)
    k_fg, k_bg = _k(mask, top_p)
    assert (k_fg, k_bg) == ((9, 19) if top_p == 0.2 else (24, 48))
    return dict(name=f"straddling_ties_s{seed}" if top_p == 0.2 else f"ties_under_greater_s{seed}", maps=[nan_map({"n_tok": 5, 2: a})],
                terms=[_term("topk", 0, 2, mask, 0.25, k_fg=k_fg, k_bg=k_bg, fg_w=1.0, bg_w=4.0)])


def straddle_preconditions(ref):
    for s in ref["fg"] + ref["bg"]:
        chunks = set((np.nonzero(s["shown"])[0] // 64).tolist())
        assert s["thr"] > 0 and s["need"] >= 2 and int(s["shown"].sum()) > s["need"] and len(chunks) >= 2, \
            (s["thr"], s["need"], int(s["shown"].sum()), chunks)


def ties_at_zero():
    """k exceeds the number of non-zero entries on both sides: thr == 0, the tie set is the zeros (visible ones and free ones)"""
    heads, hw = 3, 65
    g = _gen(3, 65, 1)
    mask = torch.zeros(hw)
    mask[torch.tensor([1, 5, 9, 20, 33, 40, 47, 63, 64, 12])] = 1
    a = torch.zeros(heads, hw)
    for h in range(heads):
        a[h, torch.tensor([5, 40, 64])] = torch.rand(3, generator=g) + 0.1              # 3 of the 10 box pixels
        a[h, torch.tensor([0, 30, 62, 50])] = torch.rand(4, generator=g) + 0.1          # 4 of the 55 outside
    return dict(name="ties_at_zero", maps=[nan_map({"n_tok": 3, 1: a})],
                terms=[_term("topk", 0, 1, mask, 0.5, k_fg=5, k_bg=7, fg_w=1.0, bg_w=2.0)])


def host_box(name, box, n_in):
    """a box that goes through the host path (guidance.add_ca_loss_per_attn_map_to_loss): the host computes mask and k"""
    heads, H = 5, 8
    g = _gen(heads, H, n_in)
    mask = torch.ones(H * H) if n_in else torch.zeros(H * H)
    k_fg, k_bg = _k(mask)
    assert (k_fg, k_bg) == ((12, 1) if n_in else (1, 12))
    return dict(name=name, maps=[nan_map({"n_tok": 3, 1: _prob_cols(heads, H * H, g)})], host=dict(box=box, top_p=0.2, fg_w=1.0, bg_w=4.0),
                terms=[_term("topk", 0, 1, mask, 0.25, k_fg=k_fg, k_bg=k_bg, fg_w=1.0, bg_w=4.0)])


def denormals():
    """distinct denormals (1e-40 and up) inside the box, ordinary values outside: the select must still order them (a flushed compare
    sees 20 equal zeros and takes the first four by index)"""
    heads, hw = 2, 65
    g = _gen(2, 65, 40)
    mask = torch.zeros(hw)
    inside = torch.arange(3, 63, 3)                                  # 20 pixels
    mask[inside] = 1
    a = _prob_cols(heads, hw, g)
    for h in range(heads):
        order = torch.randperm(20, generator=g)
        vals = np.float32(1e-40) * (1 + order.numpy()).astype(np.float32)
        assert np.all(vals > 0) and np.all(vals < np.finfo(np.float32).tiny) and len(set(vals.tolist())) == 20
        a[h, inside] = torch.from_numpy(vals)
        assert set(torch.topk(a[h, inside], 4).indices.tolist()) != {0, 1, 2, 3}
    return dict(name="denormals", maps=[nan_map({"n_tok": 2, 0: a})],
                terms=[_term("topk", 0, 0, mask, 0.5, k_fg=4, k_bg=9, fg_w=1.0, bg_w=1.0)])


def ref_exact_zero(empty_mask):
    heads, hw = 5, 65
    g = _gen(5, 65, 7, int(empty_mask))
    a = _prob_cols(heads, hw, g)
    mask = torch.zeros(hw) if empty_mask else _rand_mask(hw, g)
    ref = _prob_cols(heads, hw, g) if empty_mask else a.clone()      # empty mask: 1 / eps on both sides, every product is 0
    return dict(name="ref_empty_mask" if empty_mask else "ref_d_zero", maps=[nan_map({"n_tok": 3, 2: a})],
                terms=[_term("ref", 0, 2, mask, 0.5, ref=ref.contiguous(), eps=1e-5, exact_zero=True)])


def plan_mixed():
    """all three kinds in one launch, heads 5 / 10 / 20 and hw 16 / 64 / 144, each (heads, hw) once as top-k and once not: blocks past an
    item's last head group return early, head_terms rows are max_heads = 20 apart, the LDS is sized by the largest top-k map"""
    maps, terms = [], []
    for j, (kind, heads, hw) in enumerate((("topk", 5, 16), ("ratio", 10, 64), ("ref", 20, 144), ("ref", 5, 16), ("topk", 10, 64),
                                           ("ratio", 20, 144), ("topk", 20, 144))):
        g = _gen(heads, hw, j, 99)
        tok = j % 3
        maps.append(nan_map({"n_tok": 3, tok: _prob_cols(heads, hw, g)}))
        mask = _rand_mask(hw, g)
        if kind == "topk":
            k_fg, k_bg = _k(mask)
            terms.append(_term(kind, j, tok, mask, 0.0625, k_fg=k_fg, k_bg=k_bg, fg_w=1.0, bg_w=4.0))
        elif kind == "ratio":
            terms.append(_term(kind, j, tok, mask, 0.0625))
        else:
            terms.append(_term(kind, j, tok, mask, 0.125, ref=_prob_cols(heads, hw, g).contiguous(), eps=1e-5))
    return dict(name="plan_mixed", maps=maps, terms=terms)


def flush_collision():
    """two objects share token 2 of one map (two top-k terms with different boxes) and a ref term lands on the same column: one launch
    may hold only one of them (the host defers the others); a ratio term on token 0 shares nothing"""
    heads, H = 5, 8
    g = _gen(5, 8, 2, 2)
    m = nan_map({"n_tok": 4, 2: _prob_cols(heads, H * H, g), 0: _prob_cols(heads, H * H, g)})
    m1, m2 = box_mask(H, H, 1, 5, 0, 4), box_mask(H, H, 3, 8, 2, 7)
    terms = [_term("topk", 0, 2, m1, 0.125, k_fg=_k(m1)[0], k_bg=_k(m1)[1], fg_w=1.0, bg_w=4.0),
             _term("ratio", 0, 0, m1, 0.125),
             _term("topk", 0, 2, m2, 0.125, k_fg=_k(m2)[0], k_bg=_k(m2)[1], fg_w=1.0, bg_w=4.0),
             _term("ref", 0, 2, m2, 0.25, ref=_prob_cols(heads, H * H, g).contiguous(), eps=1e-5)]
    return dict(name="flush_collision", maps=[m], terms=terms, collides=True)


def lds_large():
    """46 x 46 = 2116 pixels, 4 heads: 4 waves x 2 x 2116 floats + 4 = 67728 bytes, the smallest square map above 64 KB of dynamic LDS"""
    heads, H = 4, 46
    g = _gen(4, 46)
    mask = box_mask(H, H, 10, 30, 5, 25)
    k_fg, k_bg = _k(mask)
    return dict(name="lds_above_64k", maps=[nan_map({"n_tok": 2, 1: _prob_cols(heads, H * H, g)})],
                terms=[_term("topk", 0, 1, mask, 0.25, k_fg=k_fg, k_bg=k_bg, fg_w=1.0, bg_w=4.0)])


def many_items():
    """300 ratio terms, one per token of one 1-head 2 x 2 map: the plan form's fold adds items in chunks of 256, this takes it into the second"""
    g = _gen(300, 4)
    a = _prob_cols(300, 4, g).t().reshape(1, 4, 300).contiguous()
    mask = torch.tensor([1.0, 0.0, 0.0, 1.0])
    return dict(name="items_over_256", maps=[a], terms=[_term("ratio", 0, tok, mask, 2.0 ** -6) for tok in range(300)])


def _build_cases():
    cs = [straddling_ties(s) for s in (0, 1, 2)] + [straddling_ties(3, 0.5)]
    cs += [ties_at_zero(), host_box("empty_box", (0.5, 0.5, 0.5, 0.5), 0), host_box("whole_image_box", (0.0, 0.0, 1.0, 1.0), 64)]
    cs += [trio(f"heads_{h}", h, 65, 4, (0, 1, 3), seed=1) for h in (1, 3, 5, 10)]
    cs += [trio(f"hw_{hw}", 5, hw, 3, (1, 2, 0), seed=2) for hw in (1, 4, 63, 64, 65, 129)]
    cs += [trio("k_is_1", 3, 65, 3, (1, 1, 1), seed=3, k=(1, 1)), trio("k_is_hw", 3, 65, 3, (1, 1, 1), seed=4, k=(65, 65))]
    cs += [trio("token_first", 5, 64, 5, (0, 0, 0), seed=5), trio("token_last", 5, 64, 5, (4, 4, 4), seed=6),
           trio("one_token", 5, 64, 1, (0, 0, 0), seed=7), trio("values_around_2", 3, 65, 3, (2, 0, 1), seed=8, mul=160.0)]
    cs += [denormals(), ref_exact_zero(False), ref_exact_zero(True), plan_mixed(), flush_collision(), lds_large(), many_items()]
    return {c["name"]: c for c in cs}


_CASES = None


def cases():
    """{name: case}: every GPU case of tests/test_guidance_edges_gpu.py (built once, never modified: tests clone what they write to)"""
    global _CASES
    if _CASES is None:
        _CASES = _build_cases()
    return _CASES


_REFS = {}


def case_refs(name):
    """the fp64 references of a case's terms, computed once and shared"""
    if name not in _REFS:
        c = cases()[name]
        _REFS[name] = [reference(t, c["maps"][t["map"]]) for t in c["terms"]]
    return _REFS[name]
