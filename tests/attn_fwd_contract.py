"""The C-ABI contracts of ``tg_attention`` / ``tg_attention_ps`` and ``tg_attn_probs`` (include/theatergen_hip.h: ``tg_attn_desc``) for checking
single launches of the forward flash kernel (csrc/tg_attention.hip), in the style of tests/attn_bwd_contract.py.

A descriptor is a plain dict with the header's field names (``ip_scale_count`` of tg_attention_ps included; ``mask`` is a pointer with the three
strides ``mask_bs`` / ``mask_hs`` / ``mask_qs``); tensors stand for the pointers.  Operands are read through ``gemm_contract.Region`` along the
descriptor's pitches, never through a tensor's logical shape.  The fp64 restatement is ``gemm_contract.attention_reference`` (extended there: the
strided mask, one ``w1_dev`` float per batch item, causal and mask together); this module adds no second one.

    O = softmax(s Q K0^T + mask [causal]) V0  +  w1[b] softmax(s Q K1^T) V1

  * ``reference(a)`` fp64 [batch, n_q, heads * head_dim]; ``floor(a)``: the same rounded once to the storage dtype (what no kernel can beat)
  * ``read_extents`` / ``written_region``: ``Region`` lists (V^T columns from ``len`` on, pad columns, gap rows and mask rows that no
        (item, head, query) addresses are NOT read)
  * ``instance(a)`` -> (DPAD, DV, ONES, FOLD, MASK): a Python statement of ``dispatch_attn``
  * ``model(a)``: an fp32 restatement that follows the kernel's SCHEDULE: 64-key tiles; the reference of the online softmax moves lazily, the
        decision taken per wave of 32 query rows (rows >= n_q of the last block take part as zero queries) when a row's tile max exceeds it by
        more than ``LAZY_LOG2`` = 8 in exp2 units; P rounded to the storage dtype where it enters PV; the ONES instances sum the denominator
        from the ROUNDED P (the PV MFMA accumulates it from a row of ones), the others from the fp32 exponentials; FOLD (head dim 40, no mask)
        rounds ``Q * scale * log2 e`` to the storage dtype and keeps a storage-dtype reference; MASK adds ``mask / scale`` in raw-score units
        and, while a row has seen no visible key, uses the reference 0; segment 1 with its own softmax and ``w1 / l1`` folded into P before the
        rounding; fp32 accumulation tile by tile, one final rounding.
        ``model(a, strict_max=True)``: the same contract with a strict per-row running max and no FOLD rounding, a second legitimate
        implementation.  ``fold_rounding=True`` keeps FOLD's rounded query and storage-dtype reference under the strict max (the second
        implementation the FOLD cases are compared with).  ``fault=`` injects one of ``FAULTS`` (tests/test_attn_fwd_contract_cpu.py),
        ``inf_fix=False`` is the MASK instance before the reference-0 rule and the far-reference rule (a reference of 2^24 exp2 units or
        more is subtracted before the multiply).  ``info``: a dict that receives ``rescales`` (tiles after the first at which a wave moved
        its reference) and ``p_max`` (the largest rounded P).
  * ``compare(got, ref, heads)``: whole-tensor rel-L2 and max|err| / max|ref|, and ``block_rel_l2``: the unit is (batch item, head, 128-query
        block) x the head's columns, what one workgroup owns.  A ragged last block of fewer than ``MERGE_BELOW`` = 8 rows is merged into the block
        before it for THIS figure only: two legitimate fp32 models (lazy and strict) differ by up to 1.50x in the worst block when that block
        is a single row and by at most 1.34x at 8 rows, measured on the CPU; max-rel and the bit checks still see the row alone.
  * ``bounds(a)``: the project's norm rule, nothing tuned on the kernel: 1.5x the model's whole-tensor rel-L2, 1.5x its worst block, 2x its
        max-rel, from the case's own operands.

``tg_attn_probs`` (fp32 out, one wave per query row): ``probs_reference`` fp64 (``tokens`` gather and ``b0`` included), ``probs_model`` fp32, and
``probs_bound``, an element-by-element operation count with u = 2^-24.  Products of two bf16 / fp16 values are exact in fp32 (16 / 22
significand bits), so a score carries the ``head_dim`` additions of its chain and the multiply by ``scale``:
        |ds_j| <= (head_dim + 1) u A_j,     A_j = |scale| sum_c |q_c k_jc|
``sc - mx`` is one rounding of x_j = s_j - max <= 0 and inherits ds_j and ds_max; ``__expf(x)`` is ``v_exp_f32(x * log2 e)``: the multiply is one
rounding (|x_j| u on the argument, so |x_j| u relative on the result) and the instruction is good to 1 ulp (2 u allowed).  Relative error of e_j:
        d_j = u ((head_dim + 1) (A_j + A_max) + 2 |x_j| + 2),   A_max = max_j A_j
The wave sum is 3 additions in the lane and 6 across lanes of positive terms: relative (sum_i p_i d_i) + 9 u.  One reciprocal (2 u: the
division may be a refined v_rcp_f32) and one multiply (u).  So
        |p^_j - p_j| <= p_j (d_j + sum_i p_i d_i + 12 u) + 2^-126            (the last term: results under the normal range may flush to 0)
to first order; second-order terms are under 1e-3 of the bound at head_dim <= 160 and |x| < 2^10.
"""
import math

import numpy as np
import torch

from tests import gemm_contract as gc
from tests.gemm_contract import Region, _rd

BLOCK, KV, WAVE, LAZY_LOG2, MERGE_BELOW = 128, 64, 32, 8.0, 8
LOG2E32 = np.float32(1.4426950408889634)
NAN, INF = float("nan"), float("inf")

FIELDS = ("batch", "heads", "head_dim", "n_q", "q", "q_ld", "q_bs", "k0", "k0_ld", "k0_bs", "vt0", "vt0_ld", "vt0_bs", "len0", "k1", "k1_ld",
          "k1_bs", "vt1", "vt1_ld", "vt1_bs", "len1", "scale", "w1", "out", "out_ld", "out_bs", "causal", "w1_dev", "mask", "mask_bs", "mask_hs",
          "mask_qs", "ip_scale_count")

FAULTS = ("vt_tail", "drop_last_key", "extra_key", "causal_strict", "causal_no_qblk", "mask_qs_ignored", "mask_hs_ignored", "mask_bs_ignored",
          "mask_no_inv_scale", "mask_on_seg1", "seg1_l0", "w1_on_seg0", "w1_dev0", "head_dpad", "qblk_rows", "no_rescale", "fold_ref_not_reset")


def read_extents(a):
    return gc.attention_read_extents(a)


def written_region(a):
    return gc.attention_written_region(a)


def reference(a):
    return gc.attention_reference(**a)


def floor(a):
    return reference(a).to(a["q"].dtype).to(torch.float64)


def instance(a):
    """``dispatch_attn`` -> (DPAD, DV, ONES, FOLD, MASK): nine unmasked instances, eight masked"""
    hd, masked = int(a["head_dim"]), a.get("mask") is not None
    for top, dv, ones in ((16, 32, True), (32, 32, False), (48, 64, True), (64, 64, False), (80, 96, True), (96, 96, False), (128, 128, False),
                          (160, 160, False)):
        if hd <= top:
            return top, dv, ones, hd == 40 and not masked, masked
    raise ValueError(f"head_dim {hd}")


ALL_INSTANCES = {(dp, dv, on, False, m) for dp, dv, on in ((16, 32, True), (32, 32, False), (48, 64, True), (64, 64, False), (80, 96, True),
                                                           (96, 96, False), (128, 128, False), (160, 160, False)) for m in (False, True)} | \
                {(48, 64, True, True, False)}


# ---- test operands -----------------------------------------------------------------------------------------------------------------
def _up8(n):
    return (n + 7) // 8 * 8


def _pitched_rows(src, B, n, inner, ld, gap, dtype, device, col0=0):
    """[B * (n + gap), ld] NaN buffer with src[b] in rows b (n + gap) .. + n, columns col0 .. col0 + inner -> (the operand view, bs)"""
    buf = torch.full((B * (n + gap), ld), NAN, dtype=dtype, device=device)
    for b in range(B):
        buf[b * (n + gap):b * (n + gap) + n, col0:col0 + inner] = src[b]
    return buf[:, col0:col0 + inner], (n + gap) * ld


def _vt(src, B, n, inner, ld, dtype, device):
    """V^T [B, inner, ld]: columns < n = src^T, NaN from n on"""
    buf = torch.full((B, inner, ld), NAN, dtype=dtype, device=device)
    buf[:, :, :n] = src.transpose(1, 2)
    return buf


MASK_KINDS = ("zero", "rand", "m1e4", "big_some", "big_row", "inf_part", "inf_tile0", "fmin")


def mask_values(kind, Bm, Hm, Qm, L, g):
    """fp32 [Bm, Hm, Qm, L].  ``rand``: N(0, 1) plus -10000 on a tenth of the keys, every (item, head, row) different (the layout cases);
    ``big_some`` / ``inf_part``: -1e30 / -inf on keys 3 .. min(40, L - 1) of every other row; ``big_row``: -1e30 on EVERY key of every third
    row; ``inf_tile0`` / ``fmin``: -inf / finfo.min on keys 0 .. 63 (the whole first tile) and on key L - 2, of every row but each fifth"""
    m = torch.zeros((Bm, Hm, Qm, L))
    if kind == "zero":
        return m
    if kind in ("rand", "m1e4"):
        hit = torch.rand((Bm, Hm, Qm, L), generator=g) < 0.1
        hit[..., L // 2] = False
        m = torch.randn((Bm, Hm, Qm, L), generator=g) if kind == "rand" else m
        return m.masked_fill(hit, -10000.0)
    if kind in ("big_some", "inf_part"):
        m[:, :, ::2, 3:min(40, L - 1)] = -1e30 if kind == "big_some" else -INF
        return m
    if kind == "big_row":
        m[:, :, ::3, :] = -1e30
        return m
    assert kind in ("inf_tile0", "fmin") and L > KV + 2, (kind, L)
    v = -INF if kind == "inf_tile0" else float(torch.finfo(torch.float32).min)
    rows = torch.ones(Qm, dtype=torch.bool)
    rows[4::5] = False
    m[:, :, rows, :KV] = v
    m[:, :, rows, L - 2] = v
    return m


def make_mask(kind, B, H, n_q, L, *, bs=True, hs=False, qs=True, pitch=0, device="cpu", seed=0):
    """-> (pointer tensor, mask_bs, mask_hs, mask_qs): rows of pitch L + ``pitch`` in one NaN-filled storage with a guard row in front and
    behind; a zero stride broadcasts.  Only the L leading elements of the rows the strides address hold values."""
    Bm, Hm, Qm, P = (B if bs else 1), (H if hs else 1), (n_q if qs else 1), L + pitch
    g = torch.Generator().manual_seed(7000 + 31 * seed + L + 3 * n_q + MASK_KINDS.index(kind))
    vals = mask_values(kind, Bm, Hm, Qm, L, g)
    store = torch.full(((Bm * Hm * Qm + 2), P), NAN)
    store[1:-1, :L] = vals.reshape(-1, L)
    store = store.to(device)
    return store[1:], (Hm * Qm * P if bs else 0), (Qm * P if hs else 0), (P if qs else 0)


def make_case(dtype, B, n_q, len0, heads, d, *, len1=0, device="cpu", seed=0, qmul=1.0, kmul=1.0, scale=None, w1=0.4, w1_dev=None,
              ip_scale_count=None, causal=False, mask=None, mask_layout=None, plain=False):
    """a ``tg_attn_desc`` with N(0, 1) q (x ``qmul``), k (x ``kmul``) and v drawn on the CPU from ``seed`` (the same bits on every device).
    Every element the contract does not read is NaN: q rows of pitch inner + 8 with two gap rows after every item; k0 the RIGHT half of a
    fused [batch * (len0 + 1), 2 inner + 8] buffer (the left half, the pad columns and the gap row are NaN); vt0 of pitch roundup8(len0) + 8
    with NaN from column len0 on; k1 / vt1 likewise; out of pitch inner + 4 with a gap row.  ``plain``: dense operands.
    ``mask``: a kind of ``MASK_KINDS``; ``mask_layout``: keywords of ``make_mask``.  ``w1_dev``: a list of floats (device weights)."""
    inner = heads * d
    g = torch.Generator().manual_seed(1000 * seed + 17 * B + n_q + 5 * len0 + 3 * heads + d + 7 * len1)
    rnd = lambda n, mul: (torch.randn((B, n, inner), generator=g) * mul).to(dtype)       # noqa: E731
    q, k0, v0 = rnd(n_q, qmul), rnd(len0, kmul), rnd(len0, 1.0)
    k1, v1 = (rnd(len1, kmul), rnd(len1, 1.0)) if len1 > 0 else (None, None)
    return assemble(dtype, B, heads, d, q, k0, v0, k1, v1, device=device, seed=seed, scale=scale, w1=w1, w1_dev=w1_dev,
                    ip_scale_count=ip_scale_count, causal=causal, mask=mask, mask_layout=mask_layout, plain=plain)


def assemble(dtype, B, heads, d, q, k0, v0, k1=None, v1=None, *, device="cpu", seed=0, scale=None, w1=0.4, w1_dev=None, ip_scale_count=None,
             causal=False, mask=None, mask_layout=None, plain=False):
    """the descriptor of ``make_case`` around given [B, n, inner] operands"""
    inner, n_q, len0 = heads * d, q.shape[1], k0.shape[1]
    len1 = 0 if k1 is None else k1.shape[1]
    gap_q, gap_k, gap_o, pad = (0, 0, 0, 0) if plain else (2, 1, 1, 8)
    a = dict(batch=B, heads=heads, head_dim=d, n_q=n_q, len0=len0, len1=len1, scale=float(scale if scale is not None else d ** -0.5),
             w1=float(w1), causal=1 if causal else 0, w1_dev=None, mask=None, mask_bs=0, mask_hs=0, mask_qs=0, ip_scale_count=ip_scale_count,
             k1=None, k1_ld=0, k1_bs=0, vt1=None, vt1_ld=0, vt1_bs=0)
    a["q_ld"] = inner + pad
    a["q"], a["q_bs"] = _pitched_rows(q, B, n_q, inner, a["q_ld"], gap_q, dtype, device)
    a["k0_ld"] = inner if plain else 2 * inner + pad
    a["k0"], a["k0_bs"] = _pitched_rows(k0, B, len0, inner, a["k0_ld"], gap_k, dtype, device, col0=0 if plain else inner)
    a["vt0_ld"] = _up8(len0) + pad
    a["vt0"], a["vt0_bs"] = _vt(v0, B, len0, inner, a["vt0_ld"], dtype, device), inner * a["vt0_ld"]
    if len1 > 0:
        a["k1_ld"] = inner + pad
        a["k1"], a["k1_bs"] = _pitched_rows(k1, B, len1, inner, a["k1_ld"], gap_k, dtype, device)
        a["vt1_ld"] = _up8(len1) + pad
        a["vt1"], a["vt1_bs"] = _vt(v1, B, len1, inner, a["vt1_ld"], dtype, device), inner * a["vt1_ld"]
    a["out_ld"] = inner + pad // 2
    a["out"] = torch.full((B * (n_q + gap_o), a["out_ld"]), NAN, dtype=dtype, device=device)[:, :inner]
    a["out_bs"] = (n_q + gap_o) * a["out_ld"]
    if w1_dev is not None:
        store = torch.full((len(w1_dev) + 2,), NAN)
        store[1:-1] = torch.tensor(w1_dev, dtype=torch.float32)
        a["w1_dev"] = store.to(device)[1:]
        # the pointer must be 4-byte aligned only; ip_scale_count None = tg_attention (one float)
    if mask is not None:
        a["mask"], a["mask_bs"], a["mask_hs"], a["mask_qs"] = make_mask(mask, B, heads, n_q, len0, device=device, seed=seed, **(mask_layout or {}))
    assert set(a) == set(FIELDS), set(a) ^ set(FIELDS)
    return a


def spike_case(dtype, B, n_q, len0, heads, d, *, spike_key, log2_above, device="cpu", seed=0, mask=None, len1=0):
    """softmax-range operands: column 0 of every head is a bias channel (q = 1, k = b_j), the other columns N(0, 0.05) (scores within a few
    hundredths of an exp2 unit), so every row's reference after a tile without a spike is ~0 and key ``spike_key`` scores ``log2_above``
    exp2 units (up to the rounding of b to the storage dtype) above it.  v is N(0, 1)."""
    inner = heads * d
    g = torch.Generator().manual_seed(5000 + 13 * seed + len0 + d + spike_key)
    rnd = lambda n, std: torch.randn((B, n, inner), generator=g) * std       # noqa: E731
    q, k0, v0 = rnd(n_q, 0.05), rnd(len0, 0.05), rnd(len0, 1.0)
    c = float(np.float32(d ** -0.5) * LOG2E32)
    q[:, :, ::d] = 1.0
    k0[:, :, ::d] = 0.0
    k0[:, spike_key, ::d] = log2_above / c
    k1, v1 = (rnd(len1, 0.05), rnd(len1, 1.0)) if len1 > 0 else (None, None)
    if k1 is not None:
        k1[:, :, ::d] = 0.0
    cast = lambda t: None if t is None else t.to(dtype)       # noqa: E731
    return assemble(dtype, B, heads, d, cast(q), cast(k0), cast(v0), cast(k1), cast(v1), device=device, seed=seed, mask=mask)


# ---- the fp32 model ------------------------------------------------------------------------------------------------------------------
def _fma(x, c, y):
    """fp32 fma(x, c, y): one rounding"""
    return (x.double() * c + y.double()).float()


def model(a, strict_max=False, fault=None, inf_fix=True, info=None, fold_rounding=None):
    """fp64 [batch, n_q, heads * head_dim] holding storage-dtype values: the schedule-faithful fp32 restatement (module docstring)"""
    assert fault is None or fault in FAULTS, fault
    B, H, D, nq, L0, L1 = (int(a[x]) for x in ("batch", "heads", "head_dim", "n_q", "len0", "len1"))
    dpad, _, ones, fold, masked = instance(a)
    fold = fold and (not strict_max if fold_rounding is None else bool(fold_rounding))
    dtype, f32 = a["q"].dtype, torch.float32
    rd = lambda x: x.to(dtype).to(f32)       # noqa: E731
    scale32 = np.float32(a["scale"])
    c, inv_scale = float(np.float32(scale32 * LOG2E32)), float(np.float32(1.0) / scale32)
    hoff = dpad if fault == "head_dpad" else D

    def rows(name, n, ld, bs):                               # [B, H, n, D]
        return torch.stack([_rd(a[name], h * hoff, (B, n, D), (bs, ld, 1)) for h in range(H)], 1).to(f32)

    def cols(name, n, ld, bs):                               # [B, H, D, n]
        return torch.stack([_rd(a[name], h * D * ld, (B, D, n), (bs, ld, 1)) for h in range(H)], 1).to(f32)      # (the head fault: q and k only)

    dev = a["q"].device
    nqp = (nq + BLOCK - 1) // BLOCK * BLOCK
    qrow = torch.arange(nqp, device=dev)
    q = torch.zeros((B, H, nqp, D), dtype=f32, device=dev)
    q[:, :, :nq] = rows("q", nq, a["q_ld"], a["q_bs"])
    if fault == "qblk_rows":
        q = q[:, :, qrow % BLOCK]
    qf = rd(q * c) if fold else q
    wave_any = lambda w: w.reshape(B, H, nqp // WAVE, WAVE).any(-1, keepdim=True).expand(-1, -1, -1, WAVE).reshape(B, H, nqp)       # noqa: E731

    M = None
    if masked:
        mbs, mhs, mqs = gc.attention_mask_strides(a)
        mbs, mhs, mqs = (0 if fault == "mask_bs_ignored" else mbs), (0 if fault == "mask_hs_ignored" else mhs), \
                        (0 if fault == "mask_qs_ignored" else mqs)
        M = torch.zeros((B, H, nqp, L0), dtype=f32, device=dev)
        M[:, :, :nq] = _rd(a["mask"], 0, (B, H, nq, L0), (mbs, mhs, mqs, 1))
        M[:, :, nq:] = M[:, :, :1]                           # rows >= n_q address row 0
        M = M * (1.0 if fault == "mask_no_inv_scale" else inv_scale)

    # segment 0
    hi = L0 - 1 if fault == "drop_last_key" else (L0 + 1 if fault == "extra_key" else L0)       # keys below ``hi`` count
    Lr = max(hi, _up8(L0) if fault == "vt_tail" else hi)                                           # V^T columns multiplied
    K = torch.zeros((B, H, Lr, D), dtype=f32, device=dev)
    K[:, :, :hi] = rows("k0", hi, a["k0_ld"], a["k0_bs"])
    V = cols("vt0", Lr, a["vt0_ld"], a["vt0_bs"])
    o = torch.zeros((B, H, nqp, D), dtype=f32, device=dev)
    l = torch.zeros((B, H, nqp), dtype=f32, device=dev)
    m = torch.full((B, H, nqp), -INF, dtype=f32, device=dev)
    qbias = torch.zeros((B, H, nqp), dtype=f32, device=dev)
    rescales, p_max = 0, 0.0
    for t in range((L0 + KV - 1) // KV):
        j0, j1 = t * KV, min(t * KV + KV, Lr)
        keys = torch.arange(j0, j1, device=dev)
        s = qf @ K[:, :, j0:j1].transpose(2, 3)
        if fold:
            s = s + qbias[..., None]
        hidden = (keys >= hi)[None, :].expand(nqp, -1)
        if a["causal"]:
            qi = (qrow % BLOCK if fault == "causal_no_qblk" else qrow)[:, None]
            hidden = hidden | ((keys[None, :] >= qi) if fault == "causal_strict" else (keys[None, :] > qi))
        s = s.masked_fill(hidden, -INF)
        if masked:
            mm = torch.zeros_like(s)
            w = min(j1, L0) - j0
            mm[..., :w] = M[..., j0:j0 + w]
            s = s + mm
        tm = s.amax(-1)
        if fold:
            W = torch.ones_like(tm, dtype=torch.bool) if t == 0 else ((tm > 0.0) if strict_max else wave_any(tm > LAZY_LOG2))
            if fault == "no_rescale" and t > 0:
                W = torch.zeros_like(W)
            sh = tm if t == 0 else tm.clamp_min(0.0)
            nb = rd(qbias - sh)
            delta = torch.where(W, nb - qbias, torch.zeros_like(nb))
            alpha = torch.ones_like(delta) if t == 0 else torch.exp2(delta)
            s = s + delta[..., None]
            qbias = torch.where(W, nb, qbias)
            e = torch.exp2(s)
        else:
            if strict_max:
                W = tm > m
            else:
                W = wave_any(tm * c > m * c + LAZY_LOG2)
            if fault == "no_rescale" and t > 0:
                W = torch.zeros_like(W)
            m_new = torch.maximum(m, tm)
            alpha = torch.exp2((m - m_new) * c)
            if masked and inf_fix:
                alpha = torch.where(m_new == -INF, torch.ones_like(alpha), alpha)
            alpha = torch.where(W, alpha, torch.ones_like(alpha))
            m = torch.where(W, m_new, m)
            mc = m * c
            if masked and inf_fix:
                mc = torch.where(m == -INF, torch.zeros_like(mc), mc)
                far = mc.abs() >= 2.0 ** 24                       # a huge finite reference (-1e30 on every key so far): (x - m) * c
                s = s - torch.where(far, m, torch.zeros_like(m))[..., None]
                mc = torch.where(far, torch.zeros_like(mc), mc)
            e = torch.exp2(_fma(s, c, -mc[..., None]))
        if t > 0 and bool(W[:, :, :nq].any()):
            rescales += 1
        o, l = o * alpha[..., None], l * alpha
        p = rd(e)
        p_max = max(p_max, float(p[:, :, :nq].nan_to_num(0.0).max()))
        l = l + (p if ones else e).sum(-1)
        o = o + p @ V[:, :, :, j0:j1].transpose(2, 3)
    o = o * (1.0 / l)[..., None]
    if B > 0 and a.get("w1_dev") is not None and L1 > 0:
        n = 1 if fault == "w1_dev0" else gc.attention_w1_count(a)
        w1 = _rd(a["w1_dev"], 0, (n,), (1,)).to(f32).expand(B) if n == 1 else _rd(a["w1_dev"], 0, (n,), (1,)).to(f32)
    else:
        w1 = torch.full((B,), float(np.float32(a["w1"])), dtype=f32, device=dev)
    w1 = w1.reshape(B, 1, 1)
    if fault == "w1_on_seg0":
        o = o * w1[..., None]
    # segment 1: one tile, its own softmax
    if L1 > 0:
        K1, V1 = rows("k1", L1, a["k1_ld"], a["k1_bs"]), cols("vt1", L1, a["vt1_ld"], a["vt1_bs"])
        s = qf @ K1.transpose(2, 3)
        if fold and fault == "fold_ref_not_reset":
            s = s + qbias[..., None]
        if fault == "mask_on_seg1" and masked:
            s = s + M[..., :L1]
        sc1 = 1.0 if fold else c
        mc1 = s.amax(-1) * sc1
        e = torch.exp2(_fma(s, sc1, -mc1[..., None]))
        l1 = l if fault == "seg1_l0" else e.sum(-1)
        p = rd(e * (w1 / l1)[..., None])
        o = o + p @ V1.transpose(2, 3)
    if info is not None:
        info.update(rescales=rescales, p_max=p_max)
    out = rd(o[:, :, :nq])                                                       # [B, H, nq, D]
    return out.permute(0, 2, 1, 3).reshape(B, nq, H * D).to(torch.float64)


# ---- the comparison ------------------------------------------------------------------------------------------------------------------
def block_ranges(n_q):
    """[(row0, row1)] of the 128-query blocks; a ragged last block under ``MERGE_BELOW`` rows joins the one before it"""
    r = [(i, min(i + BLOCK, n_q)) for i in range(0, n_q, BLOCK)]
    if len(r) > 1 and r[-1][1] - r[-1][0] < MERGE_BELOW:
        r[-2:] = [(r[-2][0], r[-1][1])]
    return r


def block_rel_l2(got, ref, heads):
    """fp64 [batch, heads, blocks]: ||got - ref|| / ||ref|| over each (batch item, head, 128-query block) x the head's columns.  A block whose
    reference is under a tenth of the tensor's rms per element is measured against that floor."""
    g, r = got.detach().to(torch.float64), ref.detach().to(torch.float64).to(got.device)
    assert g.shape == r.shape, f"{tuple(g.shape)} vs {tuple(r.shape)}"
    B, n, inner = r.shape
    d4, r4 = (g - r).reshape(B, n, heads, -1), r.reshape(B, n, heads, -1)
    rms2 = (0.1 * float(r.norm()) / math.sqrt(max(r.numel(), 1))) ** 2
    out = []
    for r0, r1 in block_ranges(n):
        dd, rr = (d4[:, r0:r1] ** 2).sum(dim=(1, 3)), (r4[:, r0:r1] ** 2).sum(dim=(1, 3))
        out.append(torch.sqrt(dd / rr.clamp_min(rms2 * (r1 - r0) * r4.shape[3]).clamp_min(1e-300)))
    return torch.stack(out, dim=-1)


def compare(got, ref, heads):
    """metrics of an output against the fp64 reference: ``rel_l2`` / ``max_rel`` of the whole tensor, ``block_rel_l2`` of the worst block"""
    g, r = got.detach().to(torch.float64), ref.detach().to(torch.float64).to(got.device)
    d = g - r
    blk = block_rel_l2(g, r, heads)
    return {"rel_l2": float(d.norm()) / max(float(r.norm()), 1e-30), "max_rel": float(d.abs().max()) / max(float(r.abs().max()), 1e-30),
            "block_rel_l2": float(blk.max()), "block_at": [int(i) for i in torch.unravel_index(torch.argmax(blk), blk.shape)],
            "finite": bool(torch.isfinite(g).all())}


def bounds(model_metrics):
    """the norm rule: (whole-tensor rel-L2, worst block, max-rel) a storage-dtype output is held to, from the model's own figures"""
    return 1.5 * model_metrics["rel_l2"], 1.5 * model_metrics["block_rel_l2"], 2.0 * model_metrics["max_rel"]


def within(m, bound):
    return m["finite"] and m["rel_l2"] <= bound[0] and m["block_rel_l2"] <= bound[1] and m["max_rel"] <= bound[2]


# ---- tg_attn_probs -------------------------------------------------------------------------------------------------------------------
def probs_case(dtype, batch, b0, heads, d, n_q, length, *, tokens=None, device="cpu", seed=0, pitched=True):
    """the arguments of ``tg_attn_probs`` as a dict: N(0, 1) q / k, pitched rows with NaN pads and gap rows (``pitched``), NaN-filled probs"""
    inner = heads * d
    g = torch.Generator().manual_seed(9000 + seed + 7 * length + n_q + d)
    q = torch.randn((batch, n_q, inner), generator=g).to(dtype)
    k = torch.randn((batch, length, inner), generator=g).to(dtype)
    pad, gap = (8, 1) if pitched else (0, 0)
    a = dict(batch=batch, b0=b0, heads=heads, head_dim=d, n_q=n_q, len=length, scale=float(d ** -0.5), q_ld=inner + pad, k_ld=inner + 2 * pad)
    a["q"], a["q_bs"] = _pitched_rows(q, batch, n_q, inner, a["q_ld"], gap, dtype, device)
    a["k"], a["k_bs"] = _pitched_rows(k, batch, length, inner, a["k_ld"], gap, dtype, device)
    a["tokens"] = None if tokens is None else torch.tensor(tokens, dtype=torch.int32, device=device)
    a["n_tokens"] = 0 if tokens is None else len(tokens)
    shape = (batch - b0, heads, n_q, length if tokens is None else len(tokens))
    store = torch.full((math.prod(shape) + 32,), NAN, dtype=torch.float32, device=device)              # 16 guard floats on either side
    a["probs"] = store[16:-16].view(shape)
    return a


def probs_read_extents(a):
    n, inner = a["batch"] - a["b0"], a["heads"] * a["head_dim"]
    regs = [Region("q", a["q"], a["b0"] * a["q_bs"], (n, a["n_q"], inner), (a["q_bs"], a["q_ld"], 1)),
            Region("k", a["k"], a["b0"] * a["k_bs"], (n, a["len"], inner), (a["k_bs"], a["k_ld"], 1))]
    if a["tokens"] is not None:
        regs.append(Region("tokens", a["tokens"], 0, (a["n_tokens"],), (1,)))
    return regs


def probs_written_region(a):
    return [Region("probs", a["probs"], 0, (a["probs"].numel(),), (1,))]


def _probs_operands(a, work):
    n, H, D = a["batch"] - a["b0"], a["heads"], a["head_dim"]
    q, k = (r.view().to(work) for r in probs_read_extents(a)[:2])
    return q.reshape(n, a["n_q"], H, D).transpose(1, 2), k.reshape(n, a["len"], H, D).transpose(1, 2)       # [n, H, rows, D]


def _gather(p, a):
    return p if a["tokens"] is None else p[..., a["tokens"].long()]


def probs_reference(a):
    """fp64 [batch - b0, heads, n_q, len or n_tokens]: softmax rows of items b0 .. batch - 1, gathered at ``tokens`` when given"""
    q, k = _probs_operands(a, torch.float64)
    return _gather(torch.softmax(float(np.float32(a["scale"])) * (q @ k.transpose(2, 3)), dim=-1), a)


def probs_model(a):
    """the same in fp32 arithmetic: fp32 dot, x scale, - max, exp, sum, x (1 / sum)"""
    q, k = _probs_operands(a, torch.float32)
    s = (q @ k.transpose(2, 3)) * float(np.float32(a["scale"]))
    e = torch.exp(s - s.amax(-1, keepdim=True))
    return _gather(e * (1.0 / e.sum(-1, keepdim=True)), a).to(torch.float64)


def probs_bound(a):
    """fp64, the shape of ``probs_reference``: the element-by-element bound of the module docstring"""
    u = 2.0 ** -24
    q, k = _probs_operands(a, torch.float64)
    sc = float(np.float32(a["scale"]))
    s = sc * (q @ k.transpose(2, 3))
    A = abs(sc) * (q.abs() @ k.abs().transpose(2, 3))
    x = (s - s.amax(-1, keepdim=True)).abs()
    p = torch.softmax(s, dim=-1)
    dj = u * ((a["head_dim"] + 1) * (A + A.amax(-1, keepdim=True)) + 2 * x + 2)
    return _gather(p * (dj + (p * dj).sum(-1, keepdim=True) + 12 * u) + 2.0 ** -126, a)


# ---- the cases of tests/test_attn_fwd_contract_cpu.py and tests/test_attn_fwd_edges_gpu.py ------------------------------------------------
HEAD_DIMS = (8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 88, 96, 104, 128, 136, 160)
LEN0S, LEN1S, NQS = (1, 7, 8, 9, 63, 64, 65, 72, 127, 128, 129, 200), (0, 1, 4, 8, 16, 63, 64), (1, 31, 32, 33, 127, 128, 129, 257)
MASK_LAYOUTS = [dict(bs=b, hs=h, qs=q) for b in (False, True) for h in (False, True) for q in (False, True)] + [dict(bs=True, hs=True, qs=True, pitch=11)]
FOLD_QMULS = (1.0, 2.0, 4.0, 8.0)
PS_W1 = (0.4, -0.7)


def _case(kind="normal", fn=make_case, **kw):
    return dict(kind=kind, fn=fn, kw=kw)


def _all_cases():
    """name -> dict(kind, fn, kw).  kind "normal": scores are N(0, 1)-scaled, the absolute figure of the suite applies on top of the model's
    bound; "peaked": judged against the model alone.  Batch 2, heads 2 throughout."""
    C = {}
    two = dict(B=2, heads=2)
    for d in HEAD_DIMS:                                                                     # every instance, head_dim < DPAD included
        for mk in (None, "rand"):
            C[f"inst d{d} {'mask' if mk else 'nomask'}"] = _case(**two, n_q=136, len0=141, d=d, len1=4, mask=mk)
    for d in (40, 64):
        for n in LEN0S:
            C[f"len0 {n} d{d}"] = _case(**two, n_q=40, len0=n, d=d)
        for n in LEN1S:
            C[f"len1 {n} d{d}"] = _case(**two, n_q=40, len0=77, d=d, len1=n)
        for n in NQS:
            C[f"nq {n} d{d}"] = _case(**two, n_q=n, len0=77, d=d, len1=4)
        C[f"causal 77 d{d}"] = _case(**two, n_q=77, len0=77, d=d, causal=True)
        C[f"causal 200 d{d}"] = _case(**two, n_q=200, len0=200, d=d, causal=True)
        C[f"causal nq150 len70 d{d}"] = _case(**two, n_q=150, len0=70, d=d, causal=True)
        C[f"causal nq70 len192 d{d}"] = _case(**two, n_q=70, len0=192, d=d, causal=True)
        C[f"causal 77 len1 4 d{d}"] = _case(**two, n_q=77, len0=77, d=d, len1=4, causal=True)
        C[f"causal 136 mask d{d}"] = _case(**two, n_q=136, len0=136, d=d, causal=True, mask="rand")
        for i, lay in enumerate(MASK_LAYOUTS):
            C[f"mask layout {i} d{d}"] = _case(**two, n_q=136, len0=77, d=d, mask="rand", mask_layout=lay)
        for mk in ("zero", "m1e4", "big_some", "big_row", "inf_part", "inf_tile0"):
            C[f"mask {mk} d{d}"] = _case(**two, n_q=136, len0=141, d=d, mask=mk)
        C[f"mask fmin d{d}"] = _case(**two, n_q=136, len0=141, d=d, mask="fmin", scale=0.125)
        for q in FOLD_QMULS:                                                                # FOLD against the zero-mask instance (d 40); d 64 for scale
            C[f"qx{q:g} d{d} nomask"] = _case("normal" if q == 1.0 else "peaked", **two, n_q=129, len0=141, d=d, qmul=q)
            C[f"qx{q:g} d{d} zeromask"] = _case("normal" if q == 1.0 else "peaked", **two, n_q=129, len0=141, d=d, qmul=q, mask="zero")
    # softmax range, one case per instance class
    for cls, d, mk in (("fold", 40, None), ("ones", 80, None), ("plain", 64, None), ("mask", 64, "zero")):
        sp = dict(fn=spike_case, **two, n_q=40, len0=141, d=d, mask=mk)
        C[f"range {cls} late +7.5"] = _case("peaked", spike_key=130, log2_above=7.5, **sp)
        C[f"range {cls} late +8.5"] = _case("peaked", spike_key=130, log2_above=8.5, **sp)
        C[f"range {cls} late +200"] = _case("peaked", spike_key=130, log2_above=200.0, **sp)
        C[f"range {cls} tile0 +200"] = _case("peaked", spike_key=5, log2_above=200.0, **sp)
        C[f"range {cls} x8"] = _case("peaked", **two, n_q=136, len0=141, d=d, len1=4, qmul=8.0, mask=mk)
    C["range fold reference 2^12"] = _case("peaked", fn=spike_case, **two, n_q=40, len0=141, d=40, len1=4, spike_key=5, log2_above=2.0 ** 12)
    # tg_attention_ps
    for d in (40, 64, 80, 160):
        for cnt, w in ((0, [0.4]), (1, [-0.7]), (2, list(PS_W1))):
            C[f"ps count {cnt} d{d}"] = _case(**two, n_q=40, len0=77, d=d, len1=4, w1=9.0, w1_dev=w, ip_scale_count=cnt)
    C["ps w1 zero and negative d64"] = _case(**two, n_q=40, len0=77, d=64, len1=4, w1=9.0, w1_dev=[0.0, -1.3], ip_scale_count=2)
    return C


CASES = _all_cases()


def build(name, dtype, device="cpu"):
    c = CASES[name]
    return c["fn"](dtype, device=device, **c["kw"])
