"""fp64 restatements of the contracts of ``tg_dino_contrastive`` and ``tg_dino_box_update`` (include/theatergen_hip.h), their case lists and the error
bounds the GPU tests hold the kernels to.  Every bound is derived here from operation counts and the number formats, none is a measured figure.

u = 2^-24 is the unit roundoff of fp32 (round to nearest).

CONTRASTIVE.  A logit is a sum of d products accumulated in fp32 by the matrix cores.  The products are exact in fp32 (bf16 x bf16 has 16 significant
bits, fp16 x fp16 has 22).  A sum of d terms accumulated in ANY order with roundoff v per addition is within ((1 + v)^(d - 1) - 1) sum|q_i t_i| <=
d v sum|q_i t_i| of the exact sum for d v << 1.  The matrix pipe's internal order and rounding of the four-way partial sums are not documented; the bound
takes v = 2 u, which also covers an accumulator that truncates instead of rounding to nearest:

    |logit - exact| <= CONTRASTIVE_C * d * 2^-24 * sum_i |q_i t_i|,     CONTRASTIVE_C = 2.

BOX UPDATE.  t = (dot + b3) + lg, ref = 1 / (1 + exp(-t)).
  dot   d / 64 FMAs per lane and a 6-step butterfly: at most d / 64 + 6 <= d roundings on any path: |dot - exact| <= d u sum|h_i w_i|.
  adds  two roundings: <= u (|dot + b3| + |t|) <= 2 u (|dot| + |b3| + |lg|).
  lg    (prior_is_box) c = clamp(x) exact; 1 - c one rounding, the quotient one: a relative input error <= 2 u is an ABSOLUTE error <= 2 u of the
        logarithm (d log y = dy / y), plus logf's own error LIBM_ULP u |lg|.  LIBM_ULP = 2 is the accuracy the device library documents for its precise
        logf / expf / sinf / cosf / powf (<= 2 ulp).
  The sigmoid's slope is at most 1 / 4, so the terms above enter ref divided by 4 (second order: t's error is < 1e-4 here).  exp, the addition and the
  division add LIBM_ULP + 2 roundings relative to the result:

    |ref - exact| <= (d u sum|h_i w_i| + 2 u (|dot| + |b3| + |lg|) + 2 u + LIBM_ULP u |lg|) / 4 + (LIBM_ULP + 2) u ref.

  ref_levels = ref * vr is one more rounding: bound(ref) vr + u |ref vr|.
  pos_in     the argument a = 2 pi c / 10000^(4 m / d), c = ref vr of level 0, |a| <= 2 pi.  Its error is the error of c scaled by 2 pi / dim plus ARG_ROUNDINGS
             = 8 relative roundings (powf's LIBM_ULP, the quotient, the reduction's subtraction is exact, the product with 2 pi and its constant, and
             the exponent 4 m / d whose relative error powf magnifies by ln(10000) 4 m / d <= 9.3 -> counted as 2 more): |da| <= 2 pi / dim * dc + 8 u |a|.
             sin and cos have slope <= 1 ("the fp32 argument error times 1"), their own error is LIBM_ULP u, and the result is rounded ONCE to the
             storage dtype: half an ulp, relative 2^-(m + 1) with m = 7 (bf16) / 10 (fp16) explicit mantissa bits, and for fp16 never less
             than half the subnormal spacing, 2^-25:

    |pos_in - exact| <= (|da| + LIBM_ULP u) (1 + 2^-(m + 1)) + 2^-(m + 1) |exact| + subnormal term.
"""
import numpy as np

U = 2.0 ** -24
CONTRASTIVE_C = 2.0
LIBM_ULP = 2.0
ARG_ROUNDINGS = 8.0
EPS = 1e-5

# (n, Lt, max_text_len, d, q pitch, text pitch, batch, mask): mask "all" = every token real, "pad" = a real prefix per item (different per item),
# "holes" = a random pattern, "none1" = item 1 has no real token.  Every n in {1, 63, 64, 65, 130}, every Lt in {1, 8, 9, 33, 256}, both d,
# max_text_len == Lt and > Lt (multiples of 4 and not: both store paths), pitches wider than d, batch 2.
CONTRASTIVE_CASES = [
    (1, 1, 1, 128, 128, 128, 1, "all"),
    (63, 8, 8, 128, 136, 128, 2, "pad"),
    (64, 9, 16, 256, 256, 264, 2, "holes"),
    (65, 33, 35, 128, 128, 144, 2, "none1"),
    (130, 256, 256, 256, 272, 256, 2, "pad"),
    (65, 9, 256, 256, 256, 256, 1, "holes"),
    (130, 33, 64, 128, 128, 128, 2, "none1"),
    (64, 1, 5, 256, 264, 264, 2, "all"),
]
CONTRASTIVE_IDS = ["n%d-Lt%d-T%d-d%d-%d-%d-b%d-%s" % c for c in CONTRASTIVE_CASES]

# (rows, batch, L, d, h pitch, prior mode): "logit" = prior used as it is (some +inf), "box" = logit taken in the kernel; the box priors of every case
# contain 0, 1, 1e-7, 0.5 and 1 - 1e-7 (the eps clamp).  rows in {1, 7, 64, 901}, L in {1, 4}, valid ratios < 1.
BOX_CASES = [
    (1, 1, 1, 128, 128, "box"),
    (7, 1, 4, 256, 256, "logit"),
    (64, 2, 4, 128, 136, "box"),
    (901, 1, 4, 256, 264, "box"),
    (901, 1, 1, 128, 128, "logit"),
    (64, 2, 1, 256, 256, "logit"),
]
BOX_IDS = ["r%d-b%d-L%d-d%d-%d-%s" % c for c in BOX_CASES]


def storage_round(a, dtype):
    """fp64 / fp32 array -> the values a torch tensor of ``dtype`` holds, as float32"""
    import torch
    return torch.from_numpy(np.asarray(a, np.float32)).to(dtype).float().numpy()


def make_contrastive_case(case, dtype, seed):
    n, Lt, mtl, d, _, _, B, mode = case
    rs = np.random.RandomState(seed)
    q = storage_round(rs.standard_normal((B, n, d)), dtype)
    text = storage_round(rs.standard_normal((B, Lt, d)), dtype)
    if mode == "all":
        mask = np.ones((B, Lt), np.uint8)
    elif mode == "pad":
        mask = np.stack([(np.arange(Lt) < max(1, Lt - 1 - 3 * b)) for b in range(B)]).astype(np.uint8)
    else:
        mask = (rs.rand(B, Lt) < 0.6).astype(np.uint8)
        mask[0, 0] = 1
        if mode == "none1":
            mask[1] = 0
    return q, text, mask


def contrastive_reference(q, text, mask, max_text_len):
    """-> (logits fp64 [B, n, max_text_len] with -inf, row_max fp64 [B, n], bound fp64 [B, n, max_text_len] (0 where -inf))"""
    q, text = np.asarray(q, np.float64), np.asarray(text, np.float64)
    B, n, d = q.shape
    Lt = text.shape[1]
    real = np.asarray(mask).astype(bool)
    out = np.full((B, n, max_text_len), -np.inf)
    bound = np.zeros((B, n, max_text_len))
    dots = np.einsum("bnd,btd->bnt", q, text)
    mags = np.einsum("bnd,btd->bnt", np.abs(q), np.abs(text))
    keep = np.broadcast_to(real[:, None, :], dots.shape)
    out[:, :, :Lt] = np.where(keep, dots, -np.inf)
    bound[:, :, :Lt] = np.where(keep, CONTRASTIVE_C * d * U * mags, 0.0)
    return out, out.max(-1), bound


def make_box_case(case, dtype, seed):
    rows, B, L, d, _, mode = case
    rs = np.random.RandomState(seed)
    h = storage_round(np.maximum(rs.standard_normal((rows, d)), 0), dtype)                  # after ReLU
    w3 = storage_round(0.1 * rs.standard_normal((4, d)), dtype)
    b3 = (0.2 * rs.standard_normal(4)).astype(np.float32)
    if mode == "box":
        prior = rs.uniform(0.02, 0.98, (rows, 4)).astype(np.float32)
        special = np.array([0.0, 1.0, 1e-7, 0.5, 1.0 - 1e-7], np.float32)
        flat = prior.reshape(-1)
        flat[:min(flat.size, 5)] = special[:min(flat.size, 5)]
        if flat.size > 16:
            flat[-5:] = special
    else:
        prior = (3.0 * rs.standard_normal((rows, 4))).astype(np.float32)
        prior[::3, 0] = np.inf
        if rows > 1:
            prior[1] = np.inf
    vr = rs.uniform(0.55, 0.98, (B, L, 2)).astype(np.float32)
    return h, w3, b3, prior, vr


def logit_eps(x, eps_dtype=np.float32):
    """torch.special.logit(x, eps = 1e-5); ``eps_dtype``: the format in which eps and 1 - eps are formed (the kernel and fp32 torch: float32)"""
    lo = eps_dtype(EPS)
    hi = eps_dtype(1) - lo
    c = np.clip(np.asarray(x, np.float64), np.float64(lo), np.float64(hi))
    return np.log(c / (1.0 - c))


def sinusoidal(c4, d):
    """encode_sinusoidal_position_embedding(c4 [rows, 4], num_pos_feats = d / 2) in fp64 -> (values [rows, 2 d], arguments, 2 pi / dim_t per channel)"""
    npf = d // 2
    j = np.arange(npf)
    dim_t = 10000.0 ** (2 * (j // 2) / npf)
    vals, args, slopes = [], [], []
    for k in (1, 0, 2, 3):                                                                  # (y, x, w, h)
        a = c4[:, k, None] * (2 * np.pi) / dim_t
        vals.append(np.where(j % 2 == 0, np.sin(a), np.cos(a)))
        args.append(a)
        slopes.append(np.broadcast_to(2 * np.pi / dim_t, a.shape))
    return np.concatenate(vals, 1), np.concatenate(args, 1), np.concatenate(slopes, 1)


def box_update_reference(h, w3, b3, prior, prior_is_box, vr, rows_per_batch, mant_bits, eps_dtype=np.float32):
    """-> dict of (value, bound) for "ref" [rows, 4], "ref_levels" [rows, L, 4] and "pos_in" [rows, 2 d]; ``mant_bits``: explicit mantissa bits of the
    storage dtype (7 for bf16, 10 for fp16)"""
    h, w3, b3 = np.asarray(h, np.float64), np.asarray(w3, np.float64), np.asarray(b3, np.float64)
    prior = np.asarray(prior, np.float64)
    rows, d = h.shape
    dot = h @ w3.T
    mag = np.abs(h) @ np.abs(w3).T
    lg = logit_eps(prior, eps_dtype) if prior_is_box else prior
    with np.errstate(over="ignore"):
        ref = 1.0 / (1.0 + np.exp(-(dot + b3 + lg)))
    fin = np.where(np.isfinite(lg), np.abs(lg), 0.0)
    b_ref = (d * U * mag + 2 * U * (np.abs(dot) + np.abs(b3) + fin) + (2 * U + LIBM_ULP * U * fin if prior_is_box else 0.0)) / 4 + (LIBM_ULP + 2) * U * ref
    b_ref = np.where(np.isposinf(lg), 0.0, b_ref)                                           # +inf: exactly 1
    vr = np.asarray(vr, np.float64)
    v4 = np.concatenate([vr, vr], -1)[np.arange(rows) // rows_per_batch]                    # [rows, L, 4]
    lev = ref[:, None, :] * v4
    b_lev = b_ref[:, None, :] * v4 + U * np.abs(lev)
    val, arg, slope = sinusoidal(lev[:, 0], d)
    order = (1, 0, 2, 3)
    dc = np.concatenate([np.broadcast_to(b_lev[:, 0, k, None], (rows, d // 2)) for k in order], 1)
    half = 2.0 ** -(mant_bits + 1)                                                          # half an ulp, relative to the binade's lower end
    sub = 2.0 ** -25 if mant_bits == 10 else 0.0
    b_pos = (slope * dc + ARG_ROUNDINGS * U * np.abs(arg) + LIBM_ULP * U) * (1 + half) + half * np.abs(val) + sub
    return {"ref": (ref, b_ref), "ref_levels": (lev, b_lev), "pos_in": (val, b_pos)}
