"""The C-ABI contracts of the five reverse-pass Jacobian entries of csrc/tg_backward.hip (include/theatergen_hip.h: ``tg_groupnorm_bwd``,
``tg_layernorm_bwd``, ``tg_geglu_bwd``, ``tg_softmax_bwd_rows``, ``tg_sumpool2x2``) restated in fp64, for checking single launches.

A launch is a plain dict: ``entry`` plus the C argument names; tensors stand for the pointers (a tensor's ``data_ptr`` is the pointer).  Operands
are read the way the kernels read raw pointers, ``gemm_contract.Region`` over the operand's storage along the pitches of the call, never the
tensor's logical shape; a launch that reads past a storage makes ``Region.view`` raise.

    groupnorm  xhat = (x - mean) rstd over one (item, group), z = gamma xhat + beta, gy = gamma dy act'(z)
               dx = rstd (gy - mean(gy) - xhat mean(gy xhat))                                   act' = SiLU' (silu) or 1
    layernorm  the same over one row, gy = gamma dy (gamma NULL: 1)
    geglu      h = [a | gate], cdf = (1 + erf(gate / sqrt 2)) / 2, pdf = exp(-gate^2 / 2) / sqrt(2 pi)
               dh = [dg gate cdf | dg a (cdf + gate pdf)]
    softmax    dS = scale P (dP + extra - sum_j P_j (dP_j + extra_j)) in columns < length, 0 in columns [length, ld_out); P copied likewise
    sumpool    out[b, y, x, c] = sum of the 2 x 2 block of du[b, 2y.., 2x.., c]

  * ``reference(a)`` -> {output name: fp64 tensor shaped like the output's written region}; ``magnitude=True``: the same sums over absolute
        values, the scale a reference that cancels to zero is measured against (softmax at length 1, layernorm at C = 1, sumpool2x2)
  * ``read_extents(a)`` / ``written_region(a)``: ``Region`` lists; the written region of ``tg_groupnorm_bwd`` includes the scratch
  * ``gnb_slabs`` / ``gn_fallback_reasons`` / ``gn_path``: the slab count and the kernel choice of tg_groupnorm_bwd restated
  * ``blocks(a)``: the unit one workgroup (or wave) owns: (item, slab, group) on the slab path, (item, group) on the fallback, a row for
        layernorm, softmax and geglu, a pixel for sumpool2x2; ``compare``: whole-tensor rel-L2 and max|err| / max|ref| plus the worst block
  * ``model(a, fault=None)``: fp32 models of the kernels (slab GroupNorm with the one-pass variance and the kernel's summation order inside
        a slab, the centred fallback, LayerNorm, GEGLU, softmax, pool), with switches that inject one fault each
  * ``judge(a, outputs)``: every assertion the GPU edge tests make on the outputs of one launch, as a list of failures
  * ``make_case(entry, dtype, ...)`` and ``CASES``: the launches of tests/test_backward_edges_gpu.py, drawn on the CPU from a seed; every
        element of an input buffer the contract does not read (pad columns, guard rows) holds NaN.
"""
import itertools
import math

import torch

from tests import launch_check as lc
from tests.attn_bwd_contract import CANCEL
from tests.gemm_contract import Region

GNB_MAX_SLOTS = 2
GRID_CAP_ELEMS = 4096 * 256                                        # grid_of: 4096 workgroups of 256 threads, then the grid-stride trip
EPS = 1e-5


def tols(dtype):
    """1.5 x the per-launch bound of launch_check (the attention edge tests' bound): rel-L2 4.5e-3 / 6e-4, max 1.5e-2 / 3.75e-3"""
    return 1.5 * lc.l2_tol(dtype), 1.5 * lc.rel_tol(dtype)


def unit_roundoff(dtype):
    """largest relative error of one rounding to ``dtype``: 2^-8 (bf16), 2^-11 (fp16)"""
    return torch.finfo(dtype).eps / 2


def _f32(v):
    return float(torch.tensor(float(v), dtype=torch.float32))


# ---- tg_groupnorm_bwd: slab count and kernel choice ------------------------------------------------------------------------------------
def gnb_slabs(batch, hw):
    s = (hw + 31) // 32
    cap = 1 if batch >= 128 else 128 // batch
    s = min(s, cap)
    return max(s, 1)


def gn_scratch_floats(batch, hw, groups):
    return batch * gnb_slabs(batch, hw) * groups * 4


def gn_fallback_reasons(a):
    """why a tg_groupnorm_bwd call runs the one-workgroup-per-(item, group) kernel; empty: the slab kernels run"""
    r = []
    if a.get("partials") is None:
        r.append("partials is NULL")
    if a["C"] % 8:
        r.append("channels not a multiple of 8")
    if a["C"] > 8 * 256 * GNB_MAX_SLOTS:
        r.append("channels > 4096")
    if a["groups"] > 256:
        r.append("groups > 256")
    if any(a[n].data_ptr() % 16 for n in ("x", "dy", "dx", "gamma", "beta")):
        r.append("a pointer is not 16-byte aligned")
    return r


def gn_path(a):
    return "fallback" if gn_fallback_reasons(a) else "slab"


def gn_slab_geometry(a):
    """(nslab, rows per slab, TC, TR) of the slab kernels"""
    nslab = gnb_slabs(a["batch"], a["hw"])
    nch = a["C"] // 8
    TC = min(nch, 256)
    return nslab, (a["hw"] + nslab - 1) // nslab, TC, 256 // TC


# ---- regions -------------------------------------------------------------------------------------------------------------------------
def _reg(name, t, sizes, strides):
    return Region(name, t, 0, tuple(int(s) for s in sizes), tuple(int(s) for s in strides))


def _gn_regs(a, names):
    B, hw, Cc = a["batch"], a["hw"], a["C"]
    return [_reg(n, a[n], (B, hw, Cc), (hw * Cc, Cc, 1)) for n in names]


def _sm_reg(a, name, ld, cols):
    return _reg(name, a[name], (a["rows"], cols), (ld, 1))


def read_extents(a):
    e = a["entry"]
    if e == "groupnorm":
        return _gn_regs(a, ("x", "dy")) + [_reg(n, a[n], (a["C"],), (1,)) for n in ("gamma", "beta")]
    if e == "layernorm":
        regs = [_reg(n, a[n], (a["rows"], a["C"]), (a["C"], 1)) for n in ("x", "dy")]
        return regs + ([_reg("gamma", a["gamma"], (a["C"],), (1,))] if a.get("gamma") is not None else [])
    if e == "geglu":
        return [_reg("h", a["h"], (a["rows"], 2 * a["inner"]), (2 * a["inner"], 1)), _reg("dg", a["dg"], (a["rows"], a["inner"]), (a["inner"], 1))]
    if e == "softmax":
        regs = [_sm_reg(a, "probs", a["ld_probs"], a["length"]), _sm_reg(a, "dprobs", a["ld_dprobs"], a["length"])]
        return regs + ([_sm_reg(a, "extra", a["ld_extra"], a["length"])] if a.get("extra") is not None else [])
    assert e == "sumpool", e
    B, h, w, Cc = a["batch"], a["h"], a["w"], a["C"]
    return [_reg("du", a["du"], (B, 2 * h, 2 * w, Cc), (4 * h * w * Cc, 2 * w * Cc, Cc, 1))]


def written_region(a):
    e = a["entry"]
    if e == "groupnorm":
        regs = _gn_regs(a, ("dx",))
        if gn_path(a) == "slab":
            B, S, G = a["batch"], gnb_slabs(a["batch"], a["hw"]), a["groups"]
            regs.append(_reg("partials", a["partials"], (B, S, G, 4), (S * G * 4, G * 4, 4, 1)))
        return regs
    if e == "layernorm":
        return [_reg("dx", a["dx"], (a["rows"], a["C"]), (a["C"], 1))]
    if e == "geglu":
        return [_reg("dh", a["dh"], (a["rows"], 2 * a["inner"]), (2 * a["inner"], 1))]
    if e == "softmax":
        regs = [_sm_reg(a, "dscores", a["ld_out"], a["ld_out"])]
        return regs + ([_sm_reg(a, "probs_out", a["ld_out"], a["ld_out"])] if a.get("probs_out") is not None else [])
    assert e == "sumpool", e
    B, h, w, Cc = a["batch"], a["h"], a["w"], a["C"]
    return [_reg("out", a["out"], (B, h, w, Cc), (h * w * Cc, w * Cc, Cc, 1))]


def _ext(a):
    return {r.name: r.view() for r in read_extents(a)}


def storage_dtype(a):
    return a[{"groupnorm": "x", "layernorm": "x", "geglu": "h", "softmax": "dprobs", "sumpool": "du"}[a["entry"]]].dtype


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def _silu_grad(z):
    s = 1.0 / (1.0 + torch.exp(-z))
    return s * (1.0 + z * (1.0 - s))


def _norm_grad(x, gy_of, dims, eps, magnitude):
    """x [..]: statistics over ``dims``; gy_of(xhat) -> gamma dy act'(gamma xhat + beta)"""
    mean = x.mean(dims, keepdim=True)
    var = ((x - mean) ** 2).mean(dims, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (x - mean) * rstd
    gy = gy_of(xh)
    if magnitude:
        return rstd * (gy.abs() + gy.abs().mean(dims, keepdim=True) + xh.abs() * (gy * xh).abs().mean(dims, keepdim=True))
    return rstd * (gy - gy.mean(dims, keepdim=True) - xh * (gy * xh).mean(dims, keepdim=True))


def gn_group_stats(a):
    """fp64 (mean, rstd) [batch, groups] of a tg_groupnorm_bwd call"""
    B, hw, Cc, G = a["batch"], a["hw"], a["C"], a["groups"]
    x = _ext(a)["x"].double().reshape(B, hw, G, Cc // G)
    mean = x.mean((1, 3))
    var = ((x - mean[:, None, :, None]) ** 2).mean((1, 3))
    return mean, 1.0 / torch.sqrt(var + _f32(a["eps"]))


def reference(a, magnitude=False):
    e, ext = a["entry"], _ext(a)
    if e == "groupnorm":
        B, hw, Cc, G = a["batch"], a["hw"], a["C"], a["groups"]
        sh = (B, hw, G, Cc // G)
        ga, be = (ext[n].double().reshape(1, 1, G, Cc // G) for n in ("gamma", "beta"))
        dy = ext["dy"].double().reshape(sh)

        def gy_of(xh):
            return ga * dy * (_silu_grad(ga * xh + be) if a["silu"] else 1.0)
        return {"dx": _norm_grad(ext["x"].double().reshape(sh), gy_of, (1, 3), _f32(a["eps"]), magnitude).reshape(B, hw, Cc)}
    if e == "layernorm":
        ga = ext["gamma"].double() if "gamma" in ext else 1.0
        dy = ext["dy"].double()
        return {"dx": _norm_grad(ext["x"].double(), lambda xh: ga * dy, (1,), _f32(a["eps"]), magnitude)}
    if e == "geglu":
        inner = a["inner"]
        h, d = ext["h"].double(), ext["dg"].double()
        av, gt = h[:, :inner], h[:, inner:]
        cdf = 0.5 * (1.0 + torch.erf(gt / math.sqrt(2.0)))
        pdf = torch.exp(-0.5 * gt * gt) / math.sqrt(2.0 * math.pi)
        if magnitude:
            return {"dh": torch.cat([(d * gt).abs() * cdf, (d * av).abs() * (cdf + gt.abs() * pdf)], dim=1)}
        return {"dh": torch.cat([d * gt * cdf, d * av * (cdf + gt * pdf)], dim=1)}
    if e == "softmax":
        rows, L, ldo = a["rows"], a["length"], a["ld_out"]
        P = ext["probs"].double()
        dP = ext["dprobs"].double() + (ext["extra"].double() if "extra" in ext else 0.0)
        s = (P * dP).sum(-1, keepdim=True)
        sc = _f32(a["scale"])
        out = {"dscores": torch.zeros((rows, ldo), dtype=torch.float64, device=P.device)}
        out["dscores"][:, :L] = abs(sc) * P * (dP.abs() + (P * dP.abs()).sum(-1, keepdim=True)) if magnitude else sc * P * (dP - s)
        if a.get("probs_out") is not None:
            out["probs_out"] = torch.zeros_like(out["dscores"])
            out["probs_out"][:, :L] = P
        return out
    assert e == "sumpool", e
    B, h, w, Cc = a["batch"], a["h"], a["w"], a["C"]
    du = ext["du"].double().reshape(B, h, 2, w, 2, Cc)
    return {"out": (du.abs() if magnitude else du).sum((2, 4))}


# ---- ownership -----------------------------------------------------------------------------------------------------------------------
def blocks(a):
    """-> (ids, grid): ``ids`` an int64 tensor shaped like the entry's main output with the index of the block that owns each element,
    ``grid`` the shape those indices unravel to"""
    e = a["entry"]
    dev = a[written_region(a)[0].name].device

    def ar(n):
        return torch.arange(n, device=dev)
    if e == "groupnorm":
        B, hw, Cc, G = a["batch"], a["hw"], a["C"], a["groups"]
        g = (ar(Cc) // (Cc // G)).reshape(1, 1, Cc)
        b = ar(B).reshape(B, 1, 1)
        if gn_path(a) == "slab":
            S, rows_per, _, _ = gn_slab_geometry(a)
            slab = (ar(hw) // rows_per).reshape(1, hw, 1)
            return (b * S + slab) * G + g, (B, S, G)
        return (b * G + g).expand(B, hw, Cc).contiguous(), (B, G)
    if e == "sumpool":
        B, h, w, Cc = a["batch"], a["h"], a["w"], a["C"]
        return ar(B * h * w).reshape(B, h, w, 1).expand(B, h, w, Cc).contiguous(), (B, h, w)
    rows = a["rows"]
    cols = {"layernorm": a.get("C"), "geglu": 2 * a.get("inner", 0), "softmax": a.get("ld_out")}[e]
    return ar(rows).reshape(rows, 1).expand(rows, cols).contiguous(), (rows,)


def _per_block(v, ids, n, reduce):
    out = torch.zeros(n, dtype=torch.float64, device=v.device)
    if reduce == "sum":
        return out.index_add_(0, ids.reshape(-1), v.reshape(-1))
    return out.scatter_reduce_(0, ids.reshape(-1), v.reshape(-1), "amax", include_self=True)


def compare(got, ref, ids, grid, l2_tol, max_tol, mag=None):
    """-> (ok, metrics): ``rel_l2`` / ``max_rel`` of the whole tensor (parity_metrics' definitions), ``block_rel_l2`` and ``block_max_rel``
    (max|err| of a block over the larger of the block's peak and a tenth of the tensor's) of the worst block with its coordinates
    ``block_at``.  Both tolerances hold for the whole tensor AND for every block.  A block whose reference is under a tenth of the tensor's rms
    per element is measured against that floor.  ``mag`` (the ``magnitude=True`` restatement): norms and peaks of the reference are taken no
    smaller than ``CANCEL`` = 2^-10 of the magnitude restatement's (attn_bwd_contract.compare: fp32 arithmetic leaves a few 2^-24 of the terms
    where the exact result cancels to zero); inert for a reference that does not cancel."""
    g, r = got.detach().to(torch.float64), ref.detach().to(torch.float64).to(got.device)
    assert g.shape == r.shape == ids.shape, f"{tuple(g.shape)} vs {tuple(r.shape)} vs {tuple(ids.shape)}"
    ids = ids.to(g.device)
    n = int(math.prod(grid))
    finite = bool(torch.isfinite(g).all())
    d = torch.nan_to_num(g - r, nan=float("inf"), posinf=float("inf"), neginf=float("inf"))
    peak, norm = float(r.abs().max()), float(r.norm())
    dd, rr = _per_block(d * d, ids, n, "sum"), _per_block(r * r, ids, n, "sum")
    cnt = _per_block(torch.ones_like(r), ids, n, "sum")
    floor = (0.1 * norm / math.sqrt(max(r.numel(), 1))) ** 2 * cnt
    bpeak = _per_block(r.abs(), ids, n, "max")
    if mag is not None:
        m = mag.detach().to(torch.float64).to(g.device)
        peak, norm = max(peak, CANCEL * float(m.abs().max())), max(norm, CANCEL * float(m.norm()))
        floor = torch.maximum(floor, CANCEL ** 2 * _per_block(m * m, ids, n, "sum"))
        bpeak = torch.maximum(bpeak, CANCEL * _per_block(m.abs(), ids, n, "max"))
    peak, norm = max(peak, 1e-30), max(norm, 1e-30)
    blk = torch.sqrt(dd / torch.maximum(rr, floor).clamp_min(1e-300))
    bmax = _per_block(d.abs(), ids, n, "max") / bpeak.clamp_min(0.1 * peak)
    at = [int(i) for i in torch.unravel_index(torch.argmax(blk), tuple(grid))]
    mt = {"rel_l2": float(d.norm()) / norm, "max_rel": float(d.abs().max()) / peak, "block_rel_l2": float(blk.max()), "block_at": at,
          "block_max_rel": float(bmax.max()), "finite": finite}
    ok = finite and max(mt["rel_l2"], mt["block_rel_l2"]) <= l2_tol and max(mt["max_rel"], mt["block_max_rel"]) <= max_tol
    return ok, mt


# ---- per-element bounds --------------------------------------------------------------------------------------------------------------
def _rounding(ref, dtype, n):
    """n roundings of |ref| to ``dtype``: n x unit roundoff x |ref|, no smaller than n halves of the smallest subnormal step"""
    return n * torch.clamp(unit_roundoff(dtype) * ref.abs(), min=torch.finfo(dtype).smallest_normal * torch.finfo(dtype).eps / 2)


def element_bound(a, ref):
    """geglu: 2 half-ulps of the storage dtype at |ref| + 2^-20 |dg| max(1, |a|, |gate|) (the fp32 cancellation of 1 + erf for gates below
    -3); sumpool2x2: one rounding of |ref| + 2^-22 of the sum of the four magnitudes.  None for the other entries."""
    dtype = storage_dtype(a)
    if a["entry"] == "geglu":
        ext, inner = _ext(a), a["inner"]
        h, d = ext["h"].double(), ext["dg"].double().abs()
        fl = 2.0 ** -20 * d * torch.maximum(torch.maximum(h[:, :inner].abs(), h[:, inner:].abs()), torch.ones_like(d))
        return {"dh": _rounding(ref["dh"], dtype, 2) + torch.cat([fl, fl], dim=1)}
    if a["entry"] == "sumpool":
        return {"out": _rounding(ref["out"], dtype, 1) + 2.0 ** -22 * reference(a, magnitude=True)["out"]}
    return None


# ---- fp32 models of the kernels ------------------------------------------------------------------------------------------------------
FAULTS = ("phase0_drops_last_row", "fold_drops_last_slab", "group_of_chunk_head", "no_silu_grad", "no_gamma", "m2_wrong_count",
          "softmax_pads_unwritten", "softmax_sum_without_extra", "grid_stride_tail_dropped", "pool_second_tap_twice")


def _seq_sum(t):
    """fp32 sum over the last dimension, one term after the other"""
    s = torch.zeros(t.shape[:-1], dtype=torch.float32)
    for i in range(t.shape[-1]):
        s = s + t[..., i]
    return s


def _slab_sums(v, a, valid):
    """v fp32 [B, hw, C] -> fp32 [B, nslab, groups]: thread (tr, tc) adds the rows tr, tr + TR, .. of its slab per channel, one thread per
    group then adds the group's channels (channel-major, thread row inside) — gn_bwd_slab_kernel's order.  ``valid`` [hw] bool"""
    B, hw, Cc, G = a["batch"], a["hw"], a["C"], a["groups"]
    S, rows_per, _, TR = gn_slab_geometry(a)
    K = (rows_per + TR - 1) // TR
    v = v * valid.reshape(1, hw, 1)
    v = torch.nn.functional.pad(v, (0, 0, 0, S * rows_per - hw)).reshape(B, S, rows_per, Cc)
    v = torch.nn.functional.pad(v, (0, 0, 0, K * TR - rows_per)).reshape(B, S, K, TR, Cc)
    acc = torch.zeros((B, S, TR, Cc), dtype=torch.float32)
    for k in range(K):
        acc = acc + v[:, :, k]
    return _seq_sum(acc.permute(0, 1, 3, 2).reshape(B, S, G, (Cc // G) * TR))


def _gn_slab_stats(a, fault=None):
    """fp32 (mean, rstd) [B, groups] of the slab path: one-pass variance from fp32 slab sums folded in fp64"""
    B, hw, Cc, G = a["batch"], a["hw"], a["C"], a["groups"]
    S, rows_per, _, _ = gn_slab_geometry(a)
    x = _ext(a)["x"].float().cpu()
    valid = torch.ones(hw, dtype=torch.bool)
    if fault == "phase0_drops_last_row":
        for s in range(S):
            r1 = min((s + 1) * rows_per, hw)
            if r1 > s * rows_per:
                valid[r1 - 1] = False
    nf = S - 1 if fault == "fold_drops_last_slab" else S
    inv_n = 1.0 / (float(hw) * (Cc // G))
    sx, sq = (_slab_sums(t, a, valid)[:, :nf].double().sum(1) for t in (x, x * x))
    mean = sx * inv_n
    var = (sq * inv_n - mean * mean).clamp_min(0.0)
    return mean.float(), (1.0 / torch.sqrt(var + _f32(a["eps"]))).float(), nf, inv_n


def gn_onepass_rstd_error(a):
    """largest relative error over the (item, group)s of the slab path's rstd (fp32 slab sums of x and x^2, E[x^2] - mean^2) against fp64"""
    _, rstd, _, _ = _gn_slab_stats(a)
    _, want = gn_group_stats(a)
    return float(((rstd.double() - want.cpu()) / want.cpu()).abs().max())


def _model_groupnorm(a, fault):
    B, hw, Cc, G = a["batch"], a["hw"], a["C"], a["groups"]
    ext = {k: v.float().cpu() for k, v in _ext(a).items()}
    x, dy, ga, be = ext["x"], ext["dy"], ext["gamma"], ext["beta"]
    cg = Cc // G
    dtype = storage_dtype(a)
    if gn_path(a) == "fallback":
        sh = (B, hw, G, cg)
        xg = x.reshape(sh)
        n = float(hw * cg)
        mean = xg.sum((1, 3), keepdim=True) / n
        rstd = torch.rsqrt(((xg - mean) ** 2).sum((1, 3), keepdim=True) / n + _f32(a["eps"]))
        xh = (xg - mean) * rstd
        gav, bev = ga.reshape(1, 1, G, cg), be.reshape(1, 1, G, cg)
        gy = dy.reshape(sh)
        if a["silu"] and fault != "no_silu_grad":
            gy = gy * _silu_grad(gav * xh + bev)
        if fault != "no_gamma":
            gy = gy * gav
        m1 = gy.sum((1, 3), keepdim=True) / n
        m2 = (gy * xh).sum((1, 3), keepdim=True) / (float(hw) if fault == "m2_wrong_count" else n)
        return {"dx": (rstd * (gy - m1 - xh * m2)).reshape(B, hw, Cc).to(dtype)}
    mean, rstd, nf, inv_n = _gn_slab_stats(a, fault)
    c = torch.arange(Cc)
    gidx = (c // 8 * 8 if fault == "group_of_chunk_head" else c) // cg
    mean_c, rstd_c = mean[:, gidx].reshape(B, 1, Cc), rstd[:, gidx].reshape(B, 1, Cc)
    xh = (x - mean_c) * rstd_c
    gy = dy
    if a["silu"] and fault != "no_silu_grad":
        gy = gy * _silu_grad(ga * xh + be)
    if fault != "no_gamma":
        gy = gy * ga
    valid = torch.ones(hw, dtype=torch.bool)
    s1, s2 = (_slab_sums(t, a, valid)[:, :nf].double().sum(1) for t in (gy, gy * xh))
    m1 = (s1 * inv_n).float()[:, gidx].reshape(B, 1, Cc)
    m2 = (s2 * (1.0 / hw if fault == "m2_wrong_count" else inv_n)).float()[:, gidx].reshape(B, 1, Cc)
    return {"dx": (rstd_c * (gy - m1 - xh * m2)).to(dtype)}


def _model_layernorm(a, fault):
    ext = {k: v.float().cpu() for k, v in _ext(a).items()}
    x, dy, Cc = ext["x"], ext["dy"], float(a["C"])
    mean = x.sum(-1, keepdim=True) / Cc
    rstd = torch.rsqrt(((x - mean) ** 2).sum(-1, keepdim=True) / Cc + _f32(a["eps"]))
    xh = (x - mean) * rstd
    gy = dy * ext["gamma"] if "gamma" in ext and fault != "no_gamma" else dy
    m1 = gy.sum(-1, keepdim=True) / Cc
    m2 = (gy * xh).sum(-1, keepdim=True) / (Cc + 1.0 if fault == "m2_wrong_count" else Cc)
    return {"dx": (rstd * (gy - m1 - xh * m2)).to(storage_dtype(a))}


def _drop_tail(flat, fault):
    if fault == "grid_stride_tail_dropped":
        flat[GRID_CAP_ELEMS:] = 0
    return flat


def _model_geglu(a, fault):
    ext = {k: v.float().cpu() for k, v in _ext(a).items()}
    inner, rows = a["inner"], a["rows"]
    h, d = ext["h"], ext["dg"]
    av, gt = h[:, :inner], h[:, inner:]
    cdf = 0.5 * (1.0 + torch.erf(gt * 0.70710678118654752440))
    pdf = 0.3989422804014327 * torch.exp(-0.5 * gt * gt)
    lo, hi = (_drop_tail(t.reshape(-1).clone(), fault).reshape(rows, inner) for t in (d * gt * cdf, d * av * (cdf + gt * pdf)))
    return {"dh": torch.cat([lo, hi], dim=1).to(storage_dtype(a))}


def _model_softmax(a, fault):
    ext = {k: v.float().cpu() for k, v in _ext(a).items()}
    rows, L, ldo, dtype = a["rows"], a["length"], a["ld_out"], storage_dtype(a)
    P, dP = ext["probs"], ext["dprobs"]
    e = ext.get("extra")
    t = dP + e if e is not None else dP
    s = (P * (dP if fault == "softmax_sum_without_extra" else t)).sum(-1, keepdim=True)
    fill = float("nan") if fault == "softmax_pads_unwritten" else 0.0
    out = {"dscores": torch.full((rows, ldo), fill, dtype=dtype)}
    out["dscores"][:, :L] = (_f32(a["scale"]) * P * (t - s)).to(dtype)
    if a.get("probs_out") is not None:
        out["probs_out"] = torch.full((rows, ldo), fill, dtype=dtype)
        out["probs_out"][:, :L] = P.to(dtype)
    return out


def _model_sumpool(a, fault):
    B, h, w, Cc = a["batch"], a["h"], a["w"], a["C"]
    du = _ext(a)["du"].float().cpu().reshape(B, h, 2, w, 2, Cc)
    t00, t01, t10, t11 = du[:, :, 0, :, 0], du[:, :, 0, :, 1], du[:, :, 1, :, 0], du[:, :, 1, :, 1]
    if fault == "pool_second_tap_twice":
        t10 = t01
    v = (t00 + t01) + (t10 + t11)
    return {"out": _drop_tail(v.reshape(-1).clone(), fault).reshape(B, h, w, Cc).to(storage_dtype(a))}


def model(a, fault=None):
    """{output name: tensor in the storage dtype shaped like the written region}: the fp32 model of the kernel this launch runs"""
    assert fault is None or fault in FAULTS, fault
    return {"groupnorm": _model_groupnorm, "layernorm": _model_layernorm, "geglu": _model_geglu, "softmax": _model_softmax,
            "sumpool": _model_sumpool}[a["entry"]](a, fault)


# ---- the verdict on one launch -------------------------------------------------------------------------------------------------------
def extra_tolerance(a):
    """0, but for the slab path on operands with |mean| / std >= 64: twice the relative rstd error the one-pass model shows on these
    operands (the factor of two: the summation order inside a thread differs from the model's)"""
    if a["entry"] == "groupnorm" and a.get("R", 0.0) >= 64.0 and gn_path(a) == "slab":
        return 2.0 * gn_onepass_rstd_error(a)
    return 0.0


def judge(a, outs, ref=None, mag=None, extra_tol=None):
    """every assertion on the outputs of one launch -> (failures, {output: metrics}).  ``outs``: {name: tensor shaped like the written region}
      * whole tensor and every block against the fp64 restatement at ``tols`` (+ ``extra_tolerance``), finite;
      * softmax: the pad columns of both outputs are exactly zero;
      * geglu, sumpool2x2: every element within ``element_bound``."""
    dtype = storage_dtype(a)
    ref = reference(a) if ref is None else ref
    mag = reference(a, magnitude=True) if mag is None else mag
    l2, mx = tols(dtype)
    ex = extra_tolerance(a) if extra_tol is None else extra_tol
    ids, grid = blocks(a)
    bound = element_bound(a, ref)
    fails, metrics = [], {}
    for name in ref:
        got = outs[name]
        ok, m = compare(got, ref[name], ids, grid, l2 + ex, mx + ex, mag[name])
        m["l2_tol"], m["max_tol"] = l2 + ex, mx + ex
        if not ok:
            fails.append(f"{name}: {m}")
        if a["entry"] == "softmax" and a["ld_out"] > a["length"]:
            pad = got[:, a["length"]:].double()
            if not bool((pad == 0).all()):
                fails.append(f"{name}: the pad columns [{a['length']}, {a['ld_out']}) are not exactly zero")
        if bound is not None:
            err = (got.double() - ref[name].to(got.device)).abs()
            over = torch.nan_to_num(err / bound[name].to(got.device), nan=float("inf"))
            m["worst_over_element_bound"] = float(over.max())
            if m["worst_over_element_bound"] > 1.0:
                at = [int(i) for i in torch.unravel_index(torch.argmax(over), tuple(over.shape))]
                fails.append(f"{name}: element {at} is {m['worst_over_element_bound']:.3f} x its bound")
        metrics[name] = m
    return fails, metrics


# ---- test operands -------------------------------------------------------------------------------------------------------------------
def _up8(n):
    return (n + 7) // 8 * 8


def _guarded(values, row, device, shift=0, fill=float("nan")):
    """``values`` inside a buffer of its own with one guard row (``row`` elements, rounded up to 8 so that 16-byte alignment is kept) of
    ``fill`` in front of and behind it; ``shift``: that many more elements in front (a misaligned pointer)"""
    g = _up8(max(int(row), 8))
    buf = torch.full((g + shift + values.numel() + g,), fill, dtype=values.dtype)
    buf[g + shift:g + shift + values.numel()] = values.reshape(-1)
    buf = buf.to(device)
    return buf[g + shift:g + shift + values.numel()].view(values.shape)


def _pitched(values, ld, device, fill=float("nan")):
    """[rows, L] values in rows of pitch ``ld`` (pad columns ``fill``), guarded"""
    rows, L = values.shape
    full = torch.full((rows, ld), fill, dtype=values.dtype)
    full[:, :L] = values
    return _guarded(full, ld, device)


def _out(shape, dtype, row, device):
    return _guarded(torch.full(shape, float("nan"), dtype=dtype), row, device)


def make_case(entry, dtype, *, device="cpu", seed=0, **k):
    """one launch with N(0, 1) operands drawn on the CPU from ``seed`` (the same bits on every device).  Every tensor sits in a storage of
    its own between two guard rows; input guards and input pad columns hold NaN, outputs (and the scratch) come back NaN-filled.
      groupnorm: B, hw, C, groups, silu=True, R=0 (x = R + N(0, 1)), const=(item, group, value) or None, scratch=True, x_shift=0 (elements)
      layernorm: rows, C, gamma=True, R=0
      geglu:     rows, inner, gate_sweep=False (one row of gates -8 .. 8 in steps of 0.25)
      softmax:   rows, L, ld_out, probs_fp32, extra, probs_out   (pitches: fp32 probs L + 5, dprobs roundup8(L) + 8, extra L + 3)
      sumpool:   B, h, w, C"""
    g = torch.Generator().manual_seed(7919 * seed + sum(ord(ch) for ch in entry))

    def rn(*shape):
        return torch.randn(shape, generator=g)
    if entry == "groupnorm":
        B, hw, Cc, G = k["B"], k["hw"], k["C"], k["groups"]
        R, silu = float(k.get("R", 0.0)), bool(k.get("silu", True))
        x = R + rn(B, hw, Cc)
        if k.get("const") is not None:
            it, grp, val = k["const"]
            x.reshape(B, hw, G, Cc // G)[it, :, grp, :] = val
        dy, ga, be = rn(B, hw, Cc), 1 + 0.2 * rn(Cc), 0.2 * rn(Cc)
        a = dict(entry=entry, batch=B, hw=hw, C=Cc, groups=G, eps=EPS, silu=int(silu), R=R,
                 x=_guarded(x.to(dtype), Cc, device, shift=int(k.get("x_shift", 0))), dy=_guarded(dy.to(dtype), Cc, device),
                 gamma=_guarded(ga.to(dtype), Cc, device), beta=_guarded(be.to(dtype), Cc, device), dx=_out((B, hw, Cc), dtype, Cc, device),
                 partials=None)
        if k.get("scratch", True):
            a["partials"] = _out((gn_scratch_floats(B, hw, G),), torch.float32, 4 * G, device)
        return a
    if entry == "layernorm":
        rows, Cc = k["rows"], k["C"]
        R = float(k.get("R", 0.0))
        x, dy, ga = R + rn(rows, Cc), rn(rows, Cc), 1 + 0.2 * rn(Cc)
        return dict(entry=entry, rows=rows, C=Cc, eps=EPS, R=R, x=_guarded(x.to(dtype), Cc, device), dy=_guarded(dy.to(dtype), Cc, device),
                    gamma=_guarded(ga.to(dtype), Cc, device) if k.get("gamma", True) else None, dx=_out((rows, Cc), dtype, Cc, device))
    if entry == "geglu":
        rows, inner = k["rows"], k["inner"]
        h, dg = rn(rows, 2 * inner), rn(rows, inner)
        if k.get("gate_sweep"):
            assert rows == 1 and inner == 65
            h[0, inner:] = torch.arange(-32, 33) * 0.25
        return dict(entry=entry, rows=rows, inner=inner, h=_guarded(h.to(dtype), 2 * inner, device), dg=_guarded(dg.to(dtype), inner, device),
                    dh=_out((rows, 2 * inner), dtype, 2 * inner, device))
    if entry == "softmax":
        rows, L, ldo = k["rows"], k["L"], k["ld_out"]
        P = torch.softmax(1.5 * rn(rows, L), -1)
        dP, ex = rn(rows, L).to(dtype), 0.3 * rn(rows, L)
        fp32 = bool(k.get("probs_fp32", True))
        ldp, ldd, lde = (L + 5 if fp32 else L), _up8(L) + 8, L + 3
        return dict(entry=entry, rows=rows, length=L, scale=0.35, probs_fp32=int(fp32), ld_probs=ldp, ld_dprobs=ldd, ld_extra=lde if k.get("extra") else 0,
                    ld_out=ldo, probs=_pitched(P if fp32 else P.to(dtype), ldp, device), dprobs=_pitched(dP, ldd, device),
                    extra=_pitched(ex, lde, device) if k.get("extra") else None, dscores=_out((rows, ldo), dtype, ldo, device),
                    probs_out=_out((rows, ldo), dtype, ldo, device) if k.get("probs_out") else None)
    assert entry == "sumpool", entry
    B, h, w, Cc = k["B"], k["h"], k["w"], k["C"]
    return dict(entry=entry, batch=B, h=h, w=w, C=Cc, du=_guarded(rn(B, 2 * h, 2 * w, Cc).to(dtype), Cc, device),
                out=_out((B, h, w, Cc), dtype, Cc, device))


# ---- the launches of tests/test_backward_edges_gpu.py ----------------------------------------------------------------------------------
def _gn(B, hw, Cc, G, **k):
    return ("groupnorm", dict(B=B, hw=hw, C=Cc, groups=G, **k))


GN_SLAB_CASES = {
    "1x1x64g32": _gn(1, 1, 64, 32),                                  # one row: 31 of the 32 thread rows idle
    "1x31x320g32": _gn(1, 31, 320, 32),                              # one slab, one row short of 32; 10-channel groups straddle the chunks
    "1x33x320g32": _gn(1, 33, 320, 32),                              # two slabs of 17 and 16 rows
    "3x1387x64g32": _gn(3, 1387, 64, 32),                            # 42 slabs of 34 rows: the last one is empty
    "130x40x64g32": _gn(130, 40, 64, 32),                            # batch >= 128: one slab
    "1x144x2560g32": _gn(1, 144, 2560, 32),                          # two chunks per thread
    "1x40x2056g8": _gn(1, 40, 2056, 8),                              # the second chunk slot for one thread column only
    "1x40x4096g32": _gn(1, 40, 4096, 32),                            # the largest slab shape
    "2x100x24g3": _gn(2, 100, 24, 3),                                # TC = 3, TR = 85: thread 255 idle
    "1x300x8g2-nosilu": _gn(1, 300, 8, 2, silu=False),               # TR = 256
    "1x64x512g256": _gn(1, 64, 512, 256),                            # every thread folds
    "2x577x640g32-const": _gn(2, 577, 640, 32, const=(1, 5, 2.0)),   # zero variance in one (item, group)
}
GN_FALLBACK_CASES = {
    "1x100x36g4": (_gn(1, 100, 36, 4), "channels not a multiple of 8"),
    "1x64x4104g8": (_gn(1, 64, 4104, 8), "channels > 4096"),
    "1x64x528g264": (_gn(1, 64, 528, 264), "groups > 256"),
    "2x64x320g32-noscratch": (_gn(2, 64, 320, 32, scratch=False), "partials is NULL"),
    "2x64x320g32-xshift4": (_gn(2, 64, 320, 32, x_shift=4), "a pointer is not 16-byte aligned"),
}
GN_OFFSET_CASES = {f"{B}x{hw}x{Cc}g{G}-R{R}{'' if scratch else '-noscratch'}": _gn(B, hw, Cc, G, R=float(R), scratch=scratch)
                   for (B, hw, Cc, G) in ((1, 1024, 320, 32), (1, 144, 2560, 32)) for R in (4, 16, 64) for scratch in (True, False)}
LN_CASES = {f"{r}x{c}": ("layernorm", dict(rows=r, C=c)) for r, c in ((1, 8), (3, 36), (5, 64), (4, 320), (7, 1280), (2, 4096), (3, 1))}
LN_CASES["5x320-nogamma"] = ("layernorm", dict(rows=5, C=320, gamma=False))
LN_CASES["6x320-R16"] = ("layernorm", dict(rows=6, C=320, R=16.0))
GEGLU_CASES = {f"{r}x{i}": ("geglu", dict(rows=r, inner=i)) for r, i in ((1, 1), (130, 256), (1030, 1024))}
GEGLU_CASES["gate-sweep"] = ("geglu", dict(rows=1, inner=65, gate_sweep=True))
POOL_CASES = {f"{B}x{h}x{w}x{c}": ("sumpool", dict(B=B, h=h, w=w, C=c)) for B, h, w, c in ((1, 1, 1, 1), (2, 3, 5, 7), (1, 33, 33, 1024))}
SM_ROWS, SM_LENGTHS = (1, 5, 70), (1, 8, 63, 64, 65, 77, 264)


def softmax_cases(L):
    """every (rows, ld_out, probs dtype, extra, probs_out) combination at one length"""
    return {f"r{rows}-L{L}-ld{ld}-{'p32' if p32 else 'pst'}-{'ex' if ex else 'noex'}-{'po' if po else 'nopo'}":
            ("softmax", dict(rows=rows, L=L, ld_out=ld, probs_fp32=p32, extra=ex, probs_out=po))
            for rows, ld, p32, ex, po in itertools.product(SM_ROWS, (_up8(L), _up8(L) + 16), (True, False), (True, False), (True, False))}


def all_cases():
    """{id: (entry, make_case keywords)} of every GPU launch"""
    out = {}
    for fam, cs in (("gn-slab", GN_SLAB_CASES), ("gn-fallback", {k: v[0] for k, v in GN_FALLBACK_CASES.items()}), ("gn-offset", GN_OFFSET_CASES),
                    ("ln", LN_CASES), ("geglu", GEGLU_CASES), ("pool", POOL_CASES)):
        out.update({f"{fam} {k}": v for k, v in cs.items()})
    for L in SM_LENGTHS:
        out.update({f"softmax {k}": v for k, v in softmax_cases(L).items()})
    return out
