"""The C-ABI contracts of the six forward normalising entries (csrc/tg_norm.hip, csrc/tg_layernorm_add.hip) restated in fp64 from
include/theatergen_hip.h ("Normalisation"), for checking single hand-made launches: ``tg_groupnorm``, ``tg_groupnorm_coef``,
``tg_groupnorm_from_partials`` (coefficient and apply mode), ``tg_layernorm``, ``tg_layernorm_stats``, ``tg_layernorm_add``.

A launch is a plain dict: ``entry`` plus the C argument names; tensors stand for the pointers.  Operands are read the way the kernels read raw
pointers, ``gemm_contract.Region`` over the operand's storage along the pitches of the call; a contract that reads past a storage raises.

    groupnorm       x = [x0 | x1] per pixel; over one (item, group): mean, var = E[(x - mean)^2]; rstd = (var + eps)^-1/2
                    a[c] = rstd gamma[c] (gamma NULL: 1), d[c] = beta[c] - mean a[c] (beta NULL: 0); out = act(x a + d), act = SiLU or identity
    groupnorm_coef  coef[b][0][c] = a, coef[b][1][c] = d (fp32)
    from_partials   mean = S / n, var = max(Q / n - mean^2, 0) with (S, Q) the sums over the producer's ``nblk`` fp32 entries per (item, group)
    layernorm       out[r, :] = (x[r, :] - mean) rstd (gamma) (+ beta) over one row;  stats[r] = (rstd, -rstd mean) (fp32)
    layernorm_add   the same over x[r, :] + res[r, :], the sum never rounded

  * ``reference(a)``: fp64 over the stored operands; ``plan(a)``: the C gates restated (which kernel, its geometry); ``blocks(a)``: the unit one
    workgroup or lane group owns; ``model(a, fault=None)``: fp32 CPU models of the kernels' own arithmetic and summation order, one switch per fault;
  * ``figures`` / ``bounds_from`` / ``judge``: the assertions of tests/test_norm_edges_gpu.py; ``CASES`` / ``make_case``: its launches, drawn on the
    CPU from a seed; every input element the contract does not read (pad columns, guard rows) holds NaN, outputs and scratch come NaN-filled.

Bounds (none tuned on a kernel).
  Storage-dtype outputs: per case and dtype 1.5 x the model's rel-L2 for the whole tensor and for the worst block, 2 x its max|err| / max|ref|
  (the row-chain tests' rule).  The one allowance: the two-launch GroupNorm path at |mean| / std >= 64 adds twice the relative rstd error the
  one-pass model shows on the same operands (``extra_tolerance``), and only if the model itself leaves the floor there.
  fp32 outputs (coef, stats), per element, u = 2^-24, L = the longest fp32 addition chain of the case's plan (``chain``):
    two-launch   L = ceil(per / ry) + (ry - 1) + cpg  (a thread's pixels, the row fold, the group fold; the partials are then folded in fp64).
                 |dS| <= L u sum|x|, |dQ| <= L u sum x^2 (the squares of storage values are exact in fp32), so
                 dmean <= L u E|x| + u |mean|;  dvar <= L u (E[x^2] + 2 |mean| E|x|);  rel(rstd) <= dvar / (2 (var + eps)) + u
    small, LN    two passes.  L = 8 MAXP' + npy + cpg / 8 (MAXP' = the plan's maxp), or 8 MAXC + log2 LPR.
                 dmean <= (L + 2) u E|x|;  rel(var) <= (L + 4) u + dmean^2 / var;  rel(rstd) <= rel(var) / 2 + 4 u  (rsqrtf: 2 u, eps add, rounding)
    partials     the sums are operands: dmean <= u |mean|, rel(rstd) <= u
    then a = rstd gamma: rel(a) <= rel(rstd) + u;  d = beta - mean a: |dd| <= |mean a| (rel(a) + u) + |a| dmean + u |d|;
    stats: rel(rstd) as above, |d(-rstd mean)| <= |rstd mean| (rel(rstd) + u) + rstd dmean.
  These are worst-case sums of magnitudes, not tuned: the model sits at a few per cent of them (tests/test_norm_contract_cpu.py prints it).
"""
import functools
import math

import torch

from tests import backward_contract as bc
from tests import launch_check as lc
from tests.gemm_contract import Region

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
U = 2.0 ** -24
GN_MAX_C = 8 * 256 * 4
LN_ENTRIES = ("layernorm", "layernorm_stats", "layernorm_add")
FAULTS = ("partial_drops_last_pixel", "apply_skips_remainder", "prefetch_on_second_slot", "fold_npart_minus_1", "from_partials_wrong_nblk",
          "group_of_chunk_head", "x1_with_c0_pitch", "count_c0", "eps_outside_sqrt", "beta_dropped_without_gamma", "small_ragged_lane_included",
          "ln_drops_ragged_chunk", "stats_wrong_sign")


def _f32(v):
    return float(torch.tensor(float(v), dtype=torch.float32))


def _cdiv(a, b):
    return (a + b - 1) // b


# ---- the C gates --------------------------------------------------------------------------------------------------------------------------
def gn_nblk(batch, hw):
    return max(1, min(hw // 8, max(512 // max(batch, 1), 1)))


def gn_scratch_floats(batch, hw, groups):
    return batch * gn_nblk(batch, hw) * groups * 2 + batch * groups * 2


def gn_small_plan(Cc, groups, hw):
    """(geometry, None) of the one-launch path or (None, why it is refused)"""
    cpg = Cc // groups
    if hw > 256:
        return None, "hw > 256"
    if cpg % 8:
        return None, "channels per group not a multiple of 8"
    g = 1
    while g < groups and (g * cpg < 64 or groups % g):
        g += 1
    if groups % g or g > 16:
        return None, "groups per block > 16"
    n = g * cpg // 8
    if n > 256:
        return None, "chunk columns > 256"
    y = 256 // n
    mp = _cdiv(hw, y)
    if mp > 24:
        return None, "pixels per lane > 24"
    return dict(gpb=g, nc=n, npy=y, maxp=mp, MAXP=3 if mp <= 3 else 6 if mp <= 6 else 12 if mp <= 12 else 24), None


def ln_instance(Cc, add=False):
    cpr = Cc // 8
    for lim, inst in ((8, (8, 1)), (40, (8, 5)), (80, (16, 5)), (160, (32, 5)), (256, (64, 4)), (512, (64, 8))):
        if cpr <= lim:
            return inst if not add or lim <= 160 else None
    return None


def _al16(t):
    return t is None or t.data_ptr() % 16 == 0


def channels(a):
    return a["c0"] + (a["c1"] if a.get("x1") is not None else 0) if a["entry"] != "from_partials" else a["C"]


def plan(a):
    """the kernel a call runs and its geometry, restated from the host code of csrc/tg_norm.hip / tg_layernorm_add.hip"""
    e = a["entry"]
    if e in LN_ENTRIES:
        LPR, MAXC = ln_instance(a["C"], add=e == "layernorm_add")
        rpb = 4 * (64 // LPR)
        return dict(path="layernorm", LPR=LPR, MAXC=MAXC, rows_per_block=rpb, grid=_cdiv(a["rows"], rpb), chain=8 * MAXC + int(math.log2(LPR)))
    Cc, G, B, hw = channels(a), a["groups"], a["batch"], a["hw"]
    cpg, cpr = Cc // G, Cc // 8
    cx = min(cpr, 256)
    ry = 256 // cx
    nblk = gn_nblk(B, hw)
    per = _cdiv(hw, nblk)
    two = dict(gn_nblk=nblk, per=per, cx=cx, ry=ry, slots=_cdiv(cpr, cx), lds_bytes=ry * 2 * Cc * 4, npart=nblk, stat_trips=_cdiv(G, 32),
               chain=_cdiv(per, ry) + ry - 1 + cpg)
    if e == "from_partials":
        return dict(two, path="partials-coef" if a.get("coef") is not None else "partials-apply", npart=a["nblk"], lds_bytes=0, chain=1)
    if not (_al16(a.get("gamma")) and _al16(a.get("beta"))):
        return dict(two, path="two-launch", why="gamma / beta not 16-byte aligned")
    sm, why = gn_small_plan(Cc, G, hw)
    if sm is None:
        return dict(two, path="two-launch", why=why)
    return dict(sm, path="small", grid=(G // sm["gpb"], B), chain=8 * sm["maxp"] + sm["npy"] + cpg // 8)


def host_check_failures(a):
    """the TG_CHECKs of the entry restated: empty for a call the library accepts"""
    e, f = a["entry"], []
    ptr = lambda k: 0 if a.get(k) is None else (a[k] if isinstance(a[k], int) else a[k].data_ptr())
    if a.get("dtype_code", 0) not in (0, 1):
        f.append("dtype")
    if e in LN_ENTRIES:
        Cc = a["C"]
        need = ("x", "stats") if e == "layernorm_stats" else ("x", "res", "gamma", "beta", "out") if e == "layernorm_add" else ("x", "out")
        if any(ptr(k) == 0 for k in need):
            f.append("null pointer")
        if a["rows"] < 1 or Cc < 8 or Cc % 8:
            f.append("rows / C")
        if Cc > (1280 if e == "layernorm_add" else 4096):
            f.append("C too large")
        lds = [a[k] for k in ("ldx", "ldres", "ldo") if k in a]
        if any(ld % 8 or ld < Cc for ld in lds):
            f.append("pitch")
        if any(ptr(k) % 16 for k in ("x", "res", "gamma", "beta", "out")) or ptr("stats") % 8:
            f.append("alignment")
        return f
    Cc, G = channels(a), a["groups"]
    if e == "from_partials":
        if ptr("partials") == 0 or a["nblk"] < 1 or (ptr("coef") == 0 and (ptr("x") == 0 or ptr("out") == 0)):
            f.append("null pointer")
        if G > 256 or Cc % 8:
            f.append("shape")
        if ptr("coef") == 0 and (ptr("x") % 16 or ptr("out") % 16):
            f.append("alignment")
    else:
        if ptr("x0") == 0 or ptr("partials") == 0 or ptr("coef" if e == "groupnorm_coef" else "out") == 0:
            f.append("null pointer")
        if a["c0"] % 8 or (a.get("x1") is not None and a["c1"] % 8) or (e == "groupnorm_coef" and G > 256):
            f.append("shape")
        if any(ptr(k) % 16 for k in ("x0", "x1", "out")):
            f.append("alignment")
    if a["batch"] < 1 or a["hw"] < 1 or G < 1 or Cc % max(G, 1) or Cc > GN_MAX_C:
        f.append("shape")
    if a["batch"] > 65535:
        f.append("batch")
    return f


# ---- regions ------------------------------------------------------------------------------------------------------------------------------
def _reg(name, t, sizes, strides):
    return Region(name, t, 0, tuple(int(s) for s in sizes), tuple(int(s) for s in strides))


def read_extents(a):
    e = a["entry"]
    regs = []
    if e in LN_ENTRIES:
        regs.append(_reg("x", a["x"], (a["rows"], a["C"]), (a["ldx"], 1)))
        if e == "layernorm_add":
            regs.append(_reg("res", a["res"], (a["rows"], a["C"]), (a["ldres"], 1)))
    elif e == "from_partials":
        B, hw, Cc, G = a["batch"], a["hw"], a["C"], a["groups"]
        if a.get("coef") is None:
            regs.append(_reg("x", a["x"], (B, hw, Cc), (hw * Cc, Cc, 1)))
        regs.append(_reg("partials", a["partials"], (B, a["nblk"], G, 2), (a["nblk"] * G * 2, G * 2, 2, 1)))
    else:
        B, hw = a["batch"], a["hw"]
        regs.append(_reg("x0", a["x0"], (B, hw, a["c0"]), (hw * a["c0"], a["c0"], 1)))
        if a.get("x1") is not None:
            regs.append(_reg("x1", a["x1"], (B, hw, a["c1"]), (hw * a["c1"], a["c1"], 1)))
    if e != "layernorm_stats":
        Cc = a["C"] if e in LN_ENTRIES else channels(a)
        regs += [_reg(n, a[n], (Cc,), (1,)) for n in ("gamma", "beta") if a.get(n) is not None]
    return regs


def written_region(a):
    """the output and, for the two GroupNorm entries that take it, the part of the scratch the path of ``plan`` writes (small path: none)"""
    e = a["entry"]
    if e == "layernorm_stats":
        return [_reg("stats", a["stats"], (a["rows"], 2), (2, 1))]
    if e in LN_ENTRIES:
        return [_reg("out", a["out"], (a["rows"], a["C"]), (a["ldo"], 1))]
    B, hw, Cc, G = a["batch"], a["hw"], channels(a), a["groups"]
    regs = [_reg("coef", a["coef"], (B, 2, Cc), (2 * Cc, Cc, 1))] if a.get("coef") is not None else [_reg("out", a["out"], (B, hw, Cc), (hw * Cc, Cc, 1))]
    if e != "from_partials" and plan(a)["path"] == "two-launch":
        n = gn_nblk(B, hw)
        regs.append(_reg("partials", a["partials"], (B, n, G, 2), (n * G * 2, G * 2, 2, 1)))
    return regs


def _ext(a):
    return {r.name: r.view().cpu() for r in read_extents(a)}


def storage_dtype(a):
    return a["dtype"]


def _x(ext, a):
    return torch.cat([ext["x0"], ext["x1"]], dim=-1) if "x1" in ext else ext.get("x0", ext.get("x"))


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
def gn_stats64(a, ext=None):
    """fp64 per (item, group): mean, var, E|x|, E[x^2] — from x, or from the partial sums for tg_groupnorm_from_partials"""
    ext = _ext(a) if ext is None else ext
    B, hw, Cc, G = a["batch"], a["hw"], channels(a), a["groups"]
    if a["entry"] == "from_partials":
        p = ext["partials"].double().sum(1)
        n = float(hw * (Cc // G))
        mean = p[..., 0] / n
        m2 = p[..., 1] / n
        return dict(mean=mean, var=(m2 - mean * mean).clamp_min(0.0), m1=mean.abs(), m2=m2)
    x = _x(ext, a).double().reshape(B, hw, G, Cc // G)
    mean = x.mean((1, 3))
    return dict(mean=mean, var=((x - mean[:, None, :, None]) ** 2).mean((1, 3)), m1=x.abs().mean((1, 3)), m2=(x * x).mean((1, 3)))


def _silu(z):
    return z / (1.0 + torch.exp(-z))


def reference(a):
    """{output name: fp64 tensor shaped like the output's written region}"""
    e, ext = a["entry"], _ext(a)
    eps = _f32(a["eps"])
    if e in LN_ENTRIES:
        x = ext["x"].double() + (ext["res"].double() if e == "layernorm_add" else 0.0)
        mean = x.mean(1, keepdim=True)
        rstd = (((x - mean) ** 2).mean(1, keepdim=True) + eps) ** -0.5
        if e == "layernorm_stats":
            return {"stats": torch.cat([rstd, -rstd * mean], dim=1)}
        y = (x - mean) * rstd
        if "gamma" in ext:
            y = y * ext["gamma"].double()
        return {"out": y + ext["beta"].double() if "beta" in ext else y}
    B, hw, Cc, G = a["batch"], a["hw"], channels(a), a["groups"]
    st = gn_stats64(a, ext)
    rep = lambda t: t.repeat_interleave(Cc // G, dim=1)
    ca = rep((st["var"] + eps) ** -0.5) * (ext["gamma"].double() if "gamma" in ext else 1.0)
    cd = (ext["beta"].double() if "beta" in ext else 0.0) - rep(st["mean"]) * ca
    if a.get("coef") is not None:
        return {"coef": torch.stack([ca, cd], dim=1)}
    y = _x(ext, a).double() * ca[:, None, :] + cd[:, None, :]
    return {"out": _silu(y) if a["silu"] else y}


# ---- ownership ----------------------------------------------------------------------------------------------------------------------------
def blocks(a):
    """(ids, grid) for the entry's output: (item, slab, group) for the two-launch / from-partials apply pass, (item, group) for the small path and for
    coefficients (either component), a row for the LayerNorm entries"""
    e = a["entry"]
    ar = torch.arange
    if e in LN_ENTRIES:
        rows, cols = a["rows"], 2 if e == "layernorm_stats" else a["C"]
        return ar(rows).reshape(rows, 1).expand(rows, cols).contiguous(), (rows,)
    B, hw, Cc, G = a["batch"], a["hw"], channels(a), a["groups"]
    g = ar(Cc) // (Cc // G)
    b = ar(B)
    if a.get("coef") is not None:
        return (b.reshape(B, 1, 1) * G + g.reshape(1, 1, Cc)).expand(B, 2, Cc).contiguous(), (B, G)
    pl = plan(a)
    if pl["path"] == "small":
        return (b.reshape(B, 1, 1) * G + g.reshape(1, 1, Cc)).expand(B, hw, Cc).contiguous(), (B, G)
    S = pl["gn_nblk"]
    slab = (ar(hw) // pl["per"]).reshape(1, hw, 1)
    return ((b.reshape(B, 1, 1) * S + slab) * G + g.reshape(1, 1, Cc)).contiguous(), (B, S, G)


# ---- fp32 models of the kernels -----------------------------------------------------------------------------------------------------------
def _fma(x, y, z):
    """round_fp32(x y + z): the product of two fp32 values and the sum are exact enough in fp64 that the one rounding is fma's (double rounding can
    differ from a true fma by one fp32 ulp in ~2^-29 of the cases)"""
    return (x.double() * y.double() + z.double()).float()


def _seq_sum(t, dim=-1):
    """fp32 (or fp64) sum over ``dim``, one term after the other"""
    t = t.movedim(dim, 0)
    s = torch.zeros_like(t[0])
    for i in range(t.shape[0]):
        s = s + t[i]
    return s


def _silu32(f):
    return f * (1.0 / (1.0 + torch.exp2(-1.4426950408889634 * f)))


def _slab_partials(a, x, pl, fault):
    """gn_partial_kernel: fp32 [B, nblk, G, 2].  Thread (column, row ty) adds the pixels ty, ty + ry, .. of its slab per channel (the 4-pixel trips
    and the remainder loop add in that same order), the ry rows are folded one after the other, one thread per group then adds the group's channels"""
    B, hw, Cc, G = a["batch"], a["hw"], channels(a), a["groups"]
    nblk, per, ry = pl["gn_nblk"], pl["per"], pl["ry"]
    valid = torch.ones(hw)
    if fault == "partial_drops_last_pixel":
        for blk in range(nblk):
            r1 = min((blk + 1) * per, hw)
            if r1 > blk * per:
                valid[r1 - 1] = 0.0
    K = _cdiv(per, ry)
    out = []
    for v in (x, x * x):
        v = v * valid.reshape(1, hw, 1)
        v = torch.nn.functional.pad(v, (0, 0, 0, nblk * per - hw)).reshape(B, nblk, per, Cc)
        v = torch.nn.functional.pad(v, (0, 0, 0, K * ry - per)).reshape(B, nblk, K, ry, Cc)
        rows = _seq_sum(_seq_sum(v, 2), 2)
        out.append(_seq_sum(rows.reshape(B, nblk, G, Cc // G)))
    return torch.stack(out, dim=-1)


def _fold_partials(p, npart):
    """gn_block_stats: thread ``part`` of 8 adds every 8th partial in fp64, the 8 parts are then added in order -> fp64 [B, G, 2]"""
    parts = [_seq_sum(p[:, k:npart:8].double(), 1) if k < npart else torch.zeros_like(p[:, 0].double()) for k in range(8)]
    return _seq_sum(torch.stack(parts, dim=0), 0)


def _stats_from_sums(sq, cnt, eps, fault):
    mean = sq[..., 0] / cnt
    var = (sq[..., 1] / cnt - mean * mean).clamp_min(0.0)
    rstd = 1.0 / (torch.sqrt(var) + eps) if fault == "eps_outside_sqrt" else 1.0 / torch.sqrt(var + eps)
    return mean.float(), rstd.float()


def _small_stats(a, x, pl, fault):
    """gn_small_kernel: two passes over the register-resident slab; thread (chunk column, pixel lane py) owns the pixels py, py + npy, ..; LDS folds
    over the pixel lanes, then over the chunk columns of a group"""
    B, hw, Cc, G = a["batch"], a["hw"], channels(a), a["groups"]
    npy, mp, cpg = pl["npy"], pl["maxp"], Cc // G
    pad = mp * npy - hw
    live = torch.cat([torch.ones(hw), torch.zeros(pad)])
    xp = torch.cat([x, x[:, hw - 1:hw].expand(B, pad, Cc)], dim=1)               # out-of-range pixels re-read the last one ...
    if fault != "small_ragged_lane_included":
        xp = xp * live.reshape(1, -1, 1)                                          # ... and are ignored
    lanes = lambda v: v.reshape(B, mp, npy, Cc // 8, 8).permute(0, 2, 3, 1, 4).reshape(B, npy, Cc // 8, mp * 8)
    fold = lambda t: _seq_sum(_seq_sum(t, 1).reshape(B, G, cpg // 8))          # [B, npy, chunks] -> [B, G]
    inv_n = torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(float(hw), dtype=torch.float32) * float(cpg))
    mean = fold(_seq_sum(lanes(xp))) * inv_n
    d = xp - mean.repeat_interleave(cpg, dim=1)[:, None, :]
    if fault != "small_ragged_lane_included":
        d = d * live.reshape(1, -1, 1)
    rstd = torch.rsqrt(fold(_seq_sum(lanes(d * d))) * inv_n + _f32(a["eps"]))
    return mean, rstd


def _model_groupnorm(a, fault):
    ext = _ext(a)
    B, hw, Cc, G = a["batch"], a["hw"], channels(a), a["groups"]
    cpg = Cc // G
    dtype = storage_dtype(a)
    pl = plan(a)
    e = a["entry"]
    x = None
    if "x0" in ext or "x" in ext:
        if fault == "x1_with_c0_pitch" and "x1" in ext:
            x1 = a["x1"].cpu().reshape(-1)
            idx = (torch.arange(B * hw).reshape(-1, 1) * a["c0"] + torch.arange(a["c1"]).reshape(1, -1)) % x1.numel()
            x = torch.cat([ext["x0"], x1[idx].reshape(B, hw, a["c1"])], dim=-1).float()
        else:
            x = _x(ext, a).float()
    cnt = float(hw) * ((a["c0"] // G) if fault == "count_c0" else cpg)
    eps = float(_f32(a["eps"]))
    if pl["path"] == "small":
        mean, rstd = _small_stats(a, x, pl, fault)
    elif e == "from_partials":
        p = ext["partials"]
        npart = a["nblk"]
        if fault == "from_partials_wrong_nblk":
            flat = torch.cat([p.reshape(-1), torch.zeros(B * max(pl["gn_nblk"], npart) * G * 2)])
            p = flat.as_strided((B, npart, G, 2), (pl["gn_nblk"] * G * 2, G * 2, 2, 1))
        mean, rstd = _stats_from_sums(_fold_partials(p, npart - 1 if fault == "fold_npart_minus_1" else npart), cnt, eps, fault)
    else:
        p = _slab_partials(a, x, pl, fault)
        mean, rstd = _stats_from_sums(_fold_partials(p, pl["npart"] - 1 if fault == "fold_npart_minus_1" else pl["npart"]), cnt, eps, fault)
    c = torch.arange(Cc)
    gidx = (c // 8 * 8 if fault == "group_of_chunk_head" else c) // cpg
    ga = ext["gamma"].float() if "gamma" in ext else torch.ones(Cc)
    be = ext["beta"].float() if "beta" in ext else torch.zeros(Cc)
    if fault == "beta_dropped_without_gamma" and "gamma" not in ext:
        be = torch.zeros(Cc)
    ca = rstd[:, gidx] * ga[None, :]
    cd = _fma(-mean[:, gidx], ca, be[None, :].expand(B, Cc))
    if a.get("coef") is not None:
        return {"coef": torch.stack([ca, cd], dim=1)}
    xin = x
    if fault == "prefetch_on_second_slot" and pl["path"] != "small" and pl["slots"] > 1:
        # the first trip of every chunk slot is served from the registers prefetched for slot 0 (only where the prefetch ran: >= 4 pixels in the thread's row)
        per, ry, cx = pl["per"], pl["ry"], pl["cx"]
        pix = torch.arange(hw)
        blk, off = pix // per, pix % per
        n_row = (torch.clamp((blk + 1) * per, max=hw) - blk * per - off % ry + ry - 1) // ry         # pixels of the thread row that owns ``pix``
        first = (off // ry < 4) & (n_row >= 4)
        src = torch.arange(Cc // 8) % cx
        alt = x.reshape(B, hw, Cc // 8, 8)[:, :, src].reshape(B, hw, Cc)
        xin = torch.where(first.reshape(1, hw, 1), alt, x)
    f = _fma(xin, ca[:, None, :], cd[:, None, :])
    if a["silu"]:
        f = _silu32(f)
    out = f.to(dtype)
    if fault == "apply_skips_remainder" and pl["path"] != "small":
        per, ry = pl["per"], pl["ry"]
        pix = torch.arange(hw)
        blk, off = pix // per, pix % per
        n_row = (torch.clamp((blk + 1) * per, max=hw) - blk * per - off % ry + ry - 1) // ry
        out[:, off // ry >= n_row // 4 * 4] = float("nan")
    return {"out": out}


def _ln_lane_sum(v, cpr, LPR, MAXC, keep):
    """v fp32 [rows, C] -> the xor-shuffle tree's result [rows]: lane l adds its chunks l, l + LPR, .. element by element, then lanes l and l ^ o are
    added for o = LPR / 2 .. 1.  ``keep`` [chunks] masks chunks out of the sum"""
    rows = v.shape[0]
    v = v.reshape(rows, cpr, 8) * keep.reshape(1, cpr, 1)
    v = torch.nn.functional.pad(v, (0, 0, 0, LPR * MAXC - cpr)).reshape(rows, MAXC, LPR, 8).permute(0, 2, 1, 3).reshape(rows, LPR, MAXC * 8)
    s = _seq_sum(v)
    while s.shape[1] > 1:
        h = s.shape[1] // 2
        s = s[:, :h] + s[:, h:]
    return s


def _model_layernorm(a, fault):
    ext = _ext(a)
    e, Cc = a["entry"], a["C"]
    pl = plan(a)
    LPR, MAXC, cpr = pl["LPR"], pl["MAXC"], Cc // 8
    x = ext["x"].float() + ext["res"].float() if e == "layernorm_add" else ext["x"].float()
    keep = torch.ones(cpr)
    if fault == "ln_drops_ragged_chunk" and cpr % LPR:
        keep[cpr // LPR * LPR:] = 0.0
    mean = _ln_lane_sum(x, cpr, LPR, MAXC, keep) / float(Cc)
    d = x - mean
    rstd = torch.rsqrt(_ln_lane_sum(d * d, cpr, LPR, MAXC, keep) / float(Cc) + _f32(a["eps"]))
    if e == "layernorm_stats":
        return {"stats": torch.cat([rstd, rstd * mean if fault == "stats_wrong_sign" else -rstd * mean], dim=1)}
    y = d * rstd
    if "gamma" in ext:
        y = y * ext["gamma"].float()
    if "beta" in ext and not (fault == "beta_dropped_without_gamma" and "gamma" not in ext):
        y = y + ext["beta"].float()
    return {"out": y.to(storage_dtype(a))}


def model(a, fault=None):
    """{output name: tensor shaped like the written region}: the fp32 model of the kernel this launch runs (storage dtype, or fp32 for coef / stats)"""
    assert fault is None or fault in FAULTS, fault
    return (_model_layernorm if a["entry"] in LN_ENTRIES else _model_groupnorm)(a, fault)


def onepass_rstd_error(a):
    """largest relative error over the (item, group)s of the two-launch path's rstd (fp32 slab sums of x and x^2, E[x^2] - mean^2) against fp64"""
    pl = plan(a)
    x = _x(_ext(a), a).float()
    cnt = float(a["hw"]) * (channels(a) // a["groups"])
    _, rstd = _stats_from_sums(_fold_partials(_slab_partials(a, x, pl, None), pl["npart"]), cnt, float(_f32(a["eps"])), None)
    want = (gn_stats64(a)["var"] + _f32(a["eps"])) ** -0.5
    return float(((rstd.double() - want) / want).abs().max())


# ---- figures, bounds, verdict -------------------------------------------------------------------------------------------------------------
def fp32_bound(a):
    """{"coef" | "stats": fp64 tensor of per-element bounds} for the fp32 outputs (module docstring); None for the other launches"""
    e = a["entry"]
    pl = plan(a)
    L = pl["chain"]
    eps = _f32(a["eps"])
    if e == "layernorm_stats":
        ext = _ext(a)
        x = ext["x"].double()
        mean = x.mean(1, keepdim=True)
        var = ((x - mean) ** 2).mean(1, keepdim=True)
        rstd = (var + eps) ** -0.5
        dmean = (L + 2) * U * x.abs().mean(1, keepdim=True)
        rel = 0.5 * ((L + 4) * U + dmean ** 2 / (var + eps)) + 4 * U
        return {"stats": torch.cat([rstd * rel, (rstd * mean).abs() * (rel + U) + rstd * dmean], dim=1)}
    if a.get("coef") is None:
        return None
    ext = _ext(a)
    Cc, G = channels(a), a["groups"]
    st = gn_stats64(a, ext)
    if pl["path"] == "two-launch":
        dmean = L * U * st["m1"] + U * st["mean"].abs()
        rel = L * U * (st["m2"] + 2 * st["mean"].abs() * st["m1"]) / (2 * (st["var"] + eps)) + U
    elif pl["path"] == "small":
        dmean = (L + 2) * U * st["m1"]
        rel = 0.5 * ((L + 4) * U + dmean ** 2 / (st["var"] + eps)) + 4 * U
    else:
        dmean, rel = U * st["mean"].abs(), torch.full_like(st["mean"], U)
    rep = lambda t: t.repeat_interleave(Cc // G, dim=1)
    ref = reference(a)["coef"]
    ca, cd = ref[:, 0].abs(), ref[:, 1].abs()
    rel_a = rep(rel) + U
    return {"coef": torch.stack([ca * rel_a, rep(st["mean"].abs()) * ca * (rel_a + U) + ca * rep(dmean) + U * cd], dim=1)}


def figures(a, outs, ref):
    """{output: (rel-L2, worst block rel-L2, max|err| / max|ref|, finite, worst block's coordinates)} — backward_contract.compare's definitions"""
    ids, grid = blocks(a)
    fig = {}
    for name, want in ref.items():
        _, m = bc.compare(outs[name].cpu(), want, ids, grid, math.inf, math.inf)
        fig[name] = (m["rel_l2"], m["block_rel_l2"], m["max_rel"], m["finite"], m["block_at"])
    return fig


def extra_tolerance(a):
    """0 but for the two-launch path at |mean| / std >= 64: twice the relative rstd error the one-pass model shows on these operands"""
    if a["entry"] in ("groupnorm", "groupnorm_coef") and a.get("R", 0.0) >= 64.0 and plan(a)["path"] == "two-launch":
        return 2.0 * onepass_rstd_error(a)
    return 0.0


def bounds_from(model_fig, extra=0.0):
    return {name: (1.5 * f[0] + extra, 1.5 * f[1] + extra, 2.0 * f[2] + extra) for name, f in model_fig.items()}


def judge(a, outs, ref, bnd, elem=None, what=""):
    """the failures of one launch's outputs: storage-dtype outputs against ``bnd`` (whole tensor, worst block, max-rel) and finite; fp32 outputs
    element by element against ``elem``.  -> (failures, figures)"""
    fig = figures(a, outs, ref)
    fails = []
    for name, f in fig.items():
        if not f[3]:
            fails.append(f"{what} {name}: not finite")
        if elem is not None and name in elem:
            over = torch.nan_to_num((outs[name].cpu().double() - ref[name]).abs() / elem[name], nan=math.inf)
            fig[name] = f + (float(over.max()),)
            if float(over.max()) > 1.0:
                at = [int(i) for i in torch.unravel_index(torch.argmax(over), tuple(over.shape))]
                fails.append(f"{what} {name}: element {at} is {float(over.max()):.3f} x its bound")
            continue
        for label, got, lim in zip(("rel-L2", "worst block", "max-rel"), f[:3], bnd[name]):
            if not got <= lim:
                fails.append(f"{what} {name}: {label} {got:.3e} > bound {lim:.3e} (block {f[4]})")
    return fails, fig


# ---- test operands ------------------------------------------------------------------------------------------------------------------------
def _gn(B, hw, c0, G, c1=0, **k):
    return dict(entry="groupnorm_coef" if k.pop("coef", False) else "groupnorm", B=B, hw=hw, c0=c0, c1=c1, groups=G, **k)


def _fp(B, hw, Cc, G, nblk, coef, **k):
    return dict(entry="from_partials", B=B, hw=hw, C=Cc, groups=G, nblk=nblk, coef=coef, **k)


def _ln(entry, rows, Cc, **k):
    return dict(entry=entry, rows=rows, C=Cc, **k)


# keywords: silu (1), eps (1e-5), gamma / beta (True), gamma_shift (elements in front of gamma: 4 = 8 bytes), mean (0.5), std (1.0) — generated
# before the rounding to the storage dtype —, const (item, group, value), R (|mean| / std, for the allowance rule)
GN_TWO_LAUNCH = {
    "1x300x320g32": _gn(1, 300, 320, 32),                                # ry 6: 16 idle threads; cpg 10 straddles chunks; remainder loop only
    "16x300x64g32": _gn(16, 300, 64, 32, silu=0, eps=1e-6),              # nblk 32, per 10: slabs 30 and 31 empty
    "3x1387x64g32": _gn(3, 1387, 64, 32),                                # nblk 170, per 9 < ry 32: idle rows, 15 empty slabs
    "1x9x24+16g4": _gn(1, 9, 24, 4, c1=16),                              # nblk 1, npart 1; group 2 crosses a chunk and the source boundary
    "1x264x8g1-nogamma": _gn(1, 264, 8, 1, gamma=False),                 # cx 1, ry 256 (at hw <= 256 one 8-channel group runs the small path)
    "1x40x8g2-nobeta": _gn(1, 40, 8, 2, beta=False, silu=0),             # cx 1, ry 256; 4 channels per group
    "1x264x2056g8": _gn(1, 264, 2056, 8),                                # column 0 uses a second chunk slot; per 8: prefetch + no remainder
    "1x257x8192g32": _gn(1, 257, 8192, 32, silu=0),                      # four slots, 64 KB LDS; per 9: two 4-pixel trips + remainder
    "1x675x1024g32": _gn(1, 675, 1024, 32),                              # ry 2, per 9: row 0 one trip + remainder, row 1 one trip
    "1x64x512g256": _gn(1, 64, 512, 256),                                # 8 trips of the statistics fold; cpg 2 refuses the small path
    "1x264x320g40": _gn(1, 264, 320, 40, eps=1e-6),                      # second trip with 8 of 32 lanes live
    "2x577x640g32-const": _gn(2, 577, 640, 32, const=(1, 5, 2.0)),       # variance exactly 0: out = act(beta)
    "2x64x512g32-gshift": _gn(2, 64, 512, 32, gamma_shift=4),            # a small map pushed onto the two-launch path by gamma's alignment
    "1x300x64g32-eps": _gn(1, 300, 64, 32, mean=0.0, std=2.0 ** -9),     # var 3.8e-6 against eps 1e-5
    "2x264x320g32-bare": _gn(2, 264, 320, 32, gamma=False, beta=False, silu=0),
    "1x64x272g34": _gn(1, 64, 272, 34),                                  # small plan refused: 17 groups per block
    "1x256x512g2": _gn(1, 256, 512, 2),                                  # small plan refused: 32 pixels per lane
    "1x16x2056g1": _gn(1, 16, 2056, 1, silu=0),                          # small plan refused: 257 chunk columns
    "coef-1x300x320g32": _gn(1, 300, 320, 32, coef=True),
    "coef-2x264x24+16g4": _gn(2, 264, 24, 4, c1=16, coef=True, gamma=False),
}
GN_OFFSET = {f"{hw}x{Cc}-R{R}": _gn(1, hw, Cc, 32, mean=16.0, std=16.0 / R, R=float(R)) for hw, Cc in ((1024, 320), (288, 2560)) for R in (4, 16, 64)}
GN_SMALL = {
    "2x64x512g32": _gn(2, 64, 512, 32),                                  # gpb 4, maxp 2: <3>
    "1x160x128g4": _gn(1, 160, 128, 4, silu=0),                          # gpb 2, maxp 5: <6>
    "1x256x320g4": _gn(1, 256, 320, 4),                                  # gpb 1, nc 10, npy 25 (6 idle threads), maxp 11: <12>; hw 256
    "1x256x1024g8": _gn(1, 256, 1024, 8),                                # maxp 16: <24>
    "3x250x64g8-nogamma": _gn(3, 250, 64, 8, gamma=False),               # gpb 8; the last pixel lane is ragged (250 = 7 x 32 + 26)
    "1x100x80g10": _gn(1, 100, 80, 10, eps=1e-6),                        # the loop ends with g == groups = 10
    "1x7x8g1": _gn(1, 7, 8, 1, silu=0),                                  # g == groups with one chunk column: npy 256
    "2x1x64g8": _gn(2, 1, 64, 8),                                        # hw 1: variance 0 per channel pair
    "1x64x40+24g4": _gn(1, 64, 40, 4, c1=24),                            # c0 inside the block's channels (and inside group 2)
    "coef-2x64x512g32": _gn(2, 64, 512, 32, coef=True),
    "1x256x320g4-m8": _gn(1, 256, 320, 4, mean=8.0, std=0.125, R=64.0),
    "2x250x64g8-m16": _gn(2, 250, 64, 8, mean=16.0, std=0.0625, R=256.0),
}
GN_PARTIALS = {
    "n1-coef": _fp(1, 40, 320, 32, 1, True),
    "n7-b2-apply": _fp(2, 400, 320, 32, 7, False),
    "n7-b2-coef": _fp(2, 400, 320, 32, 7, True, gamma=False),
    "n9-apply": _fp(1, 520, 64, 32, 9, False, silu=0),
    "n9-coef": _fp(1, 520, 64, 32, 9, True),
    "n70-apply": _fp(1, 4450, 64, 8, 70, False),
}
_LN_ROWS = {8: 33, 16: 17, 32: 9, 64: 5}
_LN_OPT = ((True, True), (True, False), (False, True), (False, False))


def _ln_cases():
    out = {}
    for i, Cc in enumerate((8, 64, 72, 200, 320, 328, 640, 648, 1280, 1288, 2048, 2056, 4096)):
        rows = _LN_ROWS[ln_instance(Cc)[0]]
        g, b = _LN_OPT[i % 4]
        pitch = (Cc + 8 * (1 + i % 3), Cc + 16) if i % 2 else None
        out[f"{rows}x{Cc}" + ("" if g else "-nogamma") + ("" if b else "-nobeta") + ("-pitch" if pitch else "")] = _ln("layernorm", rows, Cc, gamma=g, beta=b, pitch=pitch)
    out["1x640"] = _ln("layernorm", 1, 640)
    out["1x4096-pitch"] = _ln("layernorm", 1, 4096, pitch=(4104, 4104))
    out["17x320-m8-pitch"] = _ln("layernorm", 17, 320, mean=8.0, std=0.125, pitch=(328, 352))
    out["9x1280-m16"] = _ln("layernorm", 9, 1280, mean=16.0, std=0.0625)
    out["5x64-eps"] = _ln("layernorm", 5, 64, mean=0.0, std=2.0 ** -9, eps=1e-6)
    return out


def _lna_cases():
    out = {}
    for i, Cc in enumerate((8, 64, 72, 200, 320, 328, 640, 648, 1280)):
        rows = _LN_ROWS[ln_instance(Cc, add=True)[0]]
        pitch = (Cc + 8, Cc + 24, Cc + 16) if i % 2 == 0 else None
        out[f"{rows}x{Cc}" + ("-pitch" if pitch else "")] = _ln("layernorm_add", rows, Cc, pitch=pitch)
    out["1x1280"] = _ln("layernorm_add", 1, 1280)
    out["17x320-m8"] = _ln("layernorm_add", 17, 320, mean=8.0, std=0.125)
    out["9x648-m16-pitch"] = _ln("layernorm_add", 9, 648, mean=16.0, std=0.0625, pitch=(656, 648, 664))
    return out


LN_CASES, LNA_CASES = _ln_cases(), _lna_cases()
LN_STATS_CASES = {k: dict(v, entry="layernorm_stats") for k, v in LN_CASES.items()}
CASES = {"gn-two": GN_TWO_LAUNCH, "gn-offset": GN_OFFSET, "gn-small": GN_SMALL, "gn-partials": GN_PARTIALS, "ln": LN_CASES,
         "ln-stats": LN_STATS_CASES, "ln-add": LNA_CASES}
ALL = {f"{fam} {k}": v for fam, cs in CASES.items() for k, v in cs.items()}


def _seed(cid):
    fam = cid.split(" ")[0]
    fam = "ln" if fam == "ln-stats" else fam                                      # tg_layernorm_stats runs on tg_layernorm's rows
    return 1000 * list(CASES).index(fam) + list(CASES[fam]).index(cid.split(" ", 1)[1]) + 31


def fresh_outputs(a, device=None):
    """the launch with new NaN-filled outputs and scratch of the same layout (a guard row in front of and behind each)"""
    a = dict(a)
    e = a["entry"]
    dev = device or a[read_extents(a)[0].name].device
    dtype = storage_dtype(a)
    if e == "layernorm_stats":
        a["stats"] = bc._out((a["rows"], 2), torch.float32, 8, dev)
        return a
    if e in LN_ENTRIES:
        a["out"] = bc._out((a["rows"], a["ldo"]), dtype, a["ldo"], dev)[:, :a["C"]]
        return a
    B, hw, Cc, G = a["batch"], a["hw"], channels(a), a["groups"]
    if a.get("coef") is not None:
        a["coef"] = bc._out((B, 2, Cc), torch.float32, Cc, dev)
    else:
        a["out"] = bc._out((B * hw, Cc), dtype, Cc, dev)
    if e != "from_partials":
        a["partials"] = bc._out((gn_scratch_floats(B, hw, G),), torch.float32, 2 * G, dev)
    return a


def make_case(cid, dtype, device="cpu", spec=None, seed=None):
    """one launch: operands drawn on the CPU from the case's seed (the same bits on every device), each in a storage of its own between two NaN guard
    rows, pad columns NaN; outputs and the GroupNorm scratch (exactly tg_groupnorm_scratch_bytes) NaN-filled.  ``spec`` / ``seed``: a case that is
    not in ``ALL`` (the CPU test's R = 256 rows)"""
    k = dict(ALL[cid] if spec is None else spec)
    e = k["entry"]
    g = torch.Generator().manual_seed(_seed(cid) if seed is None else seed)
    rn = lambda *s: torch.randn(s, generator=g)
    mean, std = float(k.get("mean", 0.5)), float(k.get("std", 1.0))
    a = dict(entry=e, name=cid, eps=float(k.get("eps", 1e-5)), R=float(k.get("R", 0.0)), dtype=dtype, dtype_code=0 if dtype == torch.bfloat16 else 1)
    if e in LN_ENTRIES:
        rows, Cc = k["rows"], k["C"]
        pitch = k.get("pitch")
        x = (mean + std * rn(rows, Cc))
        a.update(rows=rows, C=Cc)
        if e == "layernorm_add":
            ldx, ldres, ldo = pitch or (Cc, Cc, Cc)
            r = 0.5 * std * rn(rows, Cc)
            a.update(x=bc._pitched(x.to(dtype), ldx, device)[:, :Cc], ldx=ldx, res=bc._pitched(r.to(dtype), ldres, device)[:, :Cc], ldres=ldres, ldo=ldo)
        else:
            ldx, ldo = pitch or (Cc, Cc)
            a.update(x=bc._pitched(x.to(dtype), ldx, device)[:, :Cc], ldx=ldx, ldo=ldo)
        ga, be = (1 + 0.2 * rn(Cc)).to(dtype), (0.5 * rn(Cc)).to(dtype)
        if e != "layernorm_stats":
            a["gamma"] = bc._guarded(ga, Cc, device) if k.get("gamma", True) else None
            a["beta"] = bc._guarded(be, Cc, device) if k.get("beta", True) else None
        return fresh_outputs(a, device)
    B, hw, G = k["B"], k["hw"], k["groups"]
    Cc = k["C"] if e == "from_partials" else k["c0"] + k["c1"]
    x = mean + std * rn(B, hw, Cc)
    x = x + 0.25 * std * rn(B, 1, G, 1).expand(B, 1, G, Cc // G).reshape(B, 1, Cc)      # the groups' and items' statistics differ
    if k.get("const") is not None:
        it, grp, val = k["const"]
        x.reshape(B, hw, G, Cc // G)[it, :, grp, :] = val
    x = x.to(dtype)
    ga, be = (1 + 0.2 * rn(Cc)).to(dtype), (0.3 * rn(Cc)).to(dtype)
    a.update(batch=B, hw=hw, groups=G, silu=int(k.get("silu", 1)))
    a["gamma"] = bc._guarded(ga, Cc, device, shift=int(k.get("gamma_shift", 0))) if k.get("gamma", True) else None
    a["beta"] = bc._guarded(be, Cc, device) if k.get("beta", True) else None
    if e == "from_partials":
        nblk = k["nblk"]
        assert _cdiv(hw, 64) == nblk != gn_nblk(B, hw), cid
        xp = torch.nn.functional.pad(x.double(), (0, 0, 0, nblk * 64 - hw)).reshape(B, nblk, 64, G, Cc // G)
        part = torch.stack([xp.sum((2, 4)), (xp * xp).sum((2, 4))], dim=-1).float()      # one fp32 rounding of the exact sum of every 64-pixel block
        a.update(C=Cc, nblk=nblk, partials=bc._guarded(part, 2 * G, device), x=None, coef=None, out=None)
        if k["coef"]:
            a["coef"] = True                                                            # replaced by the buffer below
            a["silu"] = 0
        else:
            a["x"] = bc._guarded(x, Cc, device)
        return fresh_outputs(a, device)
    c0, c1 = k["c0"], k["c1"]
    a.update(c0=c0, c1=c1, x0=bc._guarded(x[..., :c0].contiguous(), c0, device), x1=bc._guarded(x[..., c0:].contiguous(), c1, device) if c1 else None)
    a["coef" if e == "groupnorm_coef" else "out"] = True
    if e == "groupnorm_coef":
        a["silu"] = 0
    return fresh_outputs(a, device)


def item_launch(a, i):
    """batch item ``i`` (GroupNorm entries) or row ``i`` (LayerNorm entries) of ``a`` as a launch of its own: the same storages, new outputs and scratch"""
    b = dict(a)
    if a["entry"] in LN_ENTRIES:
        b.update(rows=1, x=a["x"][i:i + 1])
        if a.get("res") is not None:
            b["res"] = a["res"][i:i + 1]
    else:
        b["batch"] = 1
        for k in ("x0", "x1", "x", "partials") if a["entry"] == "from_partials" else ("x0", "x1"):
            if a.get(k) is not None:
                b[k] = a[k][i:i + 1]
    return fresh_outputs(b)


@functools.lru_cache(maxsize=None)
def case_data(cid, dname):
    """(launch on the CPU, fp64 reference, model outputs, model figures, bounds, per-element bounds or None) — computed once per (case, dtype) and
    shared; nobody writes into them"""
    a = make_case(cid, DTYPES[dname])
    ref = reference(a)
    mod = model(a)
    fig = figures(a, mod, ref)
    return a, ref, mod, fig, bounds_from(fig, extra_tolerance(a) if onepass_leaves_floor(a, fig, ref) else 0.0), fp32_bound(a)


def onepass_leaves_floor(a, model_fig, ref):
    """True when, on an R >= 64 two-launch case, the model's whole-tensor rel-L2 exceeds 1.5 x the floor (the fp64 result rounded once to the storage
    dtype): only then does the case get ``extra_tolerance``"""
    if extra_tolerance(a) == 0.0 or "out" not in ref:
        return False
    floor = figures(a, {"out": ref["out"].to(storage_dtype(a))}, ref)["out"][0]
    return model_fig["out"][0] > 1.5 * floor


def old_tolerance(dtype):
    """what tests/test_kernels_gpu.py allows test_groupnorm / test_layernorm"""
    return lc.l2_tol(dtype), lc.rel_tol(dtype)
