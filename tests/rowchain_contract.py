"""The C-ABI contracts of the row-chain kernels ``tg_rc_linear(_dup)``, ``tg_rc_kv_pack`` + ``tg_rc_xattn(_ps)`` and ``tg_rc_front``
(csrc/tg_rowchain.hip) restated in fp64 from include/theatergen_hip.h ("Row-chain kernels") and the reference lines it cites, for checking
single hand-made launches.  ``tg_rc_ff`` has its own fp64 test (tests/test_rc_ff2_gpu.py) and is not restated here.

    rc_linear   out[m, :] = [LayerNorm(x[m, :]; gamma, beta, eps)] W^T + bias (+ res[m, :])          (+ the same rows at out + c_dup_offset)
    rc_xattn    q = to_q(LayerNorm(h));  per head (8 x 40): O = softmax(s q Kt^T) Vt + w softmax(s q Kip^T) Vip  (two independent softmaxes over
                the 77 text keys and the T image keys, s = 40^-1/2, w = ip_scale[0], ip_scale[item] or 1);  out = to_out(O) + bias + h
                K [batch * 77, 320] / V^T [batch, 320, ldt] and image K [batch * T, 320] / V^T [batch, 320, ldi]: what tg_rc_kv_pack reads
    rc_front    X = x a[b] + d[b] (fp32 coef [batch][2][320]);  y = proj_in(X) + bias;  [q | k | v] = [to_q ; to_k ; to_v](LayerNorm1(y));
                outputs y [M, 320], qk [M, 640], vt[b, c, token]

  * ``*_reference(c, drop=())``: fp64 over the stored operands (storage dtype widened).  ``drop`` names contract clauses to leave out (``ABLATIONS``):
    never part of the contract, they show that a case exercises a clause (tests/test_rowchain_contract_cpu.py);
  * ``emulate(c, dtype)``: the same chain in fp32 on the CPU with a rounding to the storage dtype exactly where the kernels round (q, the probabilities,
    O, GroupNorm-applied rows, y, the outputs) and the fold ``rstd * (x W'^T - mean u) + v``: what a correct kernel can reach on the case;
  * ``blocks(entry, c)``: the row x column blocks one wave owns per weight chunk; ``figures`` / ``bounds`` / ``judge``: the assertions of the GPU edge test;
  * ``CASES`` / ``make_case``: the launches of tests/test_rowchain_edges_gpu.py, drawn on the CPU from a seed.

Bounds (none tuned on a kernel): per case and dtype 1.5 x the emulation's rel-L2 for the whole tensor and for the worst block, 2 x for max|err| / max|ref|.
The device rounds the same quantities at the same places, sums in another order and uses the hardware exp2 / rsq / rcp: an independent rounding set of the
same size would add sqrt(2).
"""
import functools
import math

import torch

C, HEADS, DH, TEXT = 320, 8, 40, 77
LOG2E = math.log2(math.e)
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
ABLATIONS = ("ln_eps", "ln_beta", "bias", "residual", "key_pad", "two_softmax", "ip_scale", "item", "gn_coef", "vt_transpose")
CLAUSES = {"rc_linear": ("ln_eps", "ln_beta", "bias", "residual"),
           "rc_xattn": ("ln_eps", "ln_beta", "bias", "residual", "key_pad", "two_softmax", "ip_scale", "item"),
           "rc_front": ("ln_eps", "ln_beta", "bias", "item", "gn_coef", "vt_transpose")}
# what tests/test_rowchain_gpu.py allows (rel-L2, max|err| / max|ref|): the new bounds of the non-peaked cases never exceed these
OLD_TOLS = {"bf16": (3e-3, 1e-2), "fp16": (4e-4, 2.5e-3)}


# ---- case tables ------------------------------------------------------------------------------------------------------------------------
# rc_linear: 256-token workgroups (8 waves x 32).  M 1 / 31: one partly filled wave, seven empty; 255 / 256 / 257: the workgroup edge; 2050: 9 workgroups (uneven
# split over the 8 XCDs), the last one holds 2 rows.  N 64: one chunk (prologue DMA only, trailing store only).  pitch: (ldx, ldres - N, ldc - N) or None = dense.
# ln: None or (eps, row mean, row std) — mean / std generated BEFORE the rounding to the storage dtype.  eps 1e-3 against std 0.0625: the eps clause carries weight.
def _lin(M, N, res=False, ln=None, dup=False, pitch=None):
    return dict(entry="rc_linear", M=M, N=N, res=res, ln=ln, dup=dup, pitch=pitch)


_LN = (1e-5, 0.3, 1.5)
LINEAR_CASES = {
    "m1_n64": _lin(1, 64),
    "m31_n128_res_pitch": _lin(31, 128, res=True, pitch=(352, 8, 64)),
    "m33_n64_ln": _lin(33, 64, ln=_LN),
    "m255_n320_res_ln_pitch": _lin(255, 320, res=True, ln=_LN, pitch=(352, 8, 64)),
    "m256_n128": _lin(256, 128),
    "m257_n320_ln_pitch": _lin(257, 320, ln=_LN, pitch=(328, 8, 32)),
    "m2050_n960_res": _lin(2050, 960, res=True),
    "m2050_n320_res_ln_pitch": _lin(2050, 320, res=True, ln=_LN, pitch=(352, 8, 64)),
    "m257_n128_res_dup": _lin(257, 128, res=True, dup=True),
    "m1000_n320_ln_dup_pitch": _lin(1000, 320, ln=_LN, dup=True, pitch=(352, 8, 64)),
    "m256_n320_ln_mean8": _lin(256, 320, ln=(1e-5, 8.0, 0.125)),
    "m257_n64_res_ln_mean16_pitch": _lin(257, 64, res=True, ln=(1e-3, 16.0, 0.0625), pitch=(352, 8, 64)),
}


# rc_xattn: 128-token workgroups.  ips: None (NULL = 1), a float (one device scalar) or "item" (one per batch item, including 0 and a negative one).
# peaked: to_q x 6 (score standard deviation ~ 6: a few keys carry a row).  pitch: (ldh, ldc, ldt, ldi) or None = (320, 320, 80, 8 or 16).
def _xa(B, rows, T, ips, peaked=False, pitch=None, eps=1e-5):
    return dict(entry="rc_xattn", B=B, rows=rows, T=T, ips=ips, peaked=peaked, pitch=pitch, eps=eps)


XATTN_CASES = {
    "b1_r128_t0": _xa(1, 128, 0, None),
    "b3_r128_t4_s04_pitch": _xa(3, 128, 4, 0.4, pitch=(352, 384, 80, 8)),
    "b17_r128_t16_item": _xa(17, 128, 16, "item"),
    "b1_r2176_t4_null": _xa(1, 2176, 4, None),
    "b2_r384_t16_s0_bigpitch": _xa(2, 384, 16, 0.0, pitch=(384, 328, 96, 24)),
    "b3_r128_t4_item_pitch": _xa(3, 128, 4, "item", pitch=(328, 352, 88, 16)),
    "b2_r384_t0_peaked": _xa(2, 384, 0, None, peaked=True, eps=1.0),
    "b3_r128_t16_peaked_item": _xa(3, 128, 16, "item", peaked=True, eps=1.0),
}


# rc_front: pitch (ldx, ldy, ldqk, ldt - rows) or None = dense.  Every case runs with the device's tg_groupnorm_coef output and with coef from fp64 statistics.
def _fr(B, rows, pitch=None, eps=1e-5):
    return dict(entry="rc_front", B=B, rows=rows, pitch=pitch, eps=eps)


FRONT_CASES = {
    "b1_r128": _fr(1, 128),
    "b3_r128_pitch": _fr(3, 128, pitch=(352, 328, 704, 24), eps=0.5),
    "b17_r128": _fr(17, 128),
    "b1_r2176": _fr(1, 2176),
}
CASES = {"rc_linear": LINEAR_CASES, "rc_xattn": XATTN_CASES, "rc_front": FRONT_CASES}
GN_GROUPS, GN_EPS = 32, 1e-6


def claims(entry, c):
    """the clauses a case says it exercises (the CPU test holds it to that: each moves the reference by >= 4 x the case's bound)"""
    if entry == "rc_linear":
        out = ["bias"] if not c["ln"] or c["ln"][1] < 4 else []          # (high-mean rows: the output is dominated by the residual / LayerNorm term)
        if c["res"]:
            out.append("residual")
        if c["ln"]:
            out.append("ln_beta")
            if c["ln"][0] >= 1e-3:
                out.append("ln_eps")
        return out
    if entry == "rc_xattn":
        out = ["bias", "residual", "ln_beta"]
        scales = ip_scales(c)
        live = c["T"] > 0 and scales is not None and float(scales.abs().max()) >= 0.4
        if c["eps"] >= 0.5:
            out.append("ln_eps")
        if c["T"] == 4 and (scales is None or live):
            out.append("key_pad")
        if c["T"] > 0 and (scales is None or live):
            out.append("two_softmax")
        if c["T"] > 0 and scales is not None:
            out.append("ip_scale")
        if c["B"] > 1:
            out.append("item")
        return out
    out = ["bias", "ln_beta", "gn_coef", "vt_transpose"]
    if c["eps"] >= 0.1:
        out.append("ln_eps")
    if c["B"] > 1:
        out.append("item")
    return out


def ip_scales(c):
    """the fp32 IP scales of an rc_xattn case: None (NULL), [1] or [B]"""
    if c["ips"] is None:
        return None
    if c["ips"] == "item":
        base = torch.tensor([0.4, 0.0, -0.7, 1.3, 0.25], dtype=torch.float32)
        return base[torch.arange(c["B"]) % 5].contiguous()
    return torch.tensor([float(c["ips"])], dtype=torch.float32)


def _seed(entry, name):
    return 1000 * list(CASES).index(entry) + list(CASES[entry]).index(name) + 17


def make_case(entry, name, dtype):
    """the case's dense operands on the CPU in the storage dtype (fp32: coef, IP scales); the GPU test lays them into NaN-filled pitched buffers"""
    c = dict(CASES[entry][name])
    c["name"], c["dtype"] = name, dtype
    g = torch.Generator().manual_seed(_seed(entry, name))
    rn = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    st = lambda t: t.to(dtype)
    if entry == "rc_linear":
        M, N = c["M"], c["N"]
        if c["ln"]:
            _, mean, std = c["ln"]
            c["x"] = st(rn(M, C, sc=std) + mean)
            c["gamma"], c["beta"] = st(1 + 0.2 * rn(C)), st(rn(C, sc=0.5))
        else:
            c["x"] = st(rn(M, C, sc=1.5) + 0.3)
        c["W"], c["bias"] = st(rn(N, C, sc=C ** -0.5)), st(rn(N))
        if c["res"]:
            c["resid"] = st(rn(M, N))
        c["eps"] = c["ln"][0] if c["ln"] else None
        return c
    if entry == "rc_xattn":
        B, T = c["B"], c["T"]
        M = B * c["rows"]
        c["M"] = M
        c["h"] = st(rn(M, C, sc=1.2) + 0.2)
        c["wq"] = st(rn(C, C, sc=C ** -0.5) * (6.0 if c["peaked"] else 1.0))
        c["wo"], c["bo"] = st(rn(C, C, sc=C ** -0.5)), st(rn(C, sc=0.5))
        c["gamma"], c["beta"] = st(1 + 0.2 * rn(C)), st(rn(C, sc=0.5))
        c["k"], c["v"] = st(rn(B * TEXT, C)), st(rn(B, TEXT, C))
        if T:
            c["kip"], c["vip"] = st(rn(B * T, C)), st(rn(B, T, C, sc=0.5))
        c["scales"] = ip_scales(c)
        return c
    B = c["B"]
    M = B * c["rows"]
    c["M"] = M
    item_shift = rn(B, 1, C, sc=0.5).expand(B, c["rows"], C).reshape(M, C)       # the items' statistics differ: another item's coef is a visible fault
    c["x"] = st(rn(M, C, sc=1.3) + 0.4 + item_shift)
    c["gn_gamma"], c["gn_beta"] = st(1 + 0.2 * rn(C)), st(rn(C, sc=0.3))
    c["win"], c["bin"] = st(rn(C, C, sc=C ** -0.5)), st(rn(C, sc=0.5))
    c["wqkv"] = st(rn(3 * C, C, sc=C ** -0.5))
    c["gamma"], c["beta"] = st(1 + 0.2 * rn(C)), st(rn(C, sc=0.5))
    c["coef"] = groupnorm_coef_fp64(c).float()
    return c


def groupnorm_coef_fp64(c):
    """tg_groupnorm_coef in fp64: a = rstd gamma, d = beta - mean a per (item, channel), groups of 10 channels over the item's tokens -> [B, 2, 320]"""
    B, rows = c["B"], c["rows"]
    x = c["x"].double().reshape(B, rows, GN_GROUPS, C // GN_GROUPS)
    mean = x.mean(dim=(1, 3))
    var = ((x - mean[:, None, :, None]) ** 2).mean(dim=(1, 3))
    rstd = (var + GN_EPS) ** -0.5
    rep = lambda t: t.repeat_interleave(C // GN_GROUPS, dim=1)
    a = rep(rstd) * c["gn_gamma"].double()[None]
    d = c["gn_beta"].double()[None] - rep(mean) * a
    return torch.stack([a, d], dim=1)


# ---- fp64 references --------------------------------------------------------------------------------------------------------------------
def _layer_norm(x, gamma, beta, eps, drop):
    mean = x.mean(dim=1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=1, keepdim=True)
    xn = (x - mean) / torch.sqrt(var + (0.0 if "ln_eps" in drop else eps)) * gamma
    return xn if "ln_beta" in drop else xn + beta


def rc_linear_reference(c, drop=()):
    """{"out": [M, N]}: plain, + residual, LayerNorm in front; the second destination holds the same rows"""
    d = lambda k: c[k].double()
    x = d("x")
    if c["ln"]:
        x = _layer_norm(x, d("gamma"), d("beta"), c["eps"], drop)
    out = x @ d("W").T
    if "bias" not in drop:
        out = out + d("bias")
    if c["res"] and "residual" not in drop:
        out = out + d("resid")
    return {"out": out}


def _softmax_rows(s):
    e = torch.exp(s - s.max(dim=-1, keepdim=True).values)
    return e / e.sum(dim=-1, keepdim=True)


def rc_xattn_reference(c, drop=()):
    """{"out": [M, 320]} from h, to_q, LayerNorm, K [B * 77, 320] / V [B, 77, 320] (the kernel is handed V^T [B, 320, ldt]) and the image keys"""
    d = lambda k: c[k].double()
    B, rows, T, M = c["B"], c["rows"], c["T"], c["M"]
    h = d("h")
    q = (_layer_norm(h, d("gamma"), d("beta"), c["eps"], drop) @ d("wq").T).reshape(B, rows, HEADS, DH).permute(0, 2, 1, 3)
    heads = lambda t, L: t.reshape(B, L, HEADS, DH).permute(0, 2, 1, 3)
    kt, vt = heads(d("k"), TEXT), heads(d("v"), TEXT)
    ki = vi = None
    if T:
        ki, vi = heads(d("kip"), T), heads(d("vip"), T)
    w = torch.ones(B, dtype=torch.float64)
    if T and c["scales"] is not None and "ip_scale" not in drop:
        w = c["scales"].double().expand(B).clone()
    if "item" in drop:
        kt, vt = kt[:1].expand_as(kt), vt[:1].expand_as(vt)
        if T:
            ki, vi = ki[:1].expand_as(ki), vi[:1].expand_as(vi)
        w = w[:1].expand(B)
    if "key_pad" in drop:
        # the pad slots of the fragment layout (3 behind the 77 text keys, 16 - T behind the image keys) take part with score 0 and V = 0
        z = lambda t, n: torch.cat([t, torch.zeros(B, HEADS, n, DH, dtype=torch.float64)], dim=2)
        kt, vt = z(kt, 3), z(vt, 3)
        if T:
            ki, vi = z(ki, 16 - T), z(vi, 16 - T)
    scale = DH ** -0.5
    st = q @ kt.transpose(-1, -2) * scale
    if T and "two_softmax" in drop:
        p = _softmax_rows(torch.cat([st, q @ ki.transpose(-1, -2) * scale], dim=-1))
        o = p[..., :kt.shape[2]] @ vt + w[:, None, None, None] * (p[..., kt.shape[2]:] @ vi)
    else:
        o = _softmax_rows(st) @ vt
        if T:
            o = o + w[:, None, None, None] * (_softmax_rows(q @ ki.transpose(-1, -2) * scale) @ vi)
    out = o.permute(0, 2, 1, 3).reshape(M, C) @ d("wo").T
    if "bias" not in drop:
        out = out + d("bo")
    if "residual" not in drop:
        out = out + h
    return {"out": out}


def rc_front_reference(c, drop=(), coef=None):
    """{"y": [M, 320], "qk": [M, 640], "vt": [B, 320, rows]}; ``coef``: the fp32 [B, 2, 320] tensor the launch was handed (default: the case's own)"""
    d = lambda k: c[k].double()
    B, rows, M = c["B"], c["rows"], c["M"]
    cf = (c["coef"] if coef is None else coef).double()
    if "item" in drop:
        cf = cf[:1].expand(B, 2, C)
    x = d("x").reshape(B, rows, C)
    if "gn_coef" not in drop:
        x = x * cf[:, 0][:, None, :] + cf[:, 1][:, None, :]
    y = x.reshape(M, C) @ d("win").T
    if "bias" not in drop:
        y = y + d("bin")
    qkv = _layer_norm(y, d("gamma"), d("beta"), c["eps"], drop) @ d("wqkv").T
    v = qkv[:, 2 * C:].reshape(B, rows, C)
    vt = v.reshape(B, C, rows) if "vt_transpose" in drop else v.transpose(1, 2)
    return {"y": y, "qk": qkv[:, :2 * C], "vt": vt.contiguous()}


REFERENCES = {"rc_linear": rc_linear_reference, "rc_xattn": rc_xattn_reference, "rc_front": rc_front_reference}


def reference(c, drop=(), **kw):
    return REFERENCES[c["entry"]](c, drop, **kw)


# ---- fp32 emulation of the kernels' arithmetic ----------------------------------------------------------------------------------------------
def xattn_q_fold(c):
    """W', u, v of ``rowchain.pack_xattn_q`` in natural channel order (the packer permutes the rows of exactly these)"""
    s = DH ** -0.5 * LOG2E
    w32 = c["wq"].float()
    wp = (w32 * c["gamma"].float()[None, :] * s).to(c["dtype"])
    return wp, wp.float().sum(dim=1), (w32 @ c["beta"].float()) * s


def _fold_stats(x32, eps):
    """the kernels' two-pass row statistics: (-mean, std, rstd) with std = var * rstd"""
    mean = x32.mean(dim=1, keepdim=True)
    var = ((x32 - mean) ** 2).mean(dim=1, keepdim=True) + eps
    rstd = var ** -0.5
    return -mean, var * rstd, rstd


def _folded(x32, wp, u, v, eps):
    nmean, std, rstd = _fold_stats(x32, eps)
    return (std * v[None, :] + nmean * u[None, :] + x32 @ wp.float().T) * rstd


def emulate(c, dtype=None, coef=None):
    """the case's outputs as a correct kernel computes them: fp32 sums, one rounding to the storage dtype at every place the device rounds"""
    from theatergen_amd.weights_pack import pack_ln_linear
    dtype = c["dtype"] if dtype is None else dtype
    r = lambda t: t.to(dtype).float()
    f = lambda k: c[k].float()
    entry = c["entry"]
    if entry == "rc_linear":
        if c["ln"]:
            wp, u, v = pack_ln_linear(c["W"], c["bias"], c["gamma"], c["beta"])
            o = _folded(f("x"), wp, u, v, c["eps"])
        else:
            o = f("x") @ f("W").T + f("bias")[None, :]
        if c["res"]:
            o = o + f("resid")
        return {"out": o.to(dtype)}
    if entry == "rc_xattn":
        B, rows, T, M = c["B"], c["rows"], c["T"], c["M"]
        wp, u, v = xattn_q_fold(c)
        q = r(_folded(f("h"), wp, u, v, c["eps"])).reshape(B, rows, HEADS, DH).permute(0, 2, 1, 3)      # log2 domain: scale * log2(e) is in W'
        heads = lambda t, L: t.float().reshape(B, L, HEADS, DH).permute(0, 2, 1, 3)
        s = q @ heads(c["k"], TEXT).transpose(-1, -2)
        p = r(torch.exp2(s - s.max(dim=-1, keepdim=True).values))                                  # unnormalised, rounded: the PV operand
        o = (p @ heads(c["v"], TEXT)) * (1.0 / p.sum(dim=-1, keepdim=True))                        # the denominator sums the ROUNDED probabilities
        if T:
            w = torch.ones(B) if c["scales"] is None else c["scales"].expand(B)
            si = q @ heads(c["kip"], T).transpose(-1, -2)
            e = torch.exp2(si - si.max(dim=-1, keepdim=True).values)
            pi = r(e * (w[:, None, None, None] * (1.0 / e.sum(dim=-1, keepdim=True))))            # normalised and weighted, then rounded
            o = o + pi @ heads(c["vip"], T)
        o = r(o).permute(0, 2, 1, 3).reshape(M, C)
        return {"out": (o @ f("wo").T + f("bo")[None, :] + f("h")).to(dtype)}
    B, rows, M = c["B"], c["rows"], c["M"]
    cf = (c["coef"] if coef is None else coef).float()
    x = r(torch.addcmul(cf[:, 1][:, None, :], f("x").reshape(B, rows, C), cf[:, 0][:, None, :])).reshape(M, C)   # fma(x, a, d), one rounding
    y = r(x @ f("win").T + f("bin")[None, :])
    wp, u, v = pack_ln_linear(c["wqkv"], None, c["gamma"], c["beta"])
    qkv = _folded(y, wp, u, v, c["eps"]).to(dtype)
    return {"y": y.to(dtype), "qk": qkv[:, :2 * C].contiguous(), "vt": qkv[:, 2 * C:].reshape(B, rows, C).transpose(1, 2).contiguous()}


# ---- blocks, figures, bounds, judgement -------------------------------------------------------------------------------------------------------
def blocks(entry, c):
    """{output: [index tuple, ...]}: the block one wave owns per weight chunk — 32 tokens x 64 channels of a token-major output, 32 tokens x 32 channels
    (one MFMA tile) of V^T [b, c, token]"""
    M = c["M"]
    rows = [slice(r0, min(r0 + 32, M)) for r0 in range(0, M, 32)]
    tm = lambda n: [(rs, slice(c0, c0 + 64)) for rs in rows for c0 in range(0, n, 64)]
    if entry == "rc_linear":
        return {"out": tm(c["N"])}
    if entry == "rc_xattn":
        return {"out": tm(C)}
    rpb = c["rows"]
    vt = [(b, slice(c0, c0 + 32), slice(t0, t0 + 32)) for b in range(c["B"]) for t0 in range(0, rpb, 32) for c0 in range(0, C, 32)]
    return {"y": tm(C), "qk": tm(2 * C), "vt": vt}


def figures(entry, c, outs, ref):
    """{output: (rel-L2, worst block rel-L2, max|err| / max|ref|)} of ``outs`` (storage dtype, shaped like the written regions) against ``ref`` (fp64)"""
    fig = {}
    blk = blocks(entry, c)
    for name, want in ref.items():
        got = outs[name].double()
        assert got.shape == want.shape, (name, got.shape, want.shape)
        err2, ref2 = (got - want) ** 2, want ** 2
        worst = max(math.sqrt(float(err2[ix].sum()) / max(float(ref2[ix].sum()), 1e-300)) for ix in blk[name])
        fig[name] = (math.sqrt(float(err2.sum()) / float(ref2.sum())), worst, float((got - want).abs().max() / want.abs().max()))
    return fig


def bounds_from(emu_fig):
    return {name: (1.5 * l2, 1.5 * wb, 2.0 * mx) for name, (l2, wb, mx) in emu_fig.items()}


@functools.lru_cache(maxsize=None)
def case_data(entry, name, dname):
    """(case, fp64 reference, emulation figures, bounds) — computed once per (case, dtype) and shared; nobody writes into them"""
    c = make_case(entry, name, DTYPES[dname])
    ref = reference(c)
    emu = figures(entry, c, emulate(c), ref)
    return c, ref, emu, bounds_from(emu)


def judge(entry, c, outs, ref, bnd, what=""):
    """the failures of one launch's outputs against the fp64 reference: whole tensor, worst block, max-rel; and the figures"""
    fig = figures(entry, c, outs, ref)
    fails = []
    for name, f in fig.items():
        for label, got, lim in zip(("rel-L2", "worst block", "max-rel"), f, bnd[name]):
            if not got <= lim:
                fails.append(f"{what} {name}: {label} {got:.3e} > bound {lim:.3e}")
    return fails, fig


def old_tolerance(entry, c, dname, name="out"):
    """what tests/test_rowchain_gpu.py allows for this kind of launch: x 1.5 for rc_linear behind a LayerNorm and for rc_front's y, x 2 for its qk / V^T"""
    l2, mx = OLD_TOLS[dname]
    k = 1.0
    if entry == "rc_linear" and c["ln"]:
        k = 1.5
    if entry == "rc_front":
        k = 1.5 if name == "y" else 2.0
    return k * l2, k * mx
