"""GPU: single hand-made launches of ``tg_rc_linear(_dup)``, ``tg_rc_kv_pack`` + ``tg_rc_xattn(_ps)`` and ``tg_rc_front`` (csrc/tg_rowchain.hip) against the
fp64 restatement of their C-ABI contracts (tests/rowchain_contract.py), at the smallest shapes at which each kernel can still go wrong.

Per case and dtype: every input element the contract does not read holds NaN (pad columns, V^T columns behind the keys); every output storage is NaN before
the launch, every element of the written region is finite afterwards and every other element (pad columns, guard rows, the gap between the two destinations
of ``_dup``, V^T columns >= rows_per_batch) still NaN; the outputs are judged against fp64 for the whole tensor, for every block one wave owns and at
max|err| / max|ref|; a second launch gives the same bits; a batch item launched alone reproduces its rows of the batched launch bit for bit.

Bounds: 1.5 x (whole tensor, worst block) and 2 x (max-rel) what the fp32 emulation of the kernels' arithmetic reaches ON THE SAME CASE, computed in the test
from the operands.  Measured on MI355X (profiles/rowchain_contract_findings.md has every case): the device's rel-L2 is 0.997 .. 1.0005 x the emulation's on
every case, its worst block 0.996 .. 1.017 x, its max-rel the emulation's to the last digit; the peaked (score deviation ~ 6: 3.0e-3 bf16, 3.8e-4 fp16) and
|mean| >> std cases are no exception.  Worst device / bound: 0.68 (rc_linear m257_n64_res_ln_mean16_pitch bf16, worst block 1.939e-3 against 1.5 x 1.906e-3).
The whole file takes 4 s.
"""
import ctypes as C
import functools

import pytest
import torch

from tests import rowchain_contract as rc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 3                      # guard rows behind the last row of an output storage
NAN = float("nan")
ERR_ARG = -1                   # TG_ERR_ARG
FIGURES = {}                   # (entry, case, dtype, variant) -> {output: (rel-L2, worst block, max-rel)} of the device, for the findings table


class Storage:
    """a NaN-filled device storage and the mask of the elements a launch may write"""

    def __init__(self, numel, dtype):
        self.buf = torch.full((numel,), NAN, dtype=dtype, device=DEV)
        self.mask = torch.zeros(numel, dtype=torch.bool, device=DEV)

    def view(self, offset, size, stride):
        self.mask.as_strided(size, stride, offset).fill_(True)
        return self.buf.as_strided(size, stride, offset)

    def failures(self, what):
        torch.cuda.synchronize()
        out = []
        if not bool(torch.isfinite(self.buf[self.mask]).all()):
            out.append(f"{what}: {int((~torch.isfinite(self.buf[self.mask])).sum())} elements of the written region are not finite")
        if not bool(torch.isnan(self.buf[~self.mask]).all()):
            out.append(f"{what}: {int((~torch.isnan(self.buf[~self.mask])).sum())} elements outside the written region were written")
        return out


def rows_out(M, N, ld, dtype):
    st = Storage((M + GUARD) * ld, dtype)
    return st, st.view(0, (M, N), (ld, 1))


def pitched(t, ld):
    """the rows of ``t`` [..., w] on the device at row pitch ``ld``; the pad columns hold NaN"""
    buf = torch.full(t.shape[:-1] + (ld,), NAN, dtype=t.dtype, device=DEV)
    buf[..., :t.shape[-1]] = t.to(DEV)
    return buf[..., :t.shape[-1]]


def bits(t):
    return t.contiguous().view(torch.int16)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


# ---- rc_linear --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def linear_operands(name, dname):
    from theatergen_amd.weights_pack import pack_ln_linear, rc_pack
    c = rc.case_data("rc_linear", name, dname)[0]
    N = c["N"]
    ldx, dres, dc = c["pitch"] or (rc.C, 0, 0)
    dev = lambda k: c[k].to(DEV)
    if c["ln"]:
        wp, u, v = pack_ln_linear(dev("W"), dev("bias"), dev("gamma"), dev("beta"))
        wpk = rc_pack(wp, v, u)
    else:
        wpk = rc_pack(dev("W"), dev("bias").float())
    return dict(x=pitched(c["x"], ldx), res=pitched(c["resid"], N + dres) if c["res"] else None, wpk=wpk, ldc=N + dc)


def launch_linear(c, dname, mode="plain"):
    """one launch; mode "plain", "pair" (``ops.rc_linear(pair_out=)``, dense) or "gap" (``tg_rc_linear_dup`` with room between the destinations).
    Returns ([destination views], storage)"""
    from theatergen_amd import _lib, ops
    o = linear_operands(c["name"], dname)
    M, N, ldc = c["M"], c["N"], o["ldc"]
    if mode == "plain":
        st, out = rows_out(M, N, ldc, c["dtype"])
        ops.rc_linear(o["x"], o["wpk"], N, res=o["res"], ln_eps=c["eps"], out=out)
        return [out], st
    if mode == "pair":
        st, pair = rows_out(2 * M, N, N, c["dtype"])
        ops.rc_linear(o["x"], o["wpk"], N, res=o["res"], ln_eps=c["eps"], pair_out=pair)
        return [pair[:M], pair[M:]], st
    dup = M * ldc + 64                                        # pad columns of the last row + 64 elements lie between the destinations
    st = Storage(dup + (M + GUARD) * ldc, c["dtype"])
    d0, d1 = st.view(0, (M, N), (ldc, 1)), st.view(dup, (M, N), (ldc, 1))
    d = _lib.RcLinearDesc()
    d.dtype, d.x, d.ldx, d.wpk = ops._dt(o["x"]), o["x"].data_ptr(), o["x"].stride(0), o["wpk"].data_ptr()
    d.res, d.ldres = (o["res"].data_ptr(), o["res"].stride(0)) if o["res"] is not None else (None, 0)
    d.out, d.ldc, d.M, d.N, d.K = d0.data_ptr(), ldc, M, N, rc.C
    d.ln, d.ln_eps = (1, c["eps"]) if c["ln"] else (0, 0.0)
    _lib.check(_lib.lib().tg_rc_linear_dup(C.byref(d), dup, ops._stream()))
    return [d0, d1], st


def run_linear(name, dname):
    c, ref, emu, bnd = rc.case_data("rc_linear", name, dname)
    what = f"rc_linear {name} {dname}"
    (out,), st = launch_linear(c, dname)
    fails = st.failures(what)
    f2, fig = rc.judge("rc_linear", c, {"out": out.cpu()}, ref, bnd, what)
    report("rc_linear", name, dname, "", fig, emu, bnd)
    (again,), st2 = launch_linear(c, dname)
    fails += f2 + st2.failures(what + " (second launch)")
    if not same_bits(out, again):
        fails.append(f"{what}: a second launch gave other bits")
    if c["dup"]:
        mode = "gap" if c["pitch"] else "pair"
        (d0, d1), st3 = launch_linear(c, dname, mode)
        fails += st3.failures(f"{what} ({mode})")
        if not (same_bits(d0, d1) and same_bits(d0, out)):
            fails.append(f"{what} ({mode}): the two destinations and the plain launch do not hold the same bits")
    return fails


# ---- rc_xattn ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def xattn_operands(name, dname):
    from theatergen_amd import rowchain
    c = rc.case_data("rc_xattn", name, dname)[0]
    B, T = c["B"], c["T"]
    ldh, ldc, ldt, ldi = c["pitch"] or (rc.C, rc.C, 80, 16 if T == 16 else 8)
    dev = lambda k: c[k].to(DEV)
    o = dict(h=pitched(c["h"], ldh), ldc=ldc, ldt=ldt, ldi=ldi, k=dev("k"), vt=pitched(c["v"].transpose(1, 2), ldt), kip=None, vtip=None,
             wq=rowchain.pack_xattn_q(dev("wq"), None, dev("gamma"), dev("beta"), rc.DH ** -0.5), wo=rowchain.pack_xattn_out(dev("wo"), dev("bo")),
             scales=c["scales"].to(DEV) if c["scales"] is not None else None)
    if T:
        o["kip"], o["vtip"] = dev("kip"), pitched(c["vip"].transpose(1, 2), ldi)
    return o


def launch_xattn(c, dname, T=None, scales="case", item=None, kv=None):
    """tg_rc_kv_pack + tg_rc_xattn on the case's operands; ``T`` = 0: the text keys alone; ``item``: that batch item alone.  Returns (out view, [storages])"""
    from theatergen_amd import ops
    o = xattn_operands(c["name"], dname)
    B, rows = c["B"], c["rows"]
    T = c["T"] if T is None else T
    sc = o["scales"] if isinstance(scales, str) else scales
    sts = []
    if kv is None:
        sts.append(Storage(B * 8 * 24 * 512 + 512, c["dtype"]))
        kv = ops.rc_kv_pack(o["k"], o["vt"], o["ldt"], rc.TEXT, o["kip"] if T else None, o["vtip"] if T else None, o["ldi"] if T else 0, T, B,
                            out=sts[0].view(0, (B, 8, 24 * 512), (8 * 24 * 512, 24 * 512, 1)))
    h = o["h"]
    if item is not None:
        h, kv, B = h[item * rows:(item + 1) * rows], kv[item:item + 1], 1
        if sc is not None and sc.numel() > 1:
            sc = sc[item:item + 1]
    st, out = rows_out(B * rows, rc.C, o["ldc"], c["dtype"])
    ops.rc_xattn(h, o["wq"], kv, o["wo"], rows, c["eps"], T, ip_scale=sc if T else None, out=out)
    return out, [st] + sts, kv


def run_xattn(name, dname):
    c, ref, emu, bnd = rc.case_data("rc_xattn", name, dname)
    what = f"rc_xattn {name} {dname}"
    B, rows, T = c["B"], c["rows"], c["T"]
    out, sts, kv = launch_xattn(c, dname)
    fails = [f for st in sts for f in st.failures(what)]
    f2, fig = rc.judge("rc_xattn", c, {"out": out.cpu()}, ref, bnd, what)
    report("rc_xattn", name, dname, "", fig, emu, bnd)
    again, sts2, kv2 = launch_xattn(c, dname)
    fails += f2 + [f for st in sts2 for f in st.failures(what + " (second launch)")]
    if not (same_bits(out, again) and same_bits(kv, kv2)):
        fails.append(f"{what}: a second launch gave other bits")
    for b in (sorted({0, B // 2, B - 1}) if B > 1 else []):
        one, sts3, _ = launch_xattn(c, dname, item=b, kv=kv)
        fails += [f for f in sts3[0].failures(f"{what} (item {b} alone)")]
        if not same_bits(one, out[b * rows:(b + 1) * rows]):
            fails.append(f"{what}: item {b} launched alone differs from its rows of the batched launch")
    sc = c["scales"]
    if T and sc is not None and sc.numel() == 1:
        every = launch_xattn(c, dname, scales=sc.to(DEV).expand(B).contiguous())[0]        # one float per item, all equal: tg_rc_xattn_ps
        if B > 1 and not same_bits(every, out):
            fails.append(f"{what}: per-item scales that are all equal differ from the scalar launch")
        if float(sc) == 0.0:
            text, sts4, _ = launch_xattn(c, dname, T=0)                                    # scale 0 = no image branch: the T = 0 kernel, same reference
            f4, fig4 = rc.judge("rc_xattn", c, {"out": text.cpu()}, ref, bnd, what + " (T = 0 launch)")
            report("rc_xattn", name, dname, "T0", fig4, emu, bnd)
            fails += f4 + [f for st in sts4 for f in st.failures(what + " (T = 0 launch)")]
    return fails


# ---- rc_front ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def front_operands(name, dname):
    from theatergen_amd import ops
    from theatergen_amd.weights_pack import pack_ln_linear, rc_pack_tiles
    c = rc.case_data("rc_front", name, dname)[0]
    ldx, ldy, ldqk, dt_ = c["pitch"] or (rc.C, rc.C, 2 * rc.C, 0)
    dev = lambda k: c[k].to(DEV)
    wp, u, v = pack_ln_linear(dev("wqkv"), None, dev("gamma"), dev("beta"))
    coef_dev = ops.groupnorm_coef(dev("x"), c["B"], c["rows"], rc.GN_GROUPS, rc.GN_EPS, dev("gn_gamma"), dev("gn_beta"))
    torch.cuda.synchronize()
    return dict(x=pitched(c["x"], ldx), win=rc_pack_tiles(dev("win"), dev("bin").float()), wqkv=rc_pack_tiles(wp, v, u), ldy=ldy, ldqk=ldqk,
                ldt=c["rows"] + dt_, coef={"device": coef_dev, "fp64": c["coef"].to(DEV)})


@functools.lru_cache(maxsize=None)
def front_data(name, dname, variant):
    """(case, fp64 reference, emulation figures, bounds) for the coefficients the launch is handed: the reference applies GroupNorm THROUGH them"""
    c, ref, emu, bnd = rc.case_data("rc_front", name, dname)
    if variant == "fp64":
        return c, ref, emu, bnd
    coef = front_operands(name, dname)["coef"]["device"].cpu()
    ref = rc.reference(c, coef=coef)
    emu = rc.figures("rc_front", c, rc.emulate(c, coef=coef), ref)
    return c, ref, emu, rc.bounds_from(emu)


def launch_front(c, dname, variant, item=None):
    from theatergen_amd import ops
    o = front_operands(c["name"], dname)
    B, rows = c["B"], c["rows"]
    x, coef = o["x"], o["coef"][variant]
    if item is not None:
        x, coef, B = x[item * rows:(item + 1) * rows], coef[item:item + 1], 1
    M, ldt = B * rows, o["ldt"]
    sy, y = rows_out(M, rc.C, o["ldy"], c["dtype"])
    sq, qk = rows_out(M, 2 * rc.C, o["ldqk"], c["dtype"])
    sv = Storage((B * rc.C + GUARD) * ldt, c["dtype"])
    vt = sv.view(0, (B, rc.C, rows), (rc.C * ldt, ldt, 1))
    ops.rc_front(x, coef, o["win"], o["wqkv"], rows, c["eps"], y=y, qk=qk, vt=vt)
    return {"y": y, "qk": qk, "vt": vt}, [sy, sq, sv]


def run_front(name, dname, variant):
    c, ref, emu, bnd = front_data(name, dname, variant)
    what = f"rc_front {name} {dname} coef={variant}"
    B, rows = c["B"], c["rows"]
    fails = []
    if variant == "device":
        # fp32 statistics over >= 1280 elements of magnitude ~ 1: far inside 1e-4 of the largest coefficient (the statistics kernel is not under test here;
        # the judgement below takes whichever coefficients the launch was handed)
        dv, want = front_operands(name, dname)["coef"]["device"].cpu().double(), rc.groupnorm_coef_fp64(c)
        if not float((dv - want).abs().max()) <= 1e-4 * float(want.abs().max()):
            fails.append(f"{what}: tg_groupnorm_coef is off by {float((dv - want).abs().max()):.3e}")
    outs, sts = launch_front(c, dname, variant)
    fails += [f for st in sts for f in st.failures(what)]
    f2, fig = rc.judge("rc_front", c, {k: v.cpu() for k, v in outs.items()}, ref, bnd, what)
    report("rc_front", name, dname, variant, fig, emu, bnd)
    again, sts2 = launch_front(c, dname, variant)
    fails += f2 + [f for st in sts2 for f in st.failures(what + " (second launch)")]
    if not all(same_bits(outs[k], again[k]) for k in outs):
        fails.append(f"{what}: a second launch gave other bits")
    for b in (sorted({0, B // 2, B - 1}) if B > 1 else []):
        one, sts3 = launch_front(c, dname, variant, item=b)
        fails += [f for st in sts3 for f in st.failures(f"{what} (item {b} alone)")]
        sl = slice(b * rows, (b + 1) * rows)
        if not (same_bits(one["y"], outs["y"][sl]) and same_bits(one["qk"], outs["qk"][sl]) and same_bits(one["vt"][0], outs["vt"][b])):
            fails.append(f"{what}: item {b} launched alone differs from its part of the batched launch")
    return fails


def report(entry, name, dname, variant, fig, emu, bnd):
    FIGURES[(entry, name, dname, variant)] = (fig, emu, bnd)
    for o, f in fig.items():
        print(f"FIG {entry} {name} {dname} {variant or '-'} {o}: device rel-L2 {f[0]:.3e} block {f[1]:.3e} max-rel {f[2]:.3e} | emulation "
              f"{emu[o][0]:.3e} {emu[o][1]:.3e} {emu[o][2]:.3e} | worst device / bound {max(a / b for a, b in zip(f, bnd[o])):.2f}")


@pytest.mark.parametrize("dname", list(rc.DTYPES))
@pytest.mark.parametrize("name", list(rc.LINEAR_CASES))
def test_rc_linear(name, dname):
    """MI355X: device rel-L2 / emulation rel-L2 0.997 .. 1.000 on every case (bf16 1.6e-3 .. 2.0e-3, fp16 2.1e-4 .. 2.5e-4); rows at mean 8 / std 0.125:
    1.996e-3 / 2.503e-4, at mean 16 / std 0.0625: 1.850e-3 / 2.366e-4, each the emulation's figure: the two-pass statistics hold"""
    fails = run_linear(name, dname)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dname", list(rc.DTYPES))
@pytest.mark.parametrize("name", list(rc.XATTN_CASES))
def test_rc_xattn(name, dname):
    """MI355X: device rel-L2 / emulation rel-L2 0.9997 .. 1.0005; bf16 1.7e-3 .. 1.9e-3, fp16 2.1e-4 .. 2.3e-4; peaked cases 3.045e-3 / 2.984e-3 (bf16) and
    3.787e-4 / 3.821e-4 (fp16) against emulation figures of 3.045e-3 / 2.983e-3 and 3.788e-4 / 3.822e-4"""
    fails = run_xattn(name, dname)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("variant", ["device", "fp64"])
@pytest.mark.parametrize("dname", list(rc.DTYPES))
@pytest.mark.parametrize("name", list(rc.FRONT_CASES))
def test_rc_front(name, dname, variant):
    """MI355X: device rel-L2 / emulation rel-L2 0.9997 .. 1.0004 for y, qk and V^T with either coefficient source (bf16: y 2.2e-3, qk / V^T 3.0e-3; fp16:
    2.8e-4, 3.7e-4)"""
    fails = run_front(name, dname, variant)
    assert not fails, "\n".join(fails)


# ---- refusals: one row per TG_CHECK of the four entries that can be reached without a launch ---------------------------------------------------
SENTINEL = 3.0


class Call:
    """a valid call of one entry on small operands (M = 256, 2 items of 128); a table row breaks ONE argument"""

    def __init__(self, entry):
        from theatergen_amd import _lib
        dt = torch.bfloat16
        z = lambda *s, t=dt: torch.zeros(*s, dtype=t, device=DEV)
        self.entry, self.M = entry, 256
        self.outs = [torch.full((256 * 704 + 64,), SENTINEL, dtype=dt, device=DEV) for _ in range(3)]
        self.keep = dict(x=z(257, 352), res=z(257, 352), w=torch.zeros(30 * 21 * 1024 + 3072 + 64, dtype=torch.uint8, device=DEV), kv=z(2, 8, 24 * 512),
                         coef=z(2, 2, 320, t=torch.float32), ips=z(4, t=torch.float32), k=z(2 * 80 + 1, 320), vt=z(2, 320, 96))
        k = self.keep
        self.extra = {}
        if entry == "rc_linear":
            d = _lib.RcLinearDesc()
            d.dtype, d.x, d.ldx, d.wpk, d.res, d.ldres = 0, k["x"].data_ptr(), 352, k["w"].data_ptr(), k["res"].data_ptr(), 352
            d.out, d.ldc, d.M, d.N, d.K, d.ln, d.ln_eps, d.variant = self.outs[0].data_ptr(), 328, 256, 320, 320, 0, 0.0, 0
            self.extra = dict(dup=0)
        elif entry == "rc_xattn":
            d = _lib.RcXattnDesc()
            d.dtype, d.h, d.ldh, d.wq, d.kv, d.wo = 0, k["x"].data_ptr(), 352, k["w"].data_ptr(), k["kv"].data_ptr(), k["w"].data_ptr()
            d.out, d.ldc, d.M, d.rows_per_batch, d.text_len, d.ip_tokens, d.ln_eps = self.outs[0].data_ptr(), 328, 256, 128, 77, 4, 1e-5
            d.ip_scale = k["ips"].data_ptr()
            self.extra = dict(count=2)
        elif entry == "rc_front":
            d = _lib.RcFrontDesc()
            d.dtype, d.x, d.ldx, d.coef, d.win, d.wqkv = 0, k["x"].data_ptr(), 352, k["coef"].data_ptr(), k["w"].data_ptr(), k["w"].data_ptr()
            d.y, d.ldy, d.qk, d.ldqk, d.vt, d.ldt = self.outs[0].data_ptr(), 328, self.outs[1].data_ptr(), 704, self.outs[2].data_ptr(), 136
            d.M, d.rows_per_batch, d.ln_eps, d.dbg = 256, 128, 1e-5, 0
        else:
            d = dict(dtype=0, batch=2, k=k["k"].data_ptr(), vt=k["vt"].data_ptr(), ldt=96, text_len=77, kip=k["k"].data_ptr(), vtip=k["vt"].data_ptr(),
                     ldi=96, ip_tokens=4, out=self.outs[0].data_ptr())
        self.d = d

    def set(self, **kw):
        for key, val in kw.items():
            if key in self.extra:
                self.extra[key] = val
            elif isinstance(self.d, dict):
                self.d[key] = val
            else:
                setattr(self.d, key, val)

    def get(self, key):
        return self.d[key] if isinstance(self.d, dict) else getattr(self.d, key)

    def run(self):
        from theatergen_amd import _lib, ops
        L, s = _lib.lib(), ops._stream()
        if self.entry == "rc_linear":
            return L.tg_rc_linear_dup(C.byref(self.d), self.extra["dup"], s) if self.extra["dup"] else L.tg_rc_linear(C.byref(self.d), s)
        if self.entry == "rc_xattn":
            return L.tg_rc_xattn_ps(C.byref(self.d), self.extra["count"], s)
        if self.entry == "rc_front":
            return L.tg_rc_front(C.byref(self.d), s)
        a = self.d
        return L.tg_rc_kv_pack(a["dtype"], a["batch"], a["k"], a["vt"], a["ldt"], a["text_len"], a["kip"], a["vtip"], a["ldi"], a["ip_tokens"], a["out"], s)


off = lambda field, nbytes: (lambda c: {field: c.get(field) + nbytes})          # the same storage, 8 bytes further on: not 16-byte aligned
REFUSALS = [
    ("rc_linear", "dtype", dict(dtype=2)), ("rc_linear", "K_640", dict(K=640)), ("rc_linear", "K_256", dict(K=256)), ("rc_linear", "N_96", dict(N=96)),
    ("rc_linear", "N_0", dict(N=0)), ("rc_linear", "variant", dict(variant=1)), ("rc_linear", "M_0", dict(M=0)), ("rc_linear", "x_null", dict(x=None)),
    ("rc_linear", "ldx_below", dict(ldx=312)), ("rc_linear", "ldx_not8", dict(ldx=356)), ("rc_linear", "ldc_below", dict(ldc=312)),
    ("rc_linear", "ldc_not8", dict(ldc=324)), ("rc_linear", "ldres_below", dict(ldres=312)), ("rc_linear", "ldres_not8", dict(ldres=324)),
    ("rc_linear", "dup_inside", dict(dup=255 * 328 + 312)), ("rc_linear", "dup_not8", dict(dup=256 * 328 + 4)),
    ("rc_linear", "x_misaligned", off("x", 8)), ("rc_linear", "res_misaligned", off("res", 8)), ("rc_linear", "out_misaligned", off("out", 8)),
    ("rc_linear", "wpk_misaligned", off("wpk", 8)),
    ("rc_xattn", "dtype", dict(dtype=2)), ("rc_xattn", "text_64", dict(text_len=64)), ("rc_xattn", "ip_5", dict(ip_tokens=5)),
    ("rc_xattn", "rows_100", dict(rows_per_batch=100)), ("rc_xattn", "rows_not_dividing", dict(rows_per_batch=384)), ("rc_xattn", "M_0", dict(M=0)),
    ("rc_xattn", "kv_null", dict(kv=None)), ("rc_xattn", "ldh_below", dict(ldh=312)), ("rc_xattn", "ldh_not8", dict(ldh=324)),
    ("rc_xattn", "ldc_below", dict(ldc=312)), ("rc_xattn", "ldc_not8", dict(ldc=324)), ("rc_xattn", "count_3_of_2", dict(count=3)),
    ("rc_xattn", "count_negative", dict(count=-1)), ("rc_xattn", "count_2_null", dict(ip_scale=None)), ("rc_xattn", "h_misaligned", off("h", 8)),
    ("rc_xattn", "out_misaligned", off("out", 8)), ("rc_xattn", "kv_misaligned", off("kv", 8)), ("rc_xattn", "wq_misaligned", off("wq", 8)),
    ("rc_kv_pack", "dtype", dict(dtype=2)), ("rc_kv_pack", "batch_0", dict(batch=0)), ("rc_kv_pack", "text_81", dict(text_len=81)),
    ("rc_kv_pack", "text_0", dict(text_len=0)), ("rc_kv_pack", "ip_17", dict(ip_tokens=17)), ("rc_kv_pack", "ip_negative", dict(ip_tokens=-1)),
    ("rc_kv_pack", "kip_null", dict(kip=None)), ("rc_kv_pack", "vt_null", dict(vt=None)), ("rc_kv_pack", "ldt_below_text", dict(ldt=72)),
    ("rc_kv_pack", "ldi_below_ip", dict(ldi=3)), ("rc_kv_pack", "k_misaligned", off("k", 8)), ("rc_kv_pack", "kip_misaligned", off("kip", 8)),
    ("rc_kv_pack", "out_misaligned", off("out", 8)),
    ("rc_front", "dtype", dict(dtype=2)), ("rc_front", "rows_100", dict(rows_per_batch=100)), ("rc_front", "rows_not_dividing", dict(rows_per_batch=384)),
    ("rc_front", "M_0", dict(M=0)), ("rc_front", "coef_null", dict(coef=None)), ("rc_front", "ldx_below", dict(ldx=312)), ("rc_front", "ldx_not8", dict(ldx=324)),
    ("rc_front", "ldy_below", dict(ldy=312)), ("rc_front", "ldy_not8", dict(ldy=324)), ("rc_front", "ldqk_below", dict(ldqk=632)),
    ("rc_front", "ldqk_not8", dict(ldqk=644)), ("rc_front", "ldt_below_rows", dict(ldt=120)), ("rc_front", "dbg", dict(dbg=1)),
    ("rc_front", "x_misaligned", off("x", 8)), ("rc_front", "y_misaligned", off("y", 8)), ("rc_front", "qk_misaligned", off("qk", 8)),
    ("rc_front", "coef_misaligned", off("coef", 8)),
]


@pytest.mark.parametrize("entry,label,change", REFUSALS, ids=[f"{e}-{l}" for e, l, _ in REFUSALS])
def test_refusal(entry, label, change):
    """TG_ERR_ARG before any launch, and no output element changes.  Stated field by field on the C descriptors (most of these values never pass the Python
    wrappers' own checks); the unbroken call of every entry is what the case tests above launch, so none is launched here"""
    call = Call(entry)
    call.set(**(change(call) if callable(change) else change))
    rcode = call.run()
    torch.cuda.synchronize()
    assert rcode == ERR_ARG, f"{entry} {label}: returned {rcode}"
    for o in call.outs:
        assert bool((o == SENTINEL).all()), f"{entry} {label}: a refused call wrote to an output"


def test_refusal_table_breaks_one_argument_of_a_valid_call():
    """the rows refuse for the reason they name: every base call passes each of its entry's host checks (re-stated here from the header, not launched)"""
    for entry in ("rc_linear", "rc_xattn", "rc_kv_pack", "rc_front"):
        c = Call(entry)
        g = c.get
        if entry == "rc_linear":
            ok = g("K") == 320 and g("N") % 64 == 0 and min(g("ldx"), g("ldc"), g("ldres")) >= 320 and all(g(f) % 8 == 0 for f in ("ldx", "ldc", "ldres"))
            ok = ok and all(g(f) % 16 == 0 for f in ("x", "wpk", "res", "out")) and g("variant") == 0
        elif entry == "rc_xattn":
            ok = g("text_len") == 77 and g("ip_tokens") in (0, 4, 16) and g("rows_per_batch") % 128 == 0 and g("M") % g("rows_per_batch") == 0
            ok = ok and c.extra["count"] == g("M") // g("rows_per_batch") and all(g(f) % 16 == 0 for f in ("h", "wq", "kv", "wo", "out"))
        elif entry == "rc_front":
            ok = g("rows_per_batch") % 128 == 0 and g("M") % g("rows_per_batch") == 0 and g("ldqk") >= 640 and g("ldt") >= g("rows_per_batch") and g("dbg") == 0
            ok = ok and all(g(f) % 16 == 0 for f in ("x", "coef", "win", "wqkv", "y", "qk"))
        else:
            ok = 0 < g("text_len") <= 80 and 0 <= g("ip_tokens") <= 16 and g("ldt") >= g("text_len") and g("ldi") >= g("ip_tokens")
            ok = ok and all(g(f) % 16 == 0 for f in ("k", "kip", "out"))
        assert ok, entry
