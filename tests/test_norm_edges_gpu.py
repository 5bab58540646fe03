"""GPU: single hand-made launches of ``tg_groupnorm``, ``tg_groupnorm_coef``, ``tg_groupnorm_from_partials``, ``tg_layernorm``, ``tg_layernorm_stats``
and ``tg_layernorm_add`` through the C ABI against the fp64 restatement of their contracts (tests/norm_contract.py), at the smallest shapes that enter
each kernel instance and each branch of the host code (the cases and what each enters: norm_contract.GN_TWO_LAUNCH ... LNA_CASES).

Per case and dtype: every input element the contract does not read holds NaN; outputs and the GroupNorm scratch (exactly
``tg_groupnorm_scratch_bytes``, guard rows around it) are NaN before the launch, every element of the written region is finite afterwards and every other
element still NaN; storage-dtype outputs are judged against fp64 for the whole tensor, for every block and at max|err| / max|ref| with 1.5 x / 1.5 x / 2 x
the figures the fp32 model reaches on the same case; fp32 outputs (coef, stats) element by element against the bound derived in norm_contract's
docstring; a second launch gives the same bits; a batch item (a row) launched alone gives the same bits wherever ``plan`` says the summation order is
the same, and is judged at its own bound otherwise.  Cross-entry: ``tg_groupnorm_coef`` followed by ``x a + d`` reproduces ``tg_groupnorm`` bit for bit
on the two-launch path (a SiLU case is launched once more without the activation for this; with SiLU applied on the host, and on the small path, the
result is judged at the case's bound); ``tg_layernorm_stats`` applied to the rows is
``tg_layernorm`` at the sibling case's bound; ``out`` aliasing ``x`` (or ``res``) of the LayerNorm entries gives the bits of the separate output.

No tolerance here was tuned on a kernel; the only allowance (two-launch path at |mean| / std >= 64, if the model leaves the floor) is not taken by any
case: profiles/norm_contract_findings.md has the measured tables.  Measured on MI355X: the device's rel-L2 is the model's to four digits on every launch
(bf16 1.61e-3 .. 1.87e-3, fp16 1.67e-4 .. 2.27e-4; two-launch path at |mean| / std = 64 in fp16: 2.213e-4 and 2.244e-4 against a floor of 2.10e-4 and
2.09e-4), worst device / bound 0.67, worst fp32 element / bound 0.859 (from_partials coefficients, where the bound is the two roundings of `a` alone);
coef + apply is bit-equal on every two-launch case and has the model's figures where it is judged.  The whole file takes 3 s.
"""
import pytest
import torch

from tests import norm_contract as nc
from tests.gemm_contract import _storage_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_ARG, ERR_UNSUPPORTED = -1, -3
FIGURES = {}

ARGS = {
    "groupnorm": ("dtype", "x0", "x1", "c0", "c1", "batch", "hw", "groups", "eps", "gamma", "beta", "silu", "out", "partials"),
    "groupnorm_coef": ("dtype", "x0", "x1", "c0", "c1", "batch", "hw", "groups", "eps", "gamma", "beta", "coef", "partials"),
    "from_partials": ("dtype", "x", "C", "batch", "hw", "groups", "eps", "gamma", "beta", "silu", "out", "coef", "partials", "nblk"),
    "layernorm": ("dtype", "x", "rows", "C", "ldx", "eps", "gamma", "beta", "out", "ldo"),
    "layernorm_stats": ("dtype", "x", "rows", "C", "ldx", "eps", "stats"),
    "layernorm_add": ("dtype", "x", "ldx", "res", "ldres", "rows", "C", "eps", "gamma", "beta", "out", "ldo"),
}
SYMBOL = {e: "tg_groupnorm_from_partials" if e == "from_partials" else "tg_" + e for e in ARGS}
POINTERS = ("x0", "x1", "x", "res", "gamma", "beta", "out", "coef", "stats", "partials")


def run_call(L, entry, call, stream):
    """the C call of ``entry`` with the arguments of ``call`` (pointers: integers or None)"""
    return getattr(L, SYMBOL[entry])(*[call[k] for k in ARGS[entry]], stream)


def to_call(a):
    call = {k: a.get(k) for k in ARGS[a["entry"]]}
    call["dtype"] = a["dtype_code"]
    for k in POINTERS:
        if k in call and call[k] is not None:
            call[k] = call[k].data_ptr()
    return call


def as_launch(entry, call):
    """a call as the dict norm_contract.host_check_failures reads"""
    return dict(call, entry=entry, dtype_code=call["dtype"])


def launch(a):
    from theatergen_amd import _lib, ops
    _lib.check(run_call(_lib.lib(), a["entry"], to_call(a), ops._stream()))
    return a


def storage_failures(a, what):
    """every element of the written regions finite, every other element of the output storages and of the scratch still NaN"""
    torch.cuda.synchronize()
    fails = []
    regs = nc.written_region(a)
    owners = {r.name: r for r in regs}
    for name in ("out", "coef", "stats", "partials"):
        t = a.get(name)
        if t is None or (name == "partials" and a["entry"] == "from_partials"):
            continue
        flat = _storage_tensor(t)
        mask = torch.zeros(flat.numel(), dtype=torch.bool, device=flat.device)
        if name in owners:
            r = owners[name]
            mask.as_strided(r.sizes, r.strides, r.storage_byte_offset() // r.esize).fill_(True)
        if not bool(torch.isfinite(flat[mask]).all()):
            fails.append(f"{what}: {int((~torch.isfinite(flat[mask])).sum())} elements of the written region of {name} are not finite")
        if not bool(torch.isnan(flat[~mask]).all()):
            fails.append(f"{what}: {int((~torch.isnan(flat[~mask])).sum())} elements of {name} outside the written region were written")
    return fails


def outputs(a):
    return {r.name: r.view() for r in nc.written_region(a) if r.name != "partials"}


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(x, y):
    return torch.equal(bits(x), bits(y))


def report(cid, dname, variant, fig, mfig, bnd):
    FIGURES[(cid, dname, variant)] = (fig, mfig, bnd)
    for o, f in fig.items():
        if len(f) > 5:
            print(f"FIG {cid} {dname} {variant or '-'} {o}: device rel-L2 {f[0]:.3e} max-rel {f[2]:.3e} | model {mfig[o][0]:.3e} {mfig[o][2]:.3e} | worst element / bound {f[5]:.3f}")
        else:
            print(f"FIG {cid} {dname} {variant or '-'} {o}: device rel-L2 {f[0]:.3e} block {f[1]:.3e} max-rel {f[2]:.3e} | model {mfig[o][0]:.3e} {mfig[o][1]:.3e} "
                  f"{mfig[o][2]:.3e} | device / model {f[0] / mfig[o][0]:.4f} | worst device / bound {max(x / y for x, y in zip(f[:3], bnd[o])):.2f}")


def independent_items(a):
    """(indices to launch alone, True when ``plan`` says the launch alone sums in the batched launch's order)"""
    if a["entry"] in nc.LN_ENTRIES:
        return ([a["rows"] - 1] if a["rows"] > 1 else []), True
    B = a["batch"]
    if B == 1:
        return [], True
    pl = nc.plan(a)
    same = pl["path"] in ("small", "partials-coef") or nc.gn_nblk(1, a["hw"]) == pl["gn_nblk"]
    return sorted({0, B - 1}), same


def run_case(cid, dname):
    a_cpu, ref, mod, mfig, bnd, elem = nc.case_data(cid, dname)
    what = f"{cid} {dname}"
    a = launch(nc.make_case(cid, nc.DTYPES[dname], device=DEV))
    fails = storage_failures(a, what)
    outs = outputs(a)
    f2, fig = nc.judge(a_cpu, {k: v.cpu() for k, v in outs.items()}, ref, bnd, elem, what)
    report(cid, dname, "", fig, mfig, bnd)
    fails += f2
    again = launch(nc.fresh_outputs(a))
    fails += storage_failures(again, what + " (second launch)")
    if not all(same_bits(outs[k], v) for k, v in outputs(again).items()):
        fails.append(f"{what}: a second launch gave other bits")
    idx, same = independent_items(a)
    for i in idx:
        one = launch(nc.item_launch(a, i))
        fails += storage_failures(one, f"{what} (item {i} alone)")
        for k, v in outputs(one).items():
            if same:
                if not same_bits(v[0], outs[k][i]):
                    fails.append(f"{what}: item {i} launched alone differs from its part of the batched launch")
            else:
                c1 = nc.item_launch(a_cpu, i)
                r1 = nc.reference(c1)
                m1 = nc.figures(c1, nc.model(c1), r1)
                f3, fig1 = nc.judge(c1, {k: v.cpu()}, r1, nc.bounds_from(m1), nc.fp32_bound(c1), f"{what} (item {i} alone)")
                report(cid, dname, f"item{i}", fig1, m1, nc.bounds_from(m1))
                fails += f3
    return fails, a, a_cpu, outs


def coef_then_apply(a, a_cpu, outs, cid, dname):
    """tg_groupnorm_coef on the operands of a tg_groupnorm launch, then the header's apply expression: bit for bit on the two-launch path before the activation"""
    _, ref, _, mfig, bnd, _ = nc.case_data(cid, dname)
    b = dict(a, entry="groupnorm_coef", coef=True, silu=0)
    b.pop("out")
    b = launch(nc.fresh_outputs(b))
    fails = storage_failures(b, f"{cid} {dname} (coef)")
    cf = outputs(b)["coef"].double()
    x = nc._x({r.name: r.view() for r in nc.read_extents(a) if r.name in ("x0", "x1")}, a).double()
    f = (x * cf[:, 0][:, None, :] + cf[:, 1][:, None, :]).float()                # round_fp32(x a + d): the kernel's fma
    if nc.plan(a)["path"] == "two-launch":
        plain = outs["out"] if not a["silu"] else outputs(launch(nc.fresh_outputs(dict(a, silu=0))))["out"]      # the same launch without the activation
        if not same_bits(f.to(a["dtype"]), plain):
            fails.append(f"{cid} {dname}: tg_groupnorm_coef + (x a + d) differs from tg_groupnorm in {int((bits(f.to(a['dtype'])) != bits(plain)).sum())} elements")
    if a["silu"]:
        f = f * (1.0 / (1.0 + torch.exp2(-1.4426950408889634 * f)))
    got = f.to(a["dtype"])
    if nc.plan(a)["path"] != "two-launch" or a["silu"]:
        f2, fig = nc.judge(a_cpu, {"out": got.cpu()}, ref, bnd, None, f"{cid} {dname} (coef, then x a + d)")
        report(cid, dname, "coef+apply", fig, mfig, bnd)
        fails += f2
    return fails


@pytest.mark.parametrize("dname", list(nc.DTYPES))
@pytest.mark.parametrize("name", list(nc.GN_TWO_LAUNCH) + [f"offset:{k}" for k in nc.GN_OFFSET])
def test_groupnorm_two_launch(name, dname):
    cid = f"gn-offset {name[7:]}" if name.startswith("offset:") else f"gn-two {name}"
    fails, a, a_cpu, outs = run_case(cid, dname)
    assert nc.plan(a)["path"] == "two-launch" and nc.plan(a) == nc.plan(a_cpu), "the device buffers take the CPU case's path"
    if a["entry"] == "groupnorm":
        fails += coef_then_apply(a, a_cpu, outs, cid, dname)
    if "const" in name:
        _, grp = 1, 5                                                           # variance exactly 0: the group is act(beta) to fp32 rounding of 2 a + (beta - 2 a)
        cpg = nc.channels(a) // a["groups"]
        be = a["beta"].float()[grp * cpg:(grp + 1) * cpg]
        want = be * torch.sigmoid(be)
        got = outs["out"][1, :, grp * cpg:(grp + 1) * cpg].float()
        tol = 2.0 ** -8 if dname == "bf16" else 2.0 ** -11
        if not bool(((got - want).abs() <= tol * want.abs() + 2.0 ** -14).all()):    # 2^-15: half an ulp of 2 a = 2 gamma eps^-1/2 < 1024
            fails.append(f"{cid} {dname}: the constant group is not SiLU(beta)")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dname", list(nc.DTYPES))
@pytest.mark.parametrize("name", list(nc.GN_SMALL))
def test_groupnorm_small(name, dname):
    cid = f"gn-small {name}"
    fails, a, a_cpu, outs = run_case(cid, dname)
    assert nc.plan(a)["path"] == "small" and nc.plan(a) == nc.plan(a_cpu)
    if a["entry"] == "groupnorm":
        fails += coef_then_apply(a, a_cpu, outs, cid, dname)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dname", list(nc.DTYPES))
@pytest.mark.parametrize("name", list(nc.GN_PARTIALS))
def test_groupnorm_from_partials(name, dname):
    fails, *_ = run_case(f"gn-partials {name}", dname)
    assert not fails, "\n".join(fails)


def aliased(a, which):
    """the launch with ``out`` on the storage of a copy of ``which`` (x or res): same pitch, same pad columns"""
    b = dict(a)
    ld = a["ldx" if which == "x" else "ldres"]
    src = a[which]
    buf = nc.bc._pitched(src.cpu(), ld, DEV)[:, :a["C"]]
    b[which], b["out"], b["ldo"] = buf, buf, ld
    return b


@pytest.mark.parametrize("dname", list(nc.DTYPES))
@pytest.mark.parametrize("name", list(nc.LN_CASES))
def test_layernorm(name, dname):
    cid = f"ln {name}"
    fails, a, a_cpu, outs = run_case(cid, dname)
    b = launch(aliased(a, "x"))
    fails += storage_failures(b, f"{cid} {dname} (out = x)")
    if not same_bits(outputs(b)["out"], outs["out"]):
        fails.append(f"{cid} {dname}: out aliasing x gives other bits")
    # tg_layernorm_stats on the same rows, applied: the normalised tensor at this case's bound
    s_cpu, s_ref, _, s_mfig, _, s_elem = nc.case_data(f"ln-stats {name}", dname)
    s = launch(nc.make_case(f"ln-stats {name}", nc.DTYPES[dname], device=DEV))
    fails += storage_failures(s, f"ln-stats {name} {dname}")
    st = outputs(s)["stats"]
    f2, sfig = nc.judge(s_cpu, {"stats": st.cpu()}, s_ref, None, s_elem, f"ln-stats {name} {dname}")
    report(f"ln-stats {name}", dname, "", sfig, s_mfig, None)
    fails += f2
    if not same_bits(st, outputs(launch(nc.fresh_outputs(s)))["stats"]):
        fails.append(f"ln-stats {name} {dname}: a second launch gave other bits")
    if a["rows"] > 1:
        one = launch(nc.item_launch(s, a["rows"] - 1))
        if not same_bits(outputs(one)["stats"][0], st[-1]):
            fails.append(f"ln-stats {name} {dname}: the last row launched alone gives other bits")
    _, ref, _, mfig, bnd, _ = nc.case_data(cid, dname)
    ext = nc._ext(a_cpu)
    y = ext["x"].float() * st.cpu()[:, :1] + st.cpu()[:, 1:]
    y = y * ext["gamma"].float() if "gamma" in ext else y
    y = y + ext["beta"].float() if "beta" in ext else y
    f3, fig = nc.judge(a_cpu, {"out": y.to(a["dtype"])}, ref, bnd, None, f"{cid} {dname} (through tg_layernorm_stats)")
    report(cid, dname, "stats+apply", fig, mfig, bnd)
    assert not fails + f3, "\n".join(fails + f3)


@pytest.mark.parametrize("dname", list(nc.DTYPES))
@pytest.mark.parametrize("name", list(nc.LNA_CASES))
def test_layernorm_add(name, dname):
    cid = f"ln-add {name}"
    fails, a, a_cpu, outs = run_case(cid, dname)
    for which in ("x", "res"):
        b = launch(aliased(a, which))
        fails += storage_failures(b, f"{cid} {dname} (out = {which})")
        if not same_bits(outputs(b)["out"], outs["out"]):
            fails.append(f"{cid} {dname}: out aliasing {which} gives other bits")
    assert not fails, "\n".join(fails)


# ---- refusals: one row breaks one argument of a valid call --------------------------------------------------------------------------------------
SENTINEL = 3.0
BASE = {
    "groupnorm": dict(dtype=0, c0=48, c1=16, batch=2, hw=16, groups=8, eps=1e-5, silu=1),
    "groupnorm_coef": dict(dtype=0, c0=48, c1=16, batch=2, hw=16, groups=8, eps=1e-5),
    "from_partials": dict(dtype=0, C=64, batch=2, hw=16, groups=8, eps=1e-5, silu=1, coef=None, nblk=1),
    "layernorm": dict(dtype=0, rows=4, C=64, ldx=72, eps=1e-5, ldo=80),
    "layernorm_stats": dict(dtype=0, rows=4, C=64, ldx=72, eps=1e-5),
    "layernorm_add": dict(dtype=0, rows=4, C=64, ldx=72, ldres=72, eps=1e-5, ldo=80),
}
SIZES = dict(x0=2 * 16 * 48 * 2, x1=2 * 16 * 16 * 2, x=2 * 16 * 64 * 2, res=4 * 72 * 2, gamma=64 * 2, beta=64 * 2, out=2 * 16 * 64 * 2, coef=2 * 2 * 64 * 4, stats=4 * 2 * 4,
             partials=4 * nc.gn_scratch_floats(2, 16, 8))
OUTPUTS = ("out", "coef", "stats", "partials")


def base_call(entry, alloc):
    """a valid call of ``entry`` on small operands; ``alloc(nbytes)`` -> a 16-byte aligned address"""
    call = dict(BASE[entry])
    for k in ARGS[entry]:
        if k in POINTERS and k not in call:
            call[k] = alloc(SIZES[k] + 64)
    return call


off8 = lambda field: (lambda c: {field: c[field] + 8})                          # the same storage, 8 bytes further on: not 16-byte aligned
_gn_rows = lambda e, out: [
    (e, "dtype", dict(dtype=2)), (e, "x0_null", dict(x0=None)), (e, f"{out}_null", {out: None}), (e, "partials_null", dict(partials=None)),
    (e, "batch_0", dict(batch=0)), (e, "hw_0", dict(hw=0)), (e, "groups_0", dict(groups=0)), (e, "groups_7", dict(groups=7)), (e, "c0_44", dict(c0=44)),
    (e, "c1_12", dict(c1=12)), (e, "C_8200", dict(c0=8184)), (e, "batch_65536", dict(batch=65536)), (e, "x0_misaligned", off8("x0")),
    (e, "x1_misaligned", off8("x1"))]
REFUSALS = _gn_rows("groupnorm", "out") + [("groupnorm", "out_misaligned", off8("out"))] + _gn_rows("groupnorm_coef", "coef") + [
    ("groupnorm_coef", "groups_264", dict(groups=264, c0=2096)),
    ("from_partials", "dtype", dict(dtype=2)), ("from_partials", "partials_null", dict(partials=None)), ("from_partials", "nblk_0", dict(nblk=0)),
    ("from_partials", "out_null", dict(out=None)), ("from_partials", "x_null", dict(x=None)), ("from_partials", "batch_0", dict(batch=0)),
    ("from_partials", "hw_0", dict(hw=0)), ("from_partials", "groups_7", dict(groups=7)), ("from_partials", "groups_264", dict(groups=264, C=2112)),
    ("from_partials", "C_60", dict(C=60, groups=4)), ("from_partials", "C_8200", dict(C=8200)), ("from_partials", "batch_65536", dict(batch=65536)),
    ("from_partials", "x_misaligned", off8("x")), ("from_partials", "out_misaligned", off8("out")),
    ("layernorm", "dtype", dict(dtype=2)), ("layernorm", "x_null", dict(x=None)), ("layernorm", "out_null", dict(out=None)), ("layernorm", "rows_0", dict(rows=0)),
    ("layernorm", "C_0", dict(C=0)), ("layernorm", "C_60", dict(C=60)), ("layernorm", "C_4104", dict(C=4104, ldx=4104, ldo=4104)),
    ("layernorm", "ldx_not8", dict(ldx=68)), ("layernorm", "ldo_not8", dict(ldo=68)), ("layernorm", "ldx_below", dict(ldx=56)),
    ("layernorm", "ldo_below", dict(ldo=56)), ("layernorm", "x_misaligned", off8("x")), ("layernorm", "out_misaligned", off8("out")),
    ("layernorm", "gamma_misaligned", off8("gamma")), ("layernorm", "beta_misaligned", off8("beta")),
    ("layernorm_stats", "dtype", dict(dtype=2)), ("layernorm_stats", "x_null", dict(x=None)), ("layernorm_stats", "stats_null", dict(stats=None)),
    ("layernorm_stats", "rows_0", dict(rows=0)), ("layernorm_stats", "C_60", dict(C=60)), ("layernorm_stats", "C_4104", dict(C=4104, ldx=4104)),
    ("layernorm_stats", "ldx_not8", dict(ldx=68)), ("layernorm_stats", "ldx_below", dict(ldx=56)), ("layernorm_stats", "x_misaligned", off8("x")),
    ("layernorm_stats", "stats_misaligned", lambda c: dict(stats=c["stats"] + 4)),
    ("layernorm_add", "dtype", dict(dtype=2)), ("layernorm_add", "gamma_null", dict(gamma=None)), ("layernorm_add", "res_null", dict(res=None)),
    ("layernorm_add", "rows_0", dict(rows=0)), ("layernorm_add", "C_60", dict(C=60)), ("layernorm_add", "C_1288_unsupported", dict(C=1288, ldx=1288, ldres=1288, ldo=1288)),
    ("layernorm_add", "ldres_not8", dict(ldres=68)), ("layernorm_add", "ldx_below", dict(ldx=56)), ("layernorm_add", "ldo_below", dict(ldo=56)),
    ("layernorm_add", "res_misaligned", off8("res")), ("layernorm_add", "out_misaligned", off8("out")),
]
ERR_CODES = {"C_1288_unsupported": ERR_UNSUPPORTED}


@pytest.mark.parametrize("entry,label,change", REFUSALS, ids=[f"{e}-{l}" for e, l, _ in REFUSALS])
def test_refusal(entry, label, change):
    """the documented error before any launch, and no output element changes.  The unbroken call of every entry passes every host check
    (tests/test_norm_contract_cpu.py shows it without a GPU, and shows each row refused by the library there too); none is launched here"""
    from theatergen_amd import _lib, ops
    keep = []

    def alloc(nbytes):
        keep.append(torch.full((nbytes // 4,), SENTINEL, dtype=torch.float32, device=DEV))
        return keep[-1].data_ptr()
    call = base_call(entry, alloc)
    assert nc.host_check_failures(as_launch(entry, call)) == []
    call.update(change(call) if callable(change) else change)
    rcode = run_call(_lib.lib(), entry, call, ops._stream())
    torch.cuda.synchronize()
    assert rcode == ERR_CODES.get(label, ERR_ARG), f"{entry} {label}: returned {rcode}"
    assert all(bool((t == SENTINEL).all()) for t in keep), f"{entry} {label}: a refused call wrote to a buffer"
