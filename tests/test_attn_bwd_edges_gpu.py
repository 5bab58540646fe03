"""GPU: hand-made edge descriptors of ``tg_attention_bwd`` / ``tg_attention_bwd_cross`` (csrc/tg_attention_bwd.hip: one kernel template, three
modes — row statistics, dQ, dK + dV) against the fp64 restatement of their C-ABI contracts (tests/attn_bwd_contract.py), and the materialised
fallback of ``backward.attention_input_grad`` at head dim 80.

The descriptors are filled through ``theatergen_amd._lib`` directly, so pitches the ``ops`` wrappers never produce are reachable.  Every case
  * compares dQ (dK, dV) with the restatement, whole tensor AND every (batch item, head, 128-row block) — the unit one workgroup owns;
  * fills the output storages (pad columns of pitched outputs, rows past n, the gap between batch items included) and ``stats`` with a
    sentinel byte pattern first and checks that every byte outside the written region kept it;
  * replays once into NaN-filled outputs and NaN-filled ``stats``: same bits, no NaN (every element written, from the inputs alone).
Every element of an input buffer that the contract does not read holds NaN (pad columns of fused / pitched rows, gap rows, the t_ld and
extra_ld padding), so a read outside the contract shows in the outputs.

Tolerances (not tuned on the kernel): 1.5 x launch_check's per-launch bound — rel-L2 4.5e-3 (bf16) / 6e-4 (fp16), max error 1.5e-2 / 3.75e-3
of the peak — for the whole tensor and for every block.  An fp32 model of the kernel sits at 1.75e-3 / 2.2e-4 (test_attn_bwd_contract_cpu.py),
and every fault injected there fails.  No widening for the hardware exp2 / log2 was needed: see profiles/attn_bwd_contract_findings.md for the
measured figures.  The x8 peaked-softmax input is kept: the fp32 model passes it on the CPU at the unchanged tolerances.
"""
import ctypes as C

import pytest
import torch

from tests import attn_bwd_contract as ab
from tests import gemm_contract as gc
from tests import launch_check as lc
from tests import parity_metrics as pm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
SENTINEL = 0xA5
TG_ERR_ARG, TG_ERR_UNSUPPORTED = -1, -3


def tols(dtype):
    return 1.5 * lc.l2_tol(dtype), 1.5 * lc.rel_tol(dtype)


def _gpu_transpose(src, B, rows, cols):
    from theatergen_amd import ops
    return ops.transpose(src, B, rows, cols)


def descriptor(a):
    """the ctypes descriptor of a contract dict, and its entry point"""
    from theatergen_amd import _lib, ops
    L = _lib.lib()
    p = ops._ptr
    if "n_q" in a:
        d = _lib.AttnBwdCrossDesc()
        d.dtype, d.batch, d.heads, d.head_dim, d.n_q, d.n_k = ops._dt(a["q"]), a["batch"], a["heads"], a["head_dim"], a["n_q"], a["n_k"]
        d.q, d.dout, d.q_ld, d.q_bs = p(a["q"]), p(a["dout"]), a["q_ld"], a["q_bs"]
        d.k, d.v, d.k_ld, d.k_bs = p(a["k"]), p(a["v"]), a["k_ld"], a["k_bs"]
        d.kt, d.t_ld, d.t_bs = p(a["kt"]), a["t_ld"], a["t_bs"]
        d.extra, d.extra_ld = p(a["extra"]), a["extra_ld"]
        d.stats, d.dq = p(a["stats"]), p(a["dq"])
        d.scale, d.ds_scale = a["scale"], a["ds_scale"]
        return d, L.tg_attention_bwd_cross
    d = _lib.AttnBwdDesc()
    d.dtype, d.batch, d.heads, d.head_dim, d.n = ops._dt(a["q"]), a["batch"], a["heads"], a["head_dim"], a["n"]
    d.q, d.k, d.v, d.dout, d.ld, d.bs = p(a["q"]), p(a["k"]), p(a["v"]), p(a["dout"]), a["ld"], a["bs"]
    d.qt, d.kt, d.doutt, d.t_ld, d.t_bs = p(a["qt"]), p(a["kt"]), p(a["doutt"]), a["t_ld"], a["t_bs"]
    d.stats, d.dq, d.dk, d.dv = p(a["stats"]), p(a["dq"]), p(a["dk"]), p(a["dv"])
    d.scale = a["scale"]
    return d, L.tg_attention_bwd


def launch(a):
    from theatergen_amd import ops
    d, fn = descriptor(a)
    rc = fn(C.byref(d), ops._stream())
    torch.cuda.synchronize()
    return rc


def run_case(a, what):
    """the three checks of this file on one descriptor -> {output: metrics}"""
    cross = "n_q" in a
    reads = ab.cross_read_extents(a) if cross else ab.self_read_extents(a)
    writes = ab.cross_written_region(a) if cross else ab.self_written_region(a)
    lc.LaunchChecker._check_reads(reads + writes, what)
    assert ab.transposes_consistent(a), f"{what}: the transposed operands are not the transposes"
    dtype = a["q"].dtype
    ref = ab.cross_reference(a) if cross else ab.self_reference(a)
    mag = (ab.cross_reference if cross else ab.self_reference)(a, magnitude=True)     # the floor of a reference that cancels to zero (n_k = 1)
    masks = lc.LaunchChecker._write_masks(writes)
    lc.LaunchChecker._check_overlap(masks, reads, what)
    for t, _ in masks.values():
        lc._bytes(t).fill_(SENTINEL)
    snaps = lc.LaunchChecker._snapshot(masks)
    assert launch(a) == 0, what
    lc.LaunchChecker._check_outside(masks, snaps, what)
    first = {w.name: w.view().clone() for w in writes}
    assert bool(torch.isfinite(first["stats"]).all()), f"{what}: non-finite row statistics"
    l2, mx = tols(dtype)
    out, failed = {}, []
    for name in ref:
        ok, m = ab.compare(first[name], ref[name], a["heads"], l2, mx, mag[name])
        pm.record(f"attn_bwd edge {what} {name}", m, l2_tol=l2, max_tol=mx)
        print(f"{what} {name}: rel_l2={m['rel_l2']:.3e} max={m['max_rel']:.3e} block={m['block_rel_l2']:.3e}@{m['block_at']} "
              f"block_max={m['block_max_rel']:.3e}")
        out[name] = m
        if not ok:
            failed.append((name, m))
    assert not failed, f"{what}: {failed} (tolerances rel-L2 {l2:.1e}, max {mx:.1e}, whole tensor and every block)"
    # replay: NaN everywhere the launch may write
    for t, _ in masks.values():
        gc._storage_tensor(t).fill_(float("nan"))
    assert launch(a) == 0, what
    for w in writes:
        again = w.view()
        assert not bool(torch.isnan(again).any()), f"{what}: {w.name} of the replay keeps NaN (an element was not written, or read stale memory)"
        bits = torch.int32 if w.name == "stats" else torch.int16
        assert torch.equal(again.contiguous().view(bits), first[w.name].contiguous().view(bits)), \
            f"{what}: {w.name} of the replay into NaN-filled buffers differs from the first launch"
    return out


def _name(dtype):
    return str(dtype).replace("torch.", "")


# ---- self-attention ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [8, 56, 64, 72, 120, 128, 136, 264])
def test_self_sequence_lengths(dtype, n):
    """head dim 64, 2 items x 2 heads: one partial tile (8, 56), exact tile boundaries (64, 128), an 8-row ragged tile (72, 136; at 136 the
    second row block holds 8 rows), five tiles and three row blocks (264).  n <= 128 launches 4 workgroups (fewer than the 8 XCDs), n = 264
    launches 12 (the remainder branch of the XCD walk)."""
    a = ab.make_self_case(dtype, 2, n, 2, 64, device=DEV, transpose=_gpu_transpose)
    run_case(a, f"self n={n} d=64 {_name(dtype)}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [8, 24, 40, 56])
def test_self_head_dims(dtype, d):
    """n = 136: the d < head-dim-64 cuts fall inside a 16-wide k-step (8, 24, 40, 56) and inside a 32-wide output tile (8, 24, 40, 56)"""
    a = ab.make_self_case(dtype, 1, 136, 3, d, device=DEV, transpose=_gpu_transpose)
    run_case(a, f"self n=136 d={d} {_name(dtype)}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_self_grid_not_a_multiple_of_eight(dtype):
    """3 items x 3 heads x 2 row blocks = 18 workgroups: the XCD-chunked walk's remainder branch; every (item, head) has data of its own, so
    a wrong block-to-(item, head, block) map shows in that block's figure"""
    a = ab.make_self_case(dtype, 3, 136, 3, 64, device=DEV, transpose=_gpu_transpose)
    q = a["q"].reshape(3, 136, 3, 64)
    assert len({float(q[b, :, h].double().sum()) for b in range(3) for h in range(3)}) == 9
    run_case(a, f"self grid 3x3x136 d=64 {_name(dtype)}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [40, 64])
def test_self_fused_qkv_buffer_and_padded_pitches(dtype, d):
    """q, k, v as column slices of one [batch * (n + 5) + 3, 3 * inner + 8] buffer (ld = 3 * inner + 8, five gap rows between items), dout /
    dq / dk / dv in buffers of that pitch (the descriptor has ONE ld / bs for the seven row-major tensors), t_ld = n + 8 with NaN in the pad
    columns of the transposes: the kernel may read only columns below n and write only [item][row < n][column < inner]."""
    a = ab.make_self_case(dtype, 2, 136, 2, d, device=DEV, layout="fused", transpose=_gpu_transpose)
    assert a["ld"] == 3 * 2 * d + 8 and a["t_ld"] == 144 and a["q"].data_ptr() != a["k"].data_ptr()
    assert a["k"].untyped_storage().data_ptr() == a["q"].untyped_storage().data_ptr() == a["v"].untyped_storage().data_ptr()
    run_case(a, f"self fused n=136 d={d} {_name(dtype)}")


# ---- cross-attention -----------------------------------------------------------------------------------------------------------------
CROSS_PAIRS = [(100, 1), (1, 4), (128, 7), (130, 8), (100, 63), (128, 64), (130, 65), (100, 77), (130, 129)]      # (n_q, n_k)


def test_cross_pairs_cover_every_count():
    assert {p[1] for p in CROSS_PAIRS} == {1, 4, 7, 8, 63, 64, 65, 77, 129} and {p[0] for p in CROSS_PAIRS} == {1, 100, 128, 130}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_extra", [False, True])
@pytest.mark.parametrize("d", [40, 64])
@pytest.mark.parametrize("n_q,n_k", CROSS_PAIRS)
def test_cross_key_and_query_counts(dtype, n_q, n_k, d, with_extra):
    """2 items x 3 heads, ds_scale = 0.4 x scale, every row-major operand pitched with a gap between items, extra_ld = n_k + 3 with NaN in the
    pad, kt zero in columns [n_k, roundup8(n_k)) and NaN in the eight columns after them"""
    a = ab.make_cross_case(dtype, 2, n_q, n_k, 3, d, device=DEV, with_extra=with_extra, weight=0.4, layout="pitched", transpose=_gpu_transpose)
    assert a["extra_ld"] == n_k + 3 and abs(a["ds_scale"] - 0.4 * a["scale"]) < 1e-12 and (a["extra"] is not None) == with_extra
    run_case(a, f"cross nq={n_q} nk={n_k} d={d} extra={with_extra} {_name(dtype)}")


# ---- peaked softmax ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("qmul", [4.0, 8.0])
@pytest.mark.parametrize("kind", ["self", "cross"])
def test_peaked_softmax(dtype, kind, qmul):
    """Q x4 and Q x8 (scores of spread 4 / 8 instead of 1; at x8 most rows hold one probability above 1/2): finite outputs and the unchanged
    tolerances.  The x8 input is the one test_attn_bwd_contract_cpu.py shows to be well conditioned (the fp32 model passes it)."""
    if kind == "self":
        a = ab.make_self_case(dtype, 1, 264, 2, 64, device=DEV, qmul=qmul, transpose=_gpu_transpose)
    else:
        a = ab.make_cross_case(dtype, 1, 264, 264, 2, 64, device=DEV, qmul=qmul, with_extra=True, weight=0.4, transpose=_gpu_transpose)
    for m in run_case(a, f"{kind} peaked x{qmul:g} n=264 d=64 {_name(dtype)}").values():
        assert m["finite"]


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def _refused(a, rc_want, what, edit=None):
    """host validation returns ``rc_want`` with a message and no output byte changes (no launch: the checks run before any)"""
    from theatergen_amd import _lib
    cross = "n_q" in a
    writes = ab.cross_written_region(a) if cross else ab.self_written_region(a)
    masks = lc.LaunchChecker._write_masks(writes)
    for t, _ in masks.values():
        lc._bytes(t).fill_(SENTINEL)
    d, fn = descriptor(a)
    if edit is not None:
        edit(d)
    from theatergen_amd import ops
    rc = fn(C.byref(d), ops._stream())
    torch.cuda.synchronize()
    assert rc == rc_want, f"{what}: returned {rc}, documented {rc_want}"
    assert _lib.lib().tg_last_error(), f"{what}: no error message"
    for t, _ in masks.values():
        assert bool((lc._bytes(t) == SENTINEL).all()), f"{what}: a refused descriptor wrote to its outputs"


@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals_return_the_documented_error_and_write_nothing(dtype):
    mk = dict(device=DEV, transpose=_gpu_transpose)
    _refused(ab.make_self_case(dtype, 1, 60, 1, 64, **mk), TG_ERR_UNSUPPORTED, "self n % 8 != 0")
    _refused(ab.make_self_case(dtype, 1, 64, 1, 80, **mk), TG_ERR_UNSUPPORTED, "self head_dim 80")
    _refused(ab.make_cross_case(dtype, 1, 64, 77, 1, 80, **mk), TG_ERR_UNSUPPORTED, "cross head_dim 80")
    _refused(ab.make_self_case(dtype, 1, 64, 2, 64, **mk), TG_ERR_ARG, "self t_ld < n", lambda d: setattr(d, "t_ld", 56))
    _refused(ab.make_cross_case(dtype, 1, 64, 77, 2, 64, **mk), TG_ERR_ARG, "cross extra_ld < n_k", lambda d: setattr(d, "extra_ld", 76))
    _refused(ab.make_cross_case(dtype, 1, 64, 77, 2, 64, **mk), TG_ERR_ARG, "cross kt pitch below the padded key count",
             lambda d: setattr(d, "t_ld", 72))
    for field in ("q", "k", "v", "dout", "qt", "kt", "doutt", "stats", "dq", "dk", "dv"):
        _refused(ab.make_self_case(dtype, 1, 64, 2, 64, **mk), TG_ERR_ARG, f"self null {field}", lambda d, f=field: setattr(d, f, None))
    for field in ("q", "dout", "k", "v", "kt", "stats", "dq"):
        _refused(ab.make_cross_case(dtype, 1, 64, 77, 2, 64, **mk), TG_ERR_ARG, f"cross null {field}", lambda d, f=field: setattr(d, f, None))


# ---- the materialised fallback (head dims 80 / 160 of SD-1.5's inner levels) ---------------------------------------------------------
def _fallback_tols(dtype):
    """test_backward_gpu.py::test_attention_block_input_gradient's"""
    return (2e-2, 5e-2) if dtype == torch.bfloat16 else (3e-3, 1e-2)


def _count_ops(monkeypatch, names):
    from theatergen_amd import ops
    calls = {n: 0 for n in names}
    for n in names:
        def wrapper(*a, _o=getattr(ops, n), _n=n, **k):
            calls[_n] += 1
            return _o(*a, **k)
        monkeypatch.setattr(ops, n, wrapper)
    return calls


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [64, 264])
def test_materialised_self_attention_input_gradient_head_dim_80(dtype, N, monkeypatch):
    """``backward.attention_input_grad`` at head dim 80 (the recompute kernel refuses it): N = 64 takes the tg_attn_probs branch (at most 256
    keys), N = 264 the scores-GEMM + tg_softmax_rows branch; vs fp64 autograd of the oracle processor"""
    from oracle import attention as oa
    from tests.golden import gen_common as gg
    from theatergen_amd.attention_processor import Attention, AttnProcessor
    from theatergen_amd.backward import attention_input_grad
    g = torch.Generator().manual_seed(80 + N)
    heads, B = 2, 2
    Cc = heads * 80
    l2, mx = _fallback_tols(dtype)
    ws = gg.attn_weights(Cc, Cc, seed=21, with_ip=False)
    wsr = {k: v.to(dtype).double() for k, v in ws.items()}
    h = (torch.randn((B, N, Cc), generator=g)).to(dtype)
    dout = (torch.randn((B * N, Cc), generator=g)).to(dtype)
    attn = Attention(query_dim=Cc, heads=heads, dim_head=80)
    attn.load_state_dict(ws)
    attn = attn.to(DEV, dtype)
    hr = h.double().clone().requires_grad_(True)
    ref = torch.autograd.grad(oa.attn_processor(wsr, heads, hr), hr, dout.double().reshape(B, N, Cc))[0].reshape(B * N, Cc)
    calls = _count_ops(monkeypatch, ("attention_bwd", "attention_bwd_cross", "attn_probs", "softmax_rows", "softmax_bwd_rows"))
    got = attention_input_grad(attn, AttnProcessor(), h.to(DEV).reshape(B * N, Cc), B, N, None, dout.to(DEV), None)
    torch.cuda.synchronize()
    assert calls["attention_bwd"] == 0 and calls["softmax_bwd_rows"] == B * heads
    assert (calls["attn_probs"], calls["softmax_rows"]) == ((1, 0) if N <= 256 else (0, B * heads))
    pm.check(got, ref, f"materialised self-attention input grad d=80 N={N} {dtype}", l2, mx)


@pytest.mark.parametrize("dtype", DTYPES)
def test_materialised_ip_cross_attention_input_gradient_head_dim_80(dtype, monkeypatch):
    """one IP-Adapter cross-attention layer at head dim 80 (77 text keys + 4 image keys, scale 0.4) with the loss gradient ``extra`` on the
    text probabilities, vs fp64 autograd of the oracle processor"""
    from oracle import attention as oa
    from tests.golden import gen_common as gg
    from theatergen_amd.attention_processor import Attention, IPAttnProcessor
    from theatergen_amd.backward import attention_input_grad
    g = torch.Generator().manual_seed(81)
    heads, B, N, T, ctx = 2, 2, 72, 4, 64
    Cc = heads * 80
    l2, mx = _fallback_tols(dtype)
    w = gg.attn_weights(Cc, ctx, seed=22)
    wr = {k: v.to(dtype).double() for k, v in w.items()}
    h = (torch.randn((B, N, Cc), generator=g)).to(dtype)
    enc = (torch.randn((B, 77 + T, ctx), generator=g) * 0.5).to(dtype)
    dout = (torch.randn((B * N, Cc), generator=g)).to(dtype)
    extra = torch.randn(B, heads, N, 77, generator=g) * 0.2
    attn = Attention(query_dim=Cc, cross_attention_dim=ctx, heads=heads, dim_head=80)
    attn.load_state_dict({k: v for k, v in w.items() if "_ip" not in k})
    attn = attn.to(DEV, dtype)
    proc = IPAttnProcessor(hidden_size=Cc, cross_attention_dim=ctx, scale=0.4, num_tokens=T)
    proc.load_state_dict({"to_k_ip.weight": w["to_k_ip.weight"], "to_v_ip.weight": w["to_v_ip.weight"]})
    proc = proc.to(DEV, dtype)
    hr = h.double().clone().requires_grad_(True)
    out, probs = oa.ip_attn_processor(wr, heads, hr, enc.double(), 0.4, T, return_probs=True)
    ref = torch.autograd.grad([out, probs], hr, [dout.double().reshape(B, N, Cc), extra.double()])[0].reshape(B * N, Cc)
    calls = _count_ops(monkeypatch, ("attention_bwd_cross", "attn_probs", "softmax_bwd_rows"))
    got = attention_input_grad(attn, proc, h.to(DEV).reshape(B * N, Cc), B, N, enc.to(DEV), dout.to(DEV), extra.to(DEV))
    torch.cuda.synchronize()
    assert calls["attention_bwd_cross"] == 0 and calls["attn_probs"] == 2 and calls["softmax_bwd_rows"] == 2 * B * heads
    pm.check(got, ref, f"materialised ip cross-attention input grad d=80 {dtype}", l2, mx)
