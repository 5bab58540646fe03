"""CPU: the fp64 restatement of the tg_gemm / tg_attention contracts (tests/gemm_contract.py) pinned against independent torch
formulations of the same operations, and shown to FAIL the comparison the GPU launch tests make when a reference output carries one
of the faults a kernel could have (one tile scaled, one 64-pixel block from the neighbouring image, one column tile without its bias,
V^T written untransposed, one split-K partial counted twice).  No GPU: the reference runs on the operands' device, here the host."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import gemm_contract as gc

BF16 = torch.bfloat16
L2_BF16, MAX_BF16 = 3.0e-3, 1.0e-2          # l2_tol / rel_tol of tests/test_kernels_gpu.py for bf16: what the launch tests use


def rnd(shape, g, scale=1.0, dtype=BF16):
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def f64(t):
    return t.to(torch.float64)


def _tok(x):
    """NCHW -> token-major [B * H * W, C]"""
    B, C, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(B * H * W, C).contiguous()


def _untok(y, B, H, W):
    return y.reshape(B, H, W, -1).permute(0, 3, 1, 2)


# ---- pins: mode 1 --------------------------------------------------------------------------------------------------------------------
CONV_CASES = [
    # B, H, W, c0, c1, N, stride, upsample, pad_mode, act
    (2, 6, 5, 64, 0, 32, 1, 0, 0, 0),
    (2, 7, 6, 64, 0, 16, 2, 0, 0, 1),
    (1, 4, 3, 64, 0, 8, 1, 1, 0, 2),
    (2, 8, 6, 64, 0, 12, 2, 0, 1, 3),
    (2, 5, 5, 64, 128, 24, 1, 0, 0, 0),
]


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_reference_matches_conv2d(case):
    from theatergen_amd.weights_pack import pack_conv3x3
    B, H, W, c0, c1, N, stride, up, pad_mode, act = case
    g = torch.Generator().manual_seed(sum(case))
    C = c0 + c1
    x = rnd((B, C, H, W), g)
    wt = rnd((N, C, 3, 3), g, 1 / math.sqrt(9 * C))
    bias, bvec = rnd((N,), g), rnd((B, N), g)
    xi = F.interpolate(f64(x), scale_factor=2, mode="nearest") if up else f64(x)
    if pad_mode == 1:
        y = F.conv2d(F.pad(xi, (0, 1, 0, 1)), f64(wt), stride=stride)
    else:
        y = F.conv2d(xi, f64(wt), stride=stride, padding=1)
    oh, ow = y.shape[2:]
    res = rnd((B, N, oh, ow), g)
    y = y + f64(bias)[None, :, None, None] + f64(bvec)[:, :, None, None] + f64(res)
    y = gc._act(y, act) * 0.75
    tok = _tok(x)
    args = dict(a0=tok[:, :c0].contiguous(), a1=tok[:, c0:].contiguous() if c1 else None, c0=c0, c1=c1, w=pack_conv3x3(wt),
                M=B * oh * ow, N=N, K=9 * C, mode=1, conv=(B, H, W, oh, ow, stride, up), pad_mode=pad_mode, bias=bias,
                bvec=bvec, rows_per_batch=oh * ow, res=_tok(res), act=act, out_scale=0.75)
    out, out_t = gc.gemm_reference(**args)
    assert out_t is None
    torch.testing.assert_close(_untok(out, B, oh, ow), y, rtol=1e-12, atol=1e-12)


def test_conv_reference_groupnorm_prologue():
    """a_coef / a_silu: conv(round(silu(x * a + d))) with the padding zero AFTER the prologue"""
    from theatergen_amd.weights_pack import pack_conv3x3
    g = torch.Generator().manual_seed(3)
    B, H, W, C, N = 2, 5, 4, 64, 16
    x = rnd((B, C, H, W), g)
    wt = rnd((N, C, 3, 3), g, 1 / math.sqrt(9 * C))
    coef = torch.randn(B, 2, C, generator=g)
    xn = (x.float() * coef[:, 0, :, None, None] + coef[:, 1, :, None, None])
    xn = (xn * torch.sigmoid(xn)).to(BF16)
    y = F.conv2d(f64(xn), f64(wt), padding=1)
    args = dict(a0=_tok(x), w=pack_conv3x3(wt), M=B * H * W, N=N, K=9 * C, mode=1, conv=(B, H, W, H, W, 1, 0), a_coef=coef, a_silu=True)
    out, _ = gc.gemm_reference(**args)
    torch.testing.assert_close(_untok(out, B, H, W), y, rtol=1e-12, atol=1e-12)


# ---- pins: mode 0 epilogues ----------------------------------------------------------------------------------------------------------
def test_geglu_reference_matches_unpacked_formula():
    from theatergen_amd.weights_pack import pack_geglu
    g = torch.Generator().manual_seed(4)
    M, K, inner = 40, 64, 96
    x = rnd((M, K), g)
    w, b = rnd((2 * inner, K), g, 1 / math.sqrt(K)), rnd((2 * inner,), g)
    wp, bp = pack_geglu(w, b)
    h = f64(x) @ f64(w).t() + f64(b)
    want = h[:, :inner] * F.gelu(h[:, inner:]) * 0.5
    out, _ = gc.gemm_reference(a0=x, w=wp, bias=bp, M=M, N=2 * inner, K=K, geglu=True, out_scale=0.5)
    torch.testing.assert_close(out, want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("rows", [False, True])
def test_layernorm_fold_reference_matches_layer_norm_then_linear(rows):
    from theatergen_amd.weights_pack import pack_ln_linear
    g = torch.Generator().manual_seed(5)
    M, K, N = 24, 128, 48
    x = f64(rnd((M, K), g) + 3.0)
    w, b = torch.randn(N, K, generator=g, dtype=torch.float64) / math.sqrt(K), torch.randn(N, generator=g, dtype=torch.float64)
    gamma, beta = 1 + 0.1 * torch.randn(K, generator=g, dtype=torch.float64), 0.1 * torch.randn(K, generator=g, dtype=torch.float64)
    wp, u, v = pack_ln_linear(w, b, gamma, beta)                    # fp64 W' (exact algebra), u / v summed in fp32
    want = F.linear(F.layer_norm(x, (K,), gamma, beta, 1e-5), w, b)
    ln = (u.double(), v.double(), 1e-5)
    if rows:
        mean, var = x.mean(1), x.var(1, unbiased=False)
        rstd = 1 / torch.sqrt(var + 1e-5)
        ln = ln + (torch.stack([rstd, -rstd * mean], 1).contiguous(),)
    out, _ = gc.gemm_reference(a0=x, w=wp, M=M, N=N, K=K, ln=ln)
    torch.testing.assert_close(out, want, rtol=1e-5, atol=1e-5)
    mean, rstd = gc.ln_row_stats(dict(a0=x, M=M, N=N, K=K, ln=ln))
    torch.testing.assert_close(mean, x.mean(1))


def test_split_output_and_batched_a_match_explicit_slicing():
    """a_rows_per_batch / a_batch_stride (rows [s, s + r) of every batch item of a [B, L, K] tensor), padded lda / ldw, and the
    n_split / out_t layout (V^T per batch item with row pitch ldt)"""
    g = torch.Generator().manual_seed(6)
    B, L, K, N, s, r, ns, ldt = 3, 11, 64, 96, 4, 7, 32, 16
    enc = rnd((B, L, K), g)
    w = rnd((N, K), g, 1 / math.sqrt(K))
    full = f64(enc[:, s:s + r].reshape(B * r, K)) @ f64(w).t()
    out, out_t = gc.gemm_reference(a0=enc[:, s:], w=w, M=B * r, N=N, K=K, a_rows_per_batch=r, a_batch_stride=L * K, n_split=ns,
                                   out_t=torch.empty(B * (N - ns) * ldt, dtype=BF16), ldt=ldt, rows_per_batch=r)
    torch.testing.assert_close(out, full[:, :ns])
    torch.testing.assert_close(out_t, full[:, ns:].reshape(B, r, N - ns).transpose(1, 2))
    # padded pitches: views [:, :K] of wider buffers
    M = 9
    abuf, wbuf = rnd((M, K + 24), g), rnd((N, K + 8), g)
    out, _ = gc.gemm_reference(a0=abuf[:, :K], w=wbuf[:, :K], M=M, N=N, K=K, lda=K + 24, ldw=K + 8)
    torch.testing.assert_close(out, f64(abuf[:, :K]) @ f64(wbuf[:, :K]).t())


def test_regions_of_a_column_view():
    """written_region of an ``out`` that is a column view of a wider buffer covers exactly those columns; read_extents
    follow the pitches, and a descriptor that reads past its operand's storage raises"""
    g = torch.Generator().manual_seed(7)
    M, K, N = 10, 64, 32
    buf = torch.zeros(M, 3 * N, dtype=BF16)
    a = dict(a0=rnd((M, K), g), w=rnd((N, K), g), M=M, N=N, K=K, out=buf[:, N:2 * N], n_split=16, out_t=torch.zeros(2, 16, 8, dtype=BF16),
             ldt=8, rows_per_batch=5)
    wr = gc.written_region(a)
    mask = torch.zeros(buf.untyped_storage().nbytes(), dtype=torch.bool)
    wr[0].byte_view(mask).fill_(True)
    want = torch.zeros(M, 3 * N, 2, dtype=torch.bool)
    want[:, N:N + 16] = True
    assert torch.equal(mask, want.reshape(-1))
    assert wr[1].sizes == (2, 16, 5) and wr[1].strides == (128, 8, 1)
    ranges = {r.name: r.byte_range() for r in gc.read_extents(a)}
    assert ranges["a0"] == (0, M * K * 2) and ranges["w"] == (0, N * K * 2)
    with pytest.raises(RuntimeError):
        gc.gemm_reference(**dict(a, M=M + 1))


# ---- pins: attention -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["self_causal", "two_segments_mask", "w1_dev"])
def test_attention_reference_matches_explicit_softmax(variant):
    g = torch.Generator().manual_seed(8)
    B, H, D, n, L0, L1 = 2, 3, 16, 13, 9, 5
    if variant == "self_causal":
        L0 = n
    HD = H * D
    # q and k in one [B, n, 2 HD] buffer (row pitch 2 HD), V^T with a padded pitch
    qk = rnd((B, n, 2 * HD), g)
    k0 = rnd((B, L0, HD), g) if variant != "self_causal" else None
    vt0 = rnd((B, HD, 16), g)
    k1, vt1 = rnd((B, L1, HD), g), rnd((B, HD, 8), g)
    mask = torch.randn(B, 1, n, L0, generator=g) if variant == "two_segments_mask" else None
    w1 = 0.7
    w1_dev = torch.tensor([0.4]) if variant == "w1_dev" else None
    kk = qk[:, :, HD:] if k0 is None else k0
    args = dict(q=qk, q_ld=2 * HD, q_bs=n * 2 * HD, k0=kk, k0_ld=kk.stride(1), k0_bs=kk.stride(0), vt0=vt0, vt0_ld=16, vt0_bs=HD * 16, len0=L0,
                batch=B, heads=H, head_dim=D, n_q=n, scale=D ** -0.5, out=None, out_ld=HD, out_bs=n * HD, causal=variant == "self_causal",
                mask=mask, w1_dev=w1_dev)
    if variant != "self_causal":
        args.update(k1=k1, k1_ld=HD, k1_bs=L1 * HD, vt1=vt1, vt1_ld=8, vt1_bs=HD * 8, len1=L1, w1=w1)
    else:
        args.update(len1=0)
    got = gc.attention_reference(q_chunk=5, **args)

    def heads(t, L):          # [B, L, HD] -> [B, H, L, D]
        return f64(t).reshape(B, L, H, D).permute(0, 2, 1, 3)
    q = heads(qk[:, :, :HD], n)
    s0 = q @ heads(kk, L0).transpose(-1, -2) * D ** -0.5
    if mask is not None:
        s0 = s0 + f64(mask)
    if variant == "self_causal":
        s0 = s0 + torch.triu(torch.full((n, n), float("-inf"), dtype=torch.float64), 1)
    o = torch.softmax(s0, -1) @ heads(vt0[:, :, :L0].transpose(1, 2), L0)
    if variant != "self_causal":
        s1 = q @ heads(k1, L1).transpose(-1, -2) * D ** -0.5
        o = o + (float(w1_dev[0]) if w1_dev is not None else w1) * (torch.softmax(s1, -1) @ heads(vt1[:, :, :L1].transpose(1, 2), L1))
    torch.testing.assert_close(got, o.permute(0, 2, 1, 3).reshape(B, n, HD), rtol=1e-12, atol=1e-12)


def test_gn_partials_reference():
    g = torch.Generator().manual_seed(9)
    B, hw, C, G = 2, 128, 64, 8
    out = rnd((B * hw, C), g)
    p = gc.gn_partials_reference(out, G, B, hw)
    x = f64(out).reshape(B, hw, G, C // G)
    torch.testing.assert_close(p[1, 1, 3, 0], x[1, 64:, 3].sum())
    torch.testing.assert_close(p[0, 0, 5, 1], (x[0, :64, 5] ** 2).sum())


# ---- the comparison bites ------------------------------------------------------------------------------------------------------------
def _production_like(seed=10):
    """a 16384 x 640 projection with bias (the shape of the 32 x 32 level's proj_in / to_out at CFG batch 16): fp64 reference, the bf16
    result a correct kernel stores, and the pieces the faults are built from"""
    g = torch.Generator().manual_seed(seed)
    M, N, K = 16384, 640, 128
    a, w, bias = rnd((M, K), g), rnd((N, K), g, 1 / math.sqrt(K)), rnd((N,), g, 0.5)
    ref, _ = gc.gemm_reference(a0=a, w=w, bias=bias, M=M, N=N, K=K)
    return dict(a=a, w=w, bias=bias, ref=ref, good=ref.to(BF16), M=M, N=N, K=K)


def _fails(got, ref):
    ok, m = gc.compare(got, ref, L2_BF16, MAX_BF16)
    return not ok, m


def test_correct_output_passes():
    p = _production_like()
    ok, m = gc.compare(p["good"], p["ref"], L2_BF16, MAX_BF16)
    assert ok, m


def test_fault_one_tile_scaled():
    p = _production_like()
    bad = p["good"].to(torch.float64)
    bad[128:256, 256:384] *= 1.02
    failed, m = _fails(bad.to(BF16), p["ref"])
    assert failed, m
    # the whole-tensor numbers alone miss it (a 1/640 share of the output): the tile-local one is what catches it
    assert m["rel_l2"] < L2_BF16 and m["tile_rel_l2"] > 2 * L2_BF16, m


def test_fault_block_from_neighbouring_image():
    """a conv output [2 images x 64 x 64 pixels, 320]: one 64-pixel block of image 1 holds image 0's values"""
    g = torch.Generator().manual_seed(11)
    B, H, W, C, N = 2, 64, 64, 64, 320
    x, wt = rnd((B * H * W, C), g), rnd((N, 9 * C), g, 1 / math.sqrt(9 * C))
    ref, _ = gc.gemm_reference(a0=x, w=wt, M=B * H * W, N=N, K=9 * C, mode=1, conv=(B, H, W, H, W, 1, 0))
    bad = ref.clone()
    hw = H * W
    bad[hw + 640:hw + 704] = ref[640:704]
    assert _fails(bad.to(BF16), ref)[0]
    assert not _fails(ref.to(BF16), ref)[0]


def test_fault_bias_of_one_column_tile_dropped():
    p = _production_like()
    bad = p["good"].to(torch.float64)
    bad[:, 320:480] -= f64(p["bias"][320:480])
    failed, m = _fails(bad.to(BF16), p["ref"])
    assert failed, m


def test_fault_out_t_untransposed():
    g = torch.Generator().manual_seed(12)
    B, r, K, N, ns = 4, 256, 64, 256, 128
    x, w = rnd((B * r, K), g), rnd((N, K), g, 1 / math.sqrt(K))
    _, out_t = gc.gemm_reference(a0=x, w=w, M=B * r, N=N, K=K, n_split=ns, out_t=torch.empty(B * (N - ns) * r, dtype=BF16), ldt=r,
                                 rows_per_batch=r)
    # the V^T columns stored as [B, rows, N - n_split] into the [B, N - n_split, ldt] buffer
    wrong = out_t.transpose(1, 2).contiguous().reshape(B, N - ns, r)
    assert _fails(wrong.to(BF16), out_t)[0]
    assert not _fails(out_t.to(BF16), out_t)[0]


def test_fault_split_partial_counted_twice():
    """the 8 x 8 level's weight-streaming conv split 4 ways over K: one tile's second partial added twice"""
    p = _production_like()
    a, w, K = p["a"], p["w"], p["K"]
    part = f64(a[:128, 32:64]) @ f64(w[128:256, 32:64]).t()        # K range [32, 64) of tile (0, 1)
    bad = p["good"].to(torch.float64)
    bad[:128, 128:256] += part
    failed, m = _fails(bad.to(BF16), p["ref"])
    assert failed, m
