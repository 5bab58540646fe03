"""GPU: the CFG pair's shared UNet prefix.

With classifier-free guidance the two halves of a UNet call start from the same latents (``torch.cat([latents] * 2)``, models/pipelines.py:411-414) and
the same timestep; they first differ at the first reader of ``encoder_hidden_states``.  ``UNet2DConditionModel.forward(shared_pair=True)`` runs that prefix
(conv_in, down_blocks[0].resnets[0], the first transformer's front and attn1) on half the batch, and the three producers whose results the full batch
consumes leave both halves behind: ``tg_rc_linear_dup`` and ``tg_conv_in_dup`` store every row twice from their epilogues, a tg_gemm conv is followed
by one ``tg_dup_rows`` copy (the slab conv has no registers to spare for a second store, profiles/cfg_share_findings.md).

Every kernel of the prefix treats batch items independently, so the checks are exact wherever the same kernels run:
  1. each producer with the second destination: rows [0, M) are the bits of the plain launch, rows [M, 2M) equal them, canary rows around the buffer and
     the GroupNorm partial sums are untouched / unchanged;
  2. refusals (a kernel that cannot store twice never ignores the offset) and the pitched-source copy;
  3. / 4. UNet forward with ``shared_pair`` on vs off — level 0 of the SD-1.5 plan on the row-chain path, and the tiny plan on the LDS-tiled path — with the
     launch records (``ops.gemm_profile_start / stop``) showing which launches ran on half the rows: bit-identical where both arms ran the same kernels
     (asserted outright for the cases where that is known), else within ``launch_check.l2_tol``;
  5. ``DenoiseEngine`` histories with TG_CFG_SHARE=0 (child process: the switch is read at import) and the default are equal; an engine with per-item added
     conditioning (SDXL's text_time) leaves sharing off.
"""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 24          # rows in front of and behind the pair buffer
MARK = 1234.0        # exactly representable in bf16 and fp16


def _pair_buffer(M, N, dtype):
    big = torch.full((2 * M + 2 * CANARY, N), MARK, dtype=dtype, device=DEV)
    return big, big[CANARY:CANARY + 2 * M]


def _check_pair(big, pair, plain, M, what):
    assert torch.equal(pair[:M], plain), f"{what}: the first copy differs from the plain launch"
    assert torch.equal(pair[M:], plain), f"{what}: the second copy differs from the first"
    assert bool((big[:CANARY] == MARK).all()) and bool((big[CANARY + 2 * M:] == MARK).all()), f"{what}: rows outside the pair buffer were written"


# ---- 1. one case per producer ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M", [256, 250, 301])       # one whole workgroup; a masked row tail inside the last wave; a second, part-filled workgroup
def test_rc_linear_stores_both_halves(dtype, M):
    from theatergen_amd import ops
    from theatergen_amd.weights_pack import rc_pack
    N, K = 320, 320
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(M, K, generator=g) * 1.5 + 0.3).to(dtype).to(DEV)
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(dtype).to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    r = torch.randn(M, N, generator=g).to(dtype).to(DEV)
    wpk = rc_pack(W, bias)
    plain = ops.rc_linear(x, wpk, N, res=r)
    big, pair = _pair_buffer(M, N, dtype)
    got = ops.rc_linear(x, wpk, N, res=r, pair_out=pair)
    assert got.data_ptr() == pair.data_ptr()
    _check_pair(big, pair, plain, M, f"rc_linear {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("h,w", [(16, 16), (15, 15), (24, 8)])      # 256 pixels = two whole workgroups' worth; 225: a masked tail (npix % 32 = 1); 192: npix % 128 = 64
def test_conv_in_stores_both_halves(dtype, h, w):
    from theatergen_amd import _lib, ops
    from theatergen_amd.weights_pack import pack_conv3x3
    g = torch.Generator().manual_seed(6)
    cout, M = 320, h * w
    x = torch.randn(1, 4, h, w, generator=g).to(DEV)                    # fp32 sample: the head / tail split of the kernel is on
    wt = pack_conv3x3((torch.randn(cout, 4, 3, 3, generator=g) * 0.2).to(dtype).to(DEV))
    bias = torch.randn(cout, generator=g).to(dtype).to(DEV)
    plain = ops.conv_in(x, wt, bias, cout, dtype)
    L = _lib.lib()
    assert L.tg_conv_in_takes_dup(4, cout) == 1
    big, pair = _pair_buffer(M, cout, dtype)
    _lib.check(L.tg_conv_in_dup(ops._dt(pair), x.data_ptr(), 2, 1, 4, h, w, wt.data_ptr(), bias.data_ptr(), cout, pair.data_ptr(), M * cout,
                                torch.cuda.current_stream().cuda_stream))
    _check_pair(big, pair, plain, M, f"conv_in {dtype}")
    # through ops: a pair batch computes its first half only and returns both
    full = ops.conv_in(torch.cat([x, x]), wt, bias, cout, dtype, pair=True)
    assert torch.equal(full[:M], plain) and torch.equal(full[M:], plain)
    # a problem the matrix-core kernel does not take (cout = 64) goes through the copy
    wt2, b2 = wt[:64].contiguous(), bias[:64].contiguous()
    p2 = ops.conv_in(x, wt2, b2, 64, dtype)
    f2 = ops.conv_in(torch.cat([x, x]), wt2, b2, 64, dtype, pair=True)
    assert torch.equal(f2[:M], p2) and torch.equal(f2[M:], p2)


def _smallest_slab_conv(dtype):
    """the smallest 320 -> 320 stride-1 conv (whole images of 16 / 32 / 64 pixels square) the planner gives to the slab kernel without a K split — the kernel
    of the flagship prefix's convs, with GroupNorm partial sums in its epilogue"""
    from theatergen_amd import ops
    probe = torch.empty(16, dtype=dtype, device=DEV)
    for M, b, s in sorted((b * s * s, b, s) for s in (16, 32, 64) for b in range(1, 129)):
        plan = ops.gemm(probe, probe, M, 320, 2880, mode=1, c0=320, conv=(b, s, s, s, s, 1, 0), plan_only=True)
        if plan[3] == 4 and plan[2] == 1:
            return b, s
    raise AssertionError("no candidate geometry runs on the unsplit slab kernel")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("full_epilogue", [True, False])
def test_slab_conv_pair_out_is_the_copy(dtype, full_epilogue):
    from theatergen_amd import ops
    from theatergen_amd.weights_pack import pack_conv3x3
    b, s = _smallest_slab_conv(dtype)
    C_, M = 320, b * s * s
    g = torch.Generator().manual_seed(7)
    x = torch.randn(M, C_, generator=g).to(dtype).to(DEV)
    wt = pack_conv3x3((torch.randn(C_, C_, 3, 3, generator=g) / (9 * C_) ** 0.5).to(dtype).to(DEV))
    kw = dict(bias=torch.randn(C_, generator=g).to(dtype).to(DEV))
    gn_a = gn_b = None
    if full_epilogue:
        kw.update(res=torch.randn(M, C_, generator=g).to(dtype).to(DEV), out_scale=0.75,
                  bvec=torch.randn(b, C_, generator=g).to(dtype).to(DEV), rows_per_batch=s * s)
        gn_a, gn_b = {"groups": 32}, {"groups": 32}
    plain = ops.conv3x3(x, wt, b, s, s, C_, **kw, **({"gn_out": gn_a} if gn_a else {}))
    big, pair = _pair_buffer(M, C_, dtype)
    rec = []
    ops.gemm_profile_start()
    try:
        got = ops.conv3x3(x, wt, b, s, s, C_, pair_out=pair, **kw, **({"gn_out": gn_b} if gn_b else {}))
        torch.cuda.synchronize()
    finally:
        rec = ops.gemm_profile_stop()
    assert got.data_ptr() == pair.data_ptr()
    assert len(rec) == 1 and rec[0]["kernel"].startswith("conv_slab") and rec[0]["splits"] == 1, rec
    _check_pair(big, pair, plain, M, f"slab conv {b} x {s} x {s} {dtype}")
    if full_epilogue:
        assert "partials" in gn_a and "partials" in gn_b
        assert torch.equal(gn_a["partials"], gn_b["partials"]), "GroupNorm partial sums changed with the pair output"


# ---- 2. refusal and fallback ---------------------------------------------------------------------------------------------------------------
def test_kernels_without_the_second_store_refuse_the_offset():
    from theatergen_amd import _lib, ops
    L = _lib.lib()
    dtype = torch.bfloat16
    st = torch.cuda.current_stream().cuda_stream
    # conv_in on the fp32-FMA kernels (cout = 64): argument error, nothing written
    s = torch.randn(1, 4, 16, 16, device=DEV)
    w64 = torch.randn(64, 36).to(dtype).to(DEV)
    o64 = torch.full((2 * 256, 64), MARK, dtype=dtype, device=DEV)
    assert L.tg_conv_in_dup(0, s.data_ptr(), 2, 1, 4, 16, 16, w64.data_ptr(), None, 64, o64.data_ptr(), 256 * 64, st) == -1
    torch.cuda.synchronize()
    assert bool((o64 == MARK).all())
    # a plain GEMM through ops: served by the copy
    M, N, K = 256, 64, 64
    x = torch.randn(M, K).to(dtype).to(DEV)
    W = torch.randn(N, K).to(dtype).to(DEV)
    pair = torch.full((2 * M, N), MARK, dtype=dtype, device=DEV)
    plain = ops.linear(x, W)
    ops.gemm(x, W, M, N, K, pair_out=pair)
    assert torch.equal(pair[:M], plain) and torch.equal(pair[M:], plain)


@pytest.mark.parametrize("dtype", DTYPES)
def test_dup_rows_on_a_pitched_source_is_exact(dtype):
    from theatergen_amd import ops
    rows, cols, ld = 77, 72, 104                                       # odd row count, more than one block's worth of vectors, pitch > cols
    src = torch.randn(rows, ld).to(dtype).to(DEV)
    big = torch.full((rows + 2, cols), MARK, dtype=dtype, device=DEV)
    ops.dup_rows(src[:, :cols], big[1:rows + 1])
    assert torch.equal(big[1:rows + 1], src[:, :cols]) and bool((big[0] == MARK).all()) and bool((big[-1] == MARK).all())
    with pytest.raises(RuntimeError):
        ops.dup_rows(src[:, :cols], src[:, :cols])                     # dst must be dense


# ---- 3. / 4. UNet forward, shared vs not ------------------------------------------------------------------------------------------------------
def _forward_recorded(unet, x, t, enc, shared):
    """-> (UNet output fp32, output of down_blocks[0] = what its downsampler is handed, launch records)"""
    from theatergen_amd import ops
    from theatergen_amd import unet as U
    seen = []
    orig = U.Downsample2D.run

    def spy(self, x, res=None):
        seen.append(x.t.clone())
        return orig(self, x, res=res)
    U.Downsample2D.run = spy
    ops.gemm_profile_start()
    try:
        out = unet(x, t, enc, shared_pair=shared, return_dict=False, out_dtype=torch.float32)[0]
        torch.cuda.synchronize()
    finally:
        rec = ops.gemm_profile_stop()
        U.Downsample2D.run = orig
    return out, seen[0], rec


def _compare_shared(unet, x1, enc, dtype, what, block0_only=False, expect_same=None):
    """x1: one half [n, 4, h, w]; enc: [2 n, L, D] with different halves.  -> (records of the shared run, records of the plain run)"""
    from tests import launch_check as lc
    from tests import parity_metrics as pm
    n, _, h, w = x1.shape
    x = torch.cat([x1, x1]).contiguous()
    assert not torch.equal(enc[:n], enc[n:])
    ref, ref_b0, rec0 = _forward_recorded(unet, x, 981, enc, False)
    got, got_b0, rec1 = _forward_recorded(unet, x, 981, enc, True)
    assert got_b0.shape == ref_b0.shape == (2 * n * h * w, unet.config.block_out_channels[0])
    half, full = n * h * w, 2 * n * h * w
    # plain run: nothing at half the rows
    assert all(r["M"] != half for r in rec0), [r for r in rec0 if r["M"] == half]
    # shared run: the launches at half the rows are one contiguous block that ends with attn1's to_out projection (the launch behind the self-attention) ...
    idx = [i for i, r in enumerate(rec1) if r["M"] == half]
    sa = next(i for i, r in enumerate(rec1) if r.get("attention") and "self" in r["kernel"])
    assert idx and idx == list(range(idx[0], sa + 2)), (idx, sa, [(r["kernel"], r["M"]) for r in rec1[:sa + 3]])
    assert len(idx) >= 4                                             # conv1, conv2, (front / projections), attention, to_out
    # ... nothing ran on the full level-0 rows before it, and everything after attn1 ran on the full batch exactly as without sharing
    assert all(r["M"] != full for r in rec1[:sa + 2])
    key = lambda r: (r["kernel"], r["splits"], r["M"], r["N"], r["K"])
    sa0 = next(i for i, r in enumerate(rec0) if r.get("attention") and "self" in r["kernel"])
    assert [key(r) for r in rec1[sa + 2:]] == [key(r) for r in rec0[sa0 + 2:]]
    same = [(r["kernel"], r["splits"]) for r in rec1] == [(r["kernel"], r["splits"]) for r in rec0]
    print(f"{what}: {len(idx)} launches at half the rows, same kernels in both arms: {same}, max abs diff {float((got - ref).abs().max()):.3e}")
    if expect_same is not None:
        assert same == expect_same, [(a["kernel"], a["splits"], b["kernel"], b["splits"]) for a, b in zip(rec1, rec0) if (a["kernel"], a["splits"]) != (b["kernel"], b["splits"])]
    if same:
        assert torch.equal(got_b0, ref_b0) and torch.equal(got, ref), f"{what}: same kernels, different bits"
    elif block0_only:
        # other kernels for the half-batch prefix (the planner looks at M): the block's output moves by a launch's rounding noise
        pm.check(got_b0.float().cpu(), ref_b0.float().cpu(), what + " (down_blocks[0] output)", lc.l2_tol(dtype), lc.rel_tol(dtype))
    else:
        pm.check(got.cpu(), ref.cpu(), what, lc.l2_tol(dtype), lc.rel_tol(dtype))
    return rec1, rec0


def _level0_cfg():
    """conv_in + down_blocks[0] of the SD-1.5 plan (320 channels, 8 heads of 40, 768-wide text) on top of the smallest second level that closes the UNet"""
    from theatergen_amd.config import UNetConfig
    return UNetConfig(name="sd15_level0", sample_size=32, block_out_channels=(320, 640), down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"),
                      up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"), layers_per_block=1)


@pytest.fixture(scope="module")
def level0_unets():
    from tests.test_hotpath_gpu import _build
    cfg = _level0_cfg()
    return cfg, {dt: _build(cfg, dt, seed=3)[0] for dt in DTYPES}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 2])
def test_level0_block_on_the_row_chain_path(level0_unets, monkeypatch, dtype, n):
    from theatergen_amd import rowchain
    cfg, unets = level0_unets
    # the row-chain kernels are selected by row count (a full chip of 128-token workgroups at the flagship shape): lowered so that one 32 x 32 image takes them
    monkeypatch.setattr(rowchain, "MIN_ROWS_CHAIN", 1024)
    monkeypatch.setattr(rowchain, "MIN_ROWS", 1024)
    g = torch.Generator().manual_seed(40 + n)
    x1 = torch.randn(n, 4, 32, 32, generator=g).to(DEV, dtype)
    enc = (torch.randn(2 * n, 81, cfg.cross_attention_dim, generator=g) * 0.5).to(DEV, dtype)
    # one image per half: both arms run the same kernels (2048 / 1024 rows), so the bits are equal; two per half: the convs cross a planner threshold
    # (4096 rows: the LDS-halo kernel), so the block's output is compared within the launch tolerance
    rec1, _ = _compare_shared(unets[dtype], x1, enc, dtype, f"level 0, pair 2 x {n}, {dtype}", block0_only=True, expect_same=(n == 1))
    names = [r["kernel"] for r in rec1]
    half = n * 1024
    assert any(k.startswith("rc_front_kernel") and r["M"] == half for k, r in zip(names, rec1)), names[:12]
    assert any(k.startswith("rc_linear_kernel") and r["M"] == half for k, r in zip(names, rec1)), names[:12]
    assert any(k.startswith("rc_xattn_kernel") and r["M"] == 2 * half for k, r in zip(names, rec1)), names[:12]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant,n", [("conv", 1), ("conv", 2), ("linear", 1)])
def test_tiny_plan_whole_unet(dtype, variant, n):
    from tests.test_hotpath_gpu import _build
    from theatergen_amd import config
    cfg = config.tiny(linear=variant == "linear")
    unet, _ = _build(cfg, dtype)
    g = torch.Generator().manual_seed(50 + n)
    x1 = torch.randn(n, 4, 16, 16, generator=g).to(DEV, dtype)
    enc = (torch.randn(2 * n, 81, cfg.cross_attention_dim, generator=g) * 0.5).to(DEV, dtype)
    _compare_shared(unet, x1, enc, dtype, f"tiny {variant}, pair 2 x {n}, {dtype}")
    if n == 1:
        x3 = torch.randn(3, 4, 16, 16, generator=g).to(DEV, dtype)
        e3 = torch.zeros(3, 81, cfg.cross_attention_dim, device=DEV, dtype=dtype)
        with pytest.raises(ValueError):
            unet(x3, 981, e3, shared_pair=True)
        unet(x3, 981, e3)                                            # an odd batch is fine without the claim


# ---- 5. engine --------------------------------------------------------------------------------------------------------------------------
_CHILD = r"""
import sys, torch
sys.path.insert(0, {root!r})
from tests.test_cfg_share_gpu import _engine_history
torch.save(_engine_history(torch.float16).cpu(), sys.argv[1])
"""


def _engine_history(dtype):
    from tests.test_hotpath_gpu import _build
    from theatergen_amd import config
    from theatergen_amd.pipelines import DenoiseEngine
    cfg = config.tiny()
    unet, _ = _build(cfg, dtype)
    g = torch.Generator().manual_seed(23)
    lat = torch.randn(2, 4, 16, 16, generator=g)
    enc = (torch.randn(4, 81, cfg.cross_attention_dim, generator=g) * 0.5).to(DEV, dtype)
    eng = DenoiseEngine(unet, None, n_img=2, height=128, width=128, num_inference_steps=3, guidance_scale=7.5, enc_len=81, use_graph=True)
    eng.set_conditioning(enc)
    return eng.run(lat).clone()


def _spy_shared(monkeypatch):
    from theatergen_amd.unet import UNet2DConditionModel
    seen = []
    orig = UNet2DConditionModel.forward

    def spy(self, *a, **kw):
        seen.append(bool(kw.get("shared_pair", False)))
        return orig(self, *a, **kw)
    monkeypatch.setattr(UNet2DConditionModel, "__call__", spy)
    return seen


def test_engine_history_equals_the_unshared_one(tmp_path, monkeypatch):
    from theatergen_amd import unet as U
    assert U._CFG_SHARE, "the suite runs with the default switches"
    path = str(tmp_path / "hist_share0.pt")
    env = dict(os.environ, TG_CFG_SHARE="0")
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT), path], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    ref = torch.load(path)
    seen = _spy_shared(monkeypatch)
    got = _engine_history(torch.float16).cpu()
    assert seen and all(seen), "the engine owns model_in and has no added conditioning: it claims the pair"
    assert got.shape == ref.shape == (4, 2, 4, 16, 16)
    assert torch.equal(got, ref), f"history differs from TG_CFG_SHARE=0: max abs {float((got - ref).abs().max()):.3e}"


def test_engine_with_added_conditioning_leaves_sharing_off(monkeypatch):
    from tests.test_hotpath_gpu import _build
    from theatergen_amd import config
    from theatergen_amd.pipelines import DenoiseEngine
    dtype = torch.float16
    cfg = config.tiny(xl=True)
    unet, _ = _build(cfg, dtype)
    g = torch.Generator().manual_seed(29)
    lat = torch.randn(1, 4, 16, 16, generator=g)
    enc = (torch.randn(2, 81, cfg.cross_attention_dim, generator=g) * 0.5).to(DEV, dtype)
    added = {"text_embeds": torch.randn(2, 64, generator=g).to(DEV, dtype), "time_ids": torch.tensor([[128., 128., 0., 0., 128., 128.]] * 2, device=DEV)}
    seen = _spy_shared(monkeypatch)
    eng = DenoiseEngine(unet, None, n_img=1, height=128, width=128, num_inference_steps=2, guidance_scale=5.0, enc_len=81, use_graph=False)
    eng.set_conditioning(enc, added)
    h = eng.run(lat)
    assert seen and not any(seen)
    assert bool(torch.isfinite(h).all())
