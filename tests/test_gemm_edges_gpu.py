"""GPU: the branches tg_gemm takes on operand alignment and pitch (tg_gemm_route.hip::epi_lds_of, pp_eligible,
slab_two_wave, slab_gn_partial_blocks), which the production plans never reach: out / res / bias / bvec 8-byte (not 16-byte) aligned,
ldc / ldres / ldbvec odd multiples of 4, an n_split that is a multiple of 4 but not of 64.  Every launch goes through
``tests.launch_check`` (fp64 contract reference, read extents, overlap, stray writes, NaN replay).  Only descriptors the validator accepts
are launched; a0 / a1 / w, the workspace and the LayerNorm vectors stay 16-byte aligned."""
import math

import pytest
import torch

from tests import launch_check as lc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16 = torch.bfloat16
VARIANTS = ["aligned", "offset4", "odd_pitch", "n_split"]


def _rows(g, M, cols, ld, off, scale=1.0):
    """[M, cols] view with row pitch ld, ``off`` elements into a random buffer (the rest of the buffer: values the launch must keep)"""
    base = (torch.randn(M * ld + off + 8, generator=g) * scale).to(BF16).to(DEV)
    return base[off:off + M * ld].view(M, ld)[:, :cols]


def _epilogue(g, variant, M, N, B):
    off = 4 if variant == "offset4" else 0
    ld = N + 4 if variant == "odd_pitch" else N              # N % 8 == 0 here: N + 4 is an odd multiple of 4
    bias = _rows(g, 1, N, N, off)[0]
    bvec = _rows(g, B, N, ld, off)
    res = _rows(g, M, N, ld, off)
    kw = dict(bias=bias, bvec=bvec, rows_per_batch=M // B, res=res, out_scale=0.5)
    if variant == "n_split":
        ns = N - 92 if (N - 92) % 64 else N - 96             # a multiple of 4, not of 64
        assert ns % 4 == 0 and ns % 64 != 0
        rpb = M // B
        ldt = (rpb + 7) // 8 * 8
        kw.update(n_split=ns, out_t=torch.full((B, N - ns, ldt), 3.0, dtype=BF16, device=DEV), ldt=ldt, out=_rows(g, M, ns, ns, 0))
    else:
        kw["out"] = _rows(g, M, N, ld, off)
    return kw


def _launch(monkeypatch, fn, *args, **kw):
    """one launch through the contract checker; -> (output, plan)"""
    plan = fn(*args, plan_only=True, **kw)
    chk = lc.LaunchChecker("edges").install(monkeypatch)
    try:
        out = fn(*args, **kw)
    finally:
        monkeypatch.undo()
    assert chk.launches == 1 and len(chk.metrics) == 1
    return out, plan


# ---- plain GEMM: the tile configurations the planner / force_tile reach ---------------------------------------------------------------
LINEAR = [
    # M, N, K, force_tile, force_split_k
    (512, 320, 320, 0, 0),          # 128 x 128 (three 32-wide K stages: K <= 640)
    (512, 320, 1280, 0, 0),         # 128 x 128, two 64-wide stages
    (512, 320, 320, 2, 0),          # 64 x 64
    (512, 320, 320, 3, 0),          # 128 x 64
    (512, 320, 320, 4, 0),          # 64 x 128
    (1024, 320, 640, 3, 3),         # K split 3 ways: partials through the workspace, reduce-kernel epilogue
    (2048, 640, 640, 21, 0),        # 128 x 160, three stages
    (2048, 640, 640, 23, 0),        # 128 x 160, two stages
]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", LINEAR)
def test_linear_alignment_and_pitch(monkeypatch, case, variant):
    from theatergen_amd import ops
    M, N, K, ft, fs = case
    g = torch.Generator().manual_seed(M + N + K + ft)
    a = _rows(g, M, K, K, 0)
    w = _rows(g, N, K, K, 0, 1 / math.sqrt(K))
    kw = _epilogue(g, variant, M, N, 4)
    if ft in (21, 23) and variant == "n_split":
        pytest.skip("the 128 x 160 tiles take no n_split")
    out, plan = _launch(monkeypatch, ops.linear, a, w, force_tile=ft, force_split_k=fs, **kw)
    assert plan[3] == 0


# ---- ping-pong tiles: the misaligned / odd-pitch variants must not get kind 7 -------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", [(8192, 1536, 640), (16384, 640, 640)])
def test_pingpong_declines_misaligned_epilogue_operands(monkeypatch, shape, variant):
    from theatergen_amd import ops
    M, N, K = shape
    g = torch.Generator().manual_seed(M + N)
    a = _rows(g, M, K, K, 0)
    w = _rows(g, N, K, K, 0, 1 / math.sqrt(K))
    kw = _epilogue(g, variant, M, N, 8)
    out, plan = _launch(monkeypatch, ops.linear, a, w, **kw)
    if variant == "aligned":
        assert plan[3] == 7
    elif variant in ("offset4", "odd_pitch"):
        assert plan[3] != 7, plan
    else:      # n_split % 64 != 0: not on the 256-wide tiles; the 256 x 160 ones need n_split % 80 == 0
        assert plan[3] != 7 or (plan[1] == 160 and kw["n_split"] % 80 == 0), plan


# ---- conv: halo, slab (two-wave and one-wave), implicit GEMM -------------------------------------------------------------------------
CONV = [
    # B, H, W, cin, cout, stride, force_tile, expected kind
    (2, 64, 64, 320, 320, 1, 0, 2),      # LDS-halo conv
    (2, 32, 32, 320, 320, 2, 0, 1),      # stride 2: implicit-GEMM conv
    (2, 64, 64, 320, 320, 1, 11, 4),     # slab conv, whole 64-wide rows (two-wave kernel when epi_lds holds)
    (2, 16, 96, 320, 320, 1, 11, 4),     # slab conv, 32-pixel patches
]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", CONV)
def test_conv_alignment_and_pitch(monkeypatch, case, variant):
    from theatergen_amd import ops
    from theatergen_amd.weights_pack import pack_conv3x3
    B, H, W, cin, cout, stride, ft, kind = case
    if variant == "n_split" and kind != 1:
        pytest.skip("n_split: the slab / halo kernels do not write transposed columns")
    g = torch.Generator().manual_seed(B + H + W + cin + stride + ft)
    x = _rows(g, B * H * W, cin, cin, 0)
    wp = pack_conv3x3(torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin)).to(BF16).to(DEV)
    oh, ow = (H - 1) // stride + 1, (W - 1) // stride + 1
    kw = _epilogue(g, variant, B * oh * ow, cout, B)
    gn = {"groups": 32} if kind == 4 and stride == 1 and W == 64 else None
    if gn is not None:
        kw["gn_out"] = gn
    out, plan = _launch(monkeypatch, ops.conv3x3, x, wp, B, H, W, cin, stride=stride, force_tile=ft, **kw)
    assert plan[3] == kind, plan
    if gn is not None:
        if variant == "aligned":
            assert "partials" in gn                       # the two-wave slab kernel writes them (checked against the stored output)
        else:
            assert "partials" not in gn and "nblk" not in gn, "gn_out must be declined where the one-wave slab kernel runs"


def test_layernorm_fold_with_offset_output(monkeypatch):
    """kind 6 (LayerNorm fold, ln_rows) into an 8-byte aligned output with an odd-multiple-of-4 pitch"""
    from theatergen_amd import ops
    from theatergen_amd.weights_pack import pack_ln_linear
    g = torch.Generator().manual_seed(77)
    M, K, N = 1024, 320, 640
    x = (_rows(g, M, K, K, 0).float() + 2.0).to(BF16)
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    wp, u, v = pack_ln_linear(w.to(BF16), torch.randn(N, generator=g), 1 + 0.1 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g))
    rows = ops.layernorm_stats(x, 1e-5)
    for off, ld in ((4, N + 4), (0, N)):
        out = _rows(g, M, N, ld, off)
        _, plan = _launch(monkeypatch, ops.linear, x, wp.to(DEV), ln=(u.to(DEV), v.to(DEV), 1e-5, rows), out=out)
        assert plan[3] == 6


# ---- TG_GEMM_FLAGS is a planner knob: no bit of it reaches a kernel or a launcher ----------------------------------------------------
# what the word once meant besides the planner's five bits: stagger (1), priority hints (2, 32768), the big tile's epilogue (4), the tile-major work
# order (8192), the two-wave slab kernel's timing switches (1 << 16 .. 1 << 18, wrong results by design)
RETIRED_FLAGS = 1 | 2 | 4 | 8192 | 32768 | 1 << 16 | 1 << 17 | 1 << 18
FAMILIES = [
    # id, kind, smallest shape of the family in LINEAR / CONV above and tests/test_round6_gpu.py's PP_SHAPES / P160_SHAPES, force_tile, kernel label
    ("glds_128x128", "linear", (512, 320, 320), 1, "gemm_glds_kernel<plain,128x128>"),
    ("glds_64x64", "linear", (512, 320, 320), 2, "gemm_glds_kernel<plain,64x64>"),
    ("glds_conv", "conv", (2, 32, 32, 320, 320, 2), 0, "gemm_glds_kernel<conv,"),
    ("halo_conv", "conv", (2, 64, 64, 320, 320, 1), 0, "conv_halo_kernel<128x128>"),
    ("t160", "linear", (2048, 640, 640), 21, "gemm_glds_kernel<plain,128x160>"),
    ("ln_fold", "ln", (1024, 640, 320), 0, "gemm_glds_kernel<plain+ln,"),
    ("pingpong_24", "linear", (256, 256, 128), 24, "pp_gemm_kernel<256x256>"),
    ("pingpong_25", "linear", (256, 160, 128), 25, "pp160_gemm_kernel<256x160>"),
    ("big_tile_10", "linear", (512, 320, 320), 10, "bt_gemm_kernel<256x256>"),
    ("big_tile_10_geglu", "geglu", (512, 320, 320), 10, "bt_gemm_kernel<256x256>"),      # the launch bit 2 used to move off the register-only epilogue
    ("slab", "slab1", (2, 64, 64, 320, 320, 1), 11, "conv_slab_kernel<128x320>"),
    ("slab_two_wave", "conv", (2, 64, 64, 320, 320, 1), 11, "conv_slab_pp_kernel<128x320>"),
]


@pytest.mark.parametrize("family", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_retired_flag_bits_reach_no_kernel(monkeypatch, family):
    """one launch per kernel family with TG_GEMM_FLAGS unset and one with every retired bit set: the same kernel, the same bits out"""
    from theatergen_amd import ops
    from theatergen_amd.weights_pack import pack_conv3x3, pack_ln_linear
    name, kind, shape, ft, label = family
    g = torch.Generator().manual_seed(len(name) + ft + sum(shape))
    if kind in ("conv", "slab1"):
        B, H, W, cin, cout, stride = shape
        x = _rows(g, B * H * W, cin, cin, 0)
        wp = pack_conv3x3(torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin)).to(BF16).to(DEV)
        M = B * ((H - 1) // stride + 1) * ((W - 1) // stride + 1)
        bias, res = _rows(g, 1, cout, cout, 0)[0], _rows(g, M, cout, cout, 0)
        run = lambda: ops.conv3x3(x, wp, B, H, W, cin, stride=stride, force_tile=ft, bias=bias, res=res)
        if kind == "slab1":
            monkeypatch.setenv("TG_SLAB_PP", "0")                 # conv_slab_kernel on a layer the two-wave kernel takes
    else:
        M, N, K = shape
        a = _rows(g, M, K, K, 0)
        w = _rows(g, N, K, K, 0, 1 / math.sqrt(K))
        bias = _rows(g, 1, N, N, 0)[0]
        if kind == "ln":
            wl, u, v = pack_ln_linear(w, bias, (1 + 0.1 * torch.randn(K, generator=g)).to(DEV), (0.1 * torch.randn(K, generator=g)).to(DEV))
            run = lambda: ops.linear(a, wl, ln=(u, v, 1e-5))
        elif kind == "geglu":
            run = lambda: ops.gemm(a, w, M, N, K, bias=bias, geglu=True, force_tile=ft)
        else:
            res = _rows(g, M, N, N, 0)
            run = lambda: ops.linear(a, w, bias, res=res, force_tile=ft)

    def launch():
        ops.gemm_profile_start()
        try:
            out = run()
            torch.cuda.synchronize()
        finally:
            recs = ops.gemm_profile_stop()
        assert len(recs) == 1 and recs[0]["kernel"].startswith(label), recs
        return out, recs[0]["kernel"]
    monkeypatch.delenv("TG_GEMM_FLAGS", raising=False)
    want, kernel = launch()
    monkeypatch.setenv("TG_GEMM_FLAGS", str(RETIRED_FLAGS))
    got, kernel_flags = launch()
    assert kernel_flags == kernel
    assert bool(torch.isfinite(want.float()).all())
    same = torch.equal(want, got)
    assert same, f"{name}: TG_GEMM_FLAGS={RETIRED_FLAGS} changed the output of {kernel}"
