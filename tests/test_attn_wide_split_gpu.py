"""GPU: key-split execution of the wide-head flash attention (``tg_attention_wide_split``: a partial launch over S key ranges and a combine launch;
csrc/tg_attention_wide.hip), ``ops.attention_wide(..., key_splits=)`` and the VAE switch ``flash_split`` built on it.

The cases are built as tests/test_attn_wide_gpu.py builds them (restated here): pitched q / k / V^T buffers that hold NaN outside what the contract
says is read, ``out`` filled with a sentinel that must survive outside [n_q, heads * head_dim] of every batch item, the reference in fp64 on the CPU
from the same stored inputs, and the materialised route (scores GEMM -> ``softmax_rows`` -> PV GEMM) on the same inputs.  The bounds are that
test's, unchanged:

  * ``err_split <= err_materialised``;
  * ``err_split <= 2^-8`` (bf16) / ``2^-11`` (fp16) rel-L2: P is rounded where it enters PV and O once at the end, half an ulp each (2^-9 / 2^-12);
    the partials and the combine are fp32 (errors ~1e-6), so the split adds no rounding of the storage dtype's size.

The workspace of the direct calls is allocated at exactly ``tg_attention_wide_workspace_bytes`` plus a sentinel tail and prefilled with NaN: a finite
result proves that every partial the combine reads was written, the intact tail that nothing past the stated size was.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
SENTINEL = 7.0
TAIL = 1024                                    # fp32 sentinels after the workspace
NQS = (8, 40, 136)                             # a partial wave, a partial block, two query blocks
LEN_SPLITS = ((40, 2), (72, 2), (72, 3), (200, 2), (200, 3), (200, 7))
LN2 = 0.6931471805599453


def fmt_bound(dtype):
    return 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11


def rel_l2(got, ref):
    got, ref = got.double().cpu(), ref.double()
    return float((got - ref).norm() / ref.norm())


class Case:
    """pitched q / k / V^T buffers (NaN outside what is read), the dense per-(batch, head) operands and the fp64 result"""

    def __init__(self, dtype, B, H, D, n_q, len0, seed, fill=None):
        g = torch.Generator().manual_seed(seed)
        inner = H * D
        self.dtype, self.B, self.H, self.D, self.n_q, self.len0, self.scale = dtype, B, H, D, n_q, len0, D ** -0.5
        self.q_ld, self.k_ld, self.vt_ld, self.out_ld = inner + 8, inner + 16, len0 + 8, inner + 4
        self.q_bs, self.k_bs, self.vt_bs = n_q * self.q_ld + 24, len0 * self.k_ld + 8, inner * self.vt_ld + 16
        self.out_rows = n_q + 2
        self.out_bs = self.out_rows * self.out_ld + 4
        q = torch.randn(B, n_q, inner, generator=g)
        k = torch.randn(B, len0, inner, generator=g)
        v = torch.randn(B, len0, inner, generator=g)
        if fill is not None:
            q, k = fill(q, k, g)
        self.q, self.k, self.v = q.to(dtype), k.to(dtype), v.to(dtype)            # the stored inputs
        qb = torch.full((B * self.q_bs,), float("nan"), dtype=dtype)
        kb = torch.full((B * self.k_bs,), float("nan"), dtype=dtype)
        vb = torch.full((B * self.vt_bs,), float("nan"), dtype=dtype)
        for b in range(B):
            qb[b * self.q_bs:b * self.q_bs + n_q * self.q_ld].view(n_q, self.q_ld)[:, :inner] = self.q[b]
            kb[b * self.k_bs:b * self.k_bs + len0 * self.k_ld].view(len0, self.k_ld)[:, :inner] = self.k[b]
            vb[b * self.vt_bs:b * self.vt_bs + inner * self.vt_ld].view(inner, self.vt_ld)[:, :len0] = self.v[b].t()
        self.qb, self.kb, self.vb = qb.to(DEV), kb.to(DEV), vb.to(DEV)
        q4 = self.q.double().view(B, n_q, H, D).transpose(1, 2)
        k4 = self.k.double().view(B, len0, H, D).transpose(1, 2)
        v4 = self.v.double().view(B, len0, H, D).transpose(1, 2)
        p = torch.softmax(q4 @ k4.transpose(-1, -2) * self.scale, dim=-1)
        self.ref = (p @ v4).transpose(1, 2).reshape(B, n_q, inner)                   # fp64
        self._mat = None

    def desc(self, out):
        from theatergen_amd import _lib
        d = _lib.AttnDesc()
        d.dtype = 0 if self.dtype == torch.bfloat16 else 1
        d.batch, d.heads, d.head_dim, d.n_q, d.len0 = self.B, self.H, self.D, self.n_q, self.len0
        d.q, d.q_ld, d.q_bs = self.qb.data_ptr(), self.q_ld, self.q_bs
        d.k0, d.k0_ld, d.k0_bs = self.kb.data_ptr(), self.k_ld, self.k_bs
        d.vt0, d.vt0_ld, d.vt0_bs = self.vb.data_ptr(), self.vt_ld, self.vt_bs
        d.scale = self.scale
        d.out, d.out_ld, d.out_bs = out.data_ptr(), self.out_ld, self.out_bs
        return d

    def _unpack(self, out):
        out = out.cpu()
        inner = self.H * self.D
        got = torch.stack([out[b * self.out_bs:b * self.out_bs + self.out_rows * self.out_ld].view(self.out_rows, self.out_ld)[:self.n_q, :inner]
                           for b in range(self.B)])
        guard = out.clone()
        for b in range(self.B):
            guard[b * self.out_bs:b * self.out_bs + self.out_rows * self.out_ld].view(self.out_rows, self.out_ld)[:self.n_q, :inner] = SENTINEL
        return got, bool((guard == SENTINEL).all())

    def run_ops(self, key_splits=None):
        """through ``ops.attention_wide`` (the persistent workspace of the package)"""
        from theatergen_amd import ops
        out = torch.full((self.B * self.out_bs,), SENTINEL, dtype=self.dtype, device=DEV)
        ops.attention_wide(self.qb, self.q_ld, self.q_bs, self.kb, self.k_ld, self.k_bs, self.vb, self.vt_ld, self.vt_bs, self.len0,
                           self.B, self.H, self.D, self.n_q, self.scale, out, self.out_ld, self.out_bs, key_splits=key_splits)
        torch.cuda.synchronize()
        return self._unpack(out)

    def run_split_abi(self, S):
        """``tg_attention_wide_split`` itself on a NaN workspace of exactly the stated size + a sentinel tail -> (got, out guard ok, tail ok)"""
        from theatergen_amd import _lib
        h = _lib.lib()
        out = torch.full((self.B * self.out_bs,), SENTINEL, dtype=self.dtype, device=DEV)
        d = self.desc(out)
        assert h.tg_attention_wide_splits(C.byref(d), S) == S, "the case asks for more splits than it has key tiles"
        nbytes = h.tg_attention_wide_workspace_bytes(C.byref(d), S)
        rows = ((self.n_q + 127) // 128) * 128
        assert nbytes == S * self.B * self.H * rows * (self.D + 2) * 4 and nbytes % 4 == 0
        ws = torch.full((nbytes // 4 + TAIL,), float("nan"), dtype=torch.float32, device=DEV)
        ws[nbytes // 4:] = SENTINEL
        assert ws.data_ptr() % 16 == 0
        _lib.check(h.tg_attention_wide_split(C.byref(d), S, ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        got, guard_ok = self._unpack(out)
        return got, guard_ok, bool((ws[nbytes // 4:] == SENTINEL).all())

    def err_materialised(self):
        """today's materialised route of ``VAEAttention.run``, per batch item and head, on dense copies of the same stored values (once per case)"""
        if self._mat is None:
            from theatergen_amd import ops
            B, H, D, n_q, len0 = self.B, self.H, self.D, self.n_q, self.len0
            got = torch.empty(B, n_q, H * D, dtype=self.dtype)
            for b in range(B):
                for h in range(H):
                    q = self.q[b, :, h * D:(h + 1) * D].contiguous().to(DEV)
                    k = self.k[b, :, h * D:(h + 1) * D].contiguous().to(DEV)
                    vt = self.v[b, :, h * D:(h + 1) * D].t().contiguous().to(DEV)
                    scores = torch.empty((n_q, len0), dtype=self.dtype, device=DEV)
                    o = torch.empty((n_q, D), dtype=self.dtype, device=DEV)
                    ops.gemm(q, k, n_q, len0, D, out=scores)
                    ops.softmax_rows(scores, scale=self.scale, out=scores)
                    ops.gemm(scores, vt, n_q, D, len0, out=o)
                    got[b, :, h * D:(h + 1) * D] = o.cpu()
            self._mat = rel_l2(got, self.ref)
        return self._mat


def _check(c, S, what, fails):
    got, guard_ok, tail_ok = c.run_split_abi(S)
    err, err_mat = rel_l2(got, c.ref), c.err_materialised()
    print(f"{what} S{S}: err_split={err:.3e} err_materialised={err_mat:.3e} bound={fmt_bound(c.dtype):.3e} guard_ok={guard_ok} tail_ok={tail_ok}")
    if not bool(torch.isfinite(got.float()).all()):
        fails.append(f"{what} S{S}: non-finite output (a partial the combine reads was not written, or a masked key was read)")
    if not guard_ok:
        fails.append(f"{what} S{S}: wrote outside [n_q, heads * head_dim]")
    if not tail_ok:
        fails.append(f"{what} S{S}: wrote past workspace_bytes")
    if not err <= err_mat:
        fails.append(f"{what} S{S}: err_split {err:.3e} > err_materialised {err_mat:.3e}")
    if not err <= fmt_bound(c.dtype):
        fails.append(f"{what} S{S}: err_split {err:.3e} > {fmt_bound(c.dtype):.3e}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("D,H", [(256, 1), (256, 2), (512, 1)])
def test_contract_cases_vs_fp64(D, H, dtype):
    fails = []
    for i, n_q in enumerate(NQS):
        cases = {}
        for len0, S in LEN_SPLITS:
            if len0 not in cases:
                cases[len0] = Case(dtype, 2, H, D, n_q, len0, seed=2000 + 100 * i + len0 + H)
            _check(cases[len0], S, f"d{D} h{H} {str(dtype)[6:]} n_q{n_q} len{len0}", fails)
    assert not fails, "\n".join(fails)


def _rising(step):
    """keys ordered so that the row max rises by ``step`` nats at every 32-key tile: large negative scores early, large positive late"""
    def fill(q, k, g):
        B, n_q, D = q.shape
        L = k.shape[1]
        u = torch.randn(D, generator=g)
        u = u / u.norm()
        q = u[None, None, :] * (D ** 0.25) * 4.0 + 0.25 * q                          # q . u ~ 4 d^(1/4)
        nt = (L + 31) // 32
        level = torch.tensor([(j // 32 - (nt - 2)) * step for j in range(L)])          # scores: ..., -step, 0, +step at the last tile
        k = u[None, None, :] * (level[None, :, None] * (D ** 0.25) / 4.0) + 0.25 * k    # scale * (q . u)(k . u) = level
        return q, k
    return fill


def _dominant(D):
    def fill(q, k, g):
        qm = q.mean(1)                                                               # [B, D]: every query gets the shared component below
        qdir = qm / qm.norm(dim=-1, keepdim=True)
        q = 0.5 * q + qdir[:, None, :] * (D ** 0.25) * 4.0
        k = 0.5 * k
        k[:, 70] = qdir * (15.0 * (D ** 0.25) / 4.0)                                  # scale * (q . k_70) ~ 15 nats; the others ~ N(0, 1/16)
        return q, k
    return fill


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [256, 512])
def test_rescale_cases_vs_fp64(D, dtype):
    """the row max rises by 12 nats at every tile, so every later split's reference is far above the earlier ones' (weights ~ e^-12 per tile in the
    combine); by 60 nats, where the early splits' weights underflow to exactly 0; and one dominant key in the last split's partial tile"""
    fails = []
    for step in (12.0, 60.0):
        c = Case(dtype, 2, 1, D, 40, 104, seed=7, fill=_rising(step))                   # 3 full tiles + a partial one
        s = (c.q.double() @ c.k.double().transpose(1, 2) * c.scale)
        tile_max = torch.stack([s[..., t * 32:(t + 1) * 32].max(-1).values for t in range(4)], -1)
        assert bool((tile_max[..., 1:] - tile_max[..., :-1] > 8.0 * LN2).all()), "the case does not force a rescale at every tile"
        if step == 60.0:
            # the weight of split 0 against the last one, exp(m_0 - M): below the smallest fp32 subnormal (2^-149), so exactly 0 in the combine
            assert bool((tile_max[..., 0] - tile_max[..., 3] < -150.0 * LN2).all()), "the early weights do not underflow"
        for S in (2, 4):
            _check(c, S, f"rising {step:g} d{D} {str(dtype)[6:]}", fails)
    c = Case(dtype, 2, 1, D, 40, 72, seed=8, fill=_dominant(D))                       # key 70 lives in the partial tile [64, 72) = split 2 of 3
    s = (c.q.double() @ c.k.double().transpose(1, 2) * c.scale)
    assert bool((s.argmax(-1) == 70).all()) and bool((s[..., 70] - s[..., :64].max(-1).values > 8.0 * LN2).all())
    _check(c, 3, f"dominant-last d{D} {str(dtype)[6:]}", fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [256, 512])
def test_clamp_and_one_split_equal_the_unsplit_call_bit_for_bit(D, dtype):
    c = Case(dtype, 2, 1, D, 40, 8, seed=31)                                          # one key tile: 4 requested splits are 1
    base, ok = c.run_ops(None)
    got, ok4 = c.run_ops(4)
    assert ok and ok4 and torch.equal(got, base)
    c = Case(dtype, 2, 1, D, 136, 200, seed=32)
    base, _ = c.run_ops(None)
    assert torch.equal(c.run_ops(1)[0], base)
    # the C entry with one effective split: the unsplit kernel, and the workspace (here: none at all) is not touched
    from theatergen_amd import _lib
    out = torch.full((c.B * c.out_bs,), SENTINEL, dtype=dtype, device=DEV)
    _lib.check(_lib.lib().tg_attention_wide_split(C.byref(c.desc(out)), 1, None, 0, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(c._unpack(out)[0], base)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [256, 512])
def test_forced_split_is_deterministic_and_batch_items_are_independent(D, dtype):
    from theatergen_amd import ops
    c = Case(dtype, 2, 1, D, 136, 200, seed=21)
    for S in (2, 3):
        a, _ = c.run_ops(S)
        b, _ = c.run_ops(S)
        assert torch.equal(a, b), f"S = {S}: two calls differ"
        assert bool(torch.isfinite(a.float()).all())
        out1 = torch.empty((c.n_q, D), dtype=dtype, device=DEV)
        ops.attention_wide(c.qb[c.q_bs:], c.q_ld, c.q_bs, c.kb[c.k_bs:], c.k_ld, c.k_bs, c.vb[c.vt_bs:], c.vt_ld, c.vt_bs, c.len0,
                           1, 1, D, c.n_q, c.scale, out1, D, c.n_q * D, key_splits=S)
        torch.cuda.synchronize()
        assert torch.equal(out1.cpu(), a[1]), f"S = {S}: row 1 of the B = 2 call differs from the B = 1 call"


# ---- the VAE route -------------------------------------------------------------------------------------------------------------------
def _set(vae, flash, flash_split):
    for m in (vae.encoder, vae.decoder):
        if m is not None:
            m.mid_block.attentions[0].flash = flash
            m.mid_block.attentions[0].flash_split = flash_split


def _planner_says(C_, dtype, B, N):
    from theatergen_amd import _lib
    d = _lib.AttnDesc()
    d.dtype = 0 if dtype == torch.bfloat16 else 1
    d.batch, d.heads, d.head_dim, d.n_q, d.len0 = B, 1, C_, N, N
    d.q = d.k0 = d.vt0 = d.out = 16                                                   # the planner reads sizes only
    d.q_ld, d.q_bs, d.k0_ld, d.k0_bs, d.vt0_ld, d.vt0_bs = 2 * C_, N * 2 * C_, 2 * C_, N * 2 * C_, N, C_ * N
    d.out_ld, d.out_bs, d.scale = C_, N * C_, C_ ** -0.5
    S = _lib.lib().tg_attention_wide_splits(C.byref(d), 0)
    assert S >= 1
    return S


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("C_", [256, 512])
def test_vae_reduced_plan_flash_split_vs_off_vs_oracle(C_, dtype):
    """block_out_channels (128, C): mid block at the 16 x 16 latent (N = 256, 8 key tiles), B = 2"""
    from oracle import vae as ov
    from tests.test_hotpath_gpu import _build_vae_full, close, net_tol
    from theatergen_amd import ops
    from theatergen_amd.vae import sd_vae_config
    cfg = sd_vae_config(block_out_channels=(128, C_), sample_size=32)
    vae, sd_r = _build_vae_full(cfg, dtype)
    g = torch.Generator().manual_seed(60 + C_)
    lat = torch.randn(2, 4, 16, 16, generator=g) * cfg.scaling_factor
    img = torch.rand(2, 3, 32, 32, generator=g) * 2 - 1
    ref_d, ref_e = ov.decode(cfg, sd_r, lat), ov.encode_moments(cfg, sd_r, img.to(dtype).float())
    auto = _planner_says(C_, dtype, 2, 256)
    plain, split2, comb = f"attention_wide_kernel<d{C_}>", f"attention_wide_kernel<d{C_},split2>", f"attention_wide_combine_kernel<d{C_}>"
    want = {None: {plain: 2}, 2: {split2: 2, comb: 2},
            True: {plain: 2} if auto == 1 else {f"attention_wide_kernel<d{C_},split{auto}>": 2, comb: 2}}
    got = {}
    for fs in (None, 2, True):
        _set(vae, True, fs)
        ops.gemm_profile_start()
        got[fs] = (vae.decode_latents(lat.to(DEV))[0], vae.encode(img.to(DEV, dtype)).latent_dist.parameters)
        torch.cuda.synchronize()
        names = [r["kernel"] for r in ops.gemm_profile_stop()]
        wide = {n: names.count(n) for n in set(names) if "attention_wide" in n}
        assert wide == want[fs], f"flash_split={fs} (planner: {auto}): {wide}"                    # one (pair of) launch(es) per call: decode + encode
        close(got[fs][0], ref_d, net_tol(dtype), f"reduced vae decode C={C_}, flash_split {fs}")
        close(got[fs][1], ref_e, net_tol(dtype), f"reduced vae encode C={C_}, flash_split {fs}")
    close(got[2][0], got[None][0].cpu(), net_tol(dtype), f"reduced vae decode C={C_}: flash_split 2 vs off")
    close(got[2][1], got[None][1].cpu(), net_tol(dtype), f"reduced vae encode C={C_}: flash_split 2 vs off")
    _set(vae, False, 2)                                                                # the materialised route ignores the switch
    ops.gemm_profile_start()
    vae.decode_latents(lat.to(DEV))
    torch.cuda.synchronize()
    assert not [r["kernel"] for r in ops.gemm_profile_stop() if "attention_wide" in r["kernel"]]


def test_narrow_flash_route_ignores_the_switch():
    """C = 128 runs on ``tg_attention``: ``flash_split`` changes nothing, bit for bit"""
    from theatergen_amd.unet import _Act
    from theatergen_amd.vae import VAEAttention
    torch.manual_seed(3)
    m = VAEAttention(128, flash=True).requires_grad_(False).to(DEV, torch.bfloat16)
    x = torch.randn(2 * 64, 128, generator=torch.Generator().manual_seed(4)).to(torch.bfloat16).to(DEV)
    a = m.run(_Act(x, 2, 8, 8, 128)).t.clone()
    m.flash_split = 2
    assert torch.equal(m.run(_Act(x, 2, 8, 8, 128)).t, a)


def test_graph_capture_replays_bit_equal_to_eager():
    """flash on, flash_split 2, B = 2, C = 256, N = 64 (two key tiles: one per split): captured once, replayed twice with new input contents"""
    from theatergen_amd import ops
    from theatergen_amd.unet import _Act
    from theatergen_amd.vae import VAEAttention
    dtype, C_, B = torch.bfloat16, 256, 2
    torch.manual_seed(3)
    m = VAEAttention(C_, flash=True, flash_split=2).requires_grad_(False).to(DEV, dtype)
    g = torch.Generator().manual_seed(25)
    xs = [torch.randn(B * 64, C_, generator=g).to(dtype).to(DEV) for _ in range(3)]
    ops.gemm_profile_start()
    first = m.run(_Act(xs[0], B, 8, 8, C_)).t.clone()
    torch.cuda.synchronize()
    names = [r["kernel"] for r in ops.gemm_profile_stop()]
    assert names.count("attention_wide_kernel<d256,split2>") == 1 and names.count("attention_wide_combine_kernel<d256>") == 1, names
    eager = [first] + [m.run(_Act(x, B, 8, 8, C_)).t.clone() for x in xs[1:]]
    static_in = xs[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.run(_Act(static_in, B, 8, 8, C_))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = m.run(_Act(static_in, B, 8, 8, C_)).t
    for x, want in zip(xs[1:], eager[1:]):
        static_in.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_out, want)
