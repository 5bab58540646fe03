"""GPU: the wide-head flash attention (``tg_attention_wide``, head_dim 256 / 512; csrc/tg_attention_wide.hip) and the VAE route built on it
(``VAEAttention.flash`` / ``TG_VAE_FLASH=1``).

The reference of every kernel case is computed here, in fp64 on the CPU, from the same stored inputs.  Two bounds per case:

  * ``err_new <= err_materialised``: the rel-L2 error of today's route on the same inputs (scores GEMM -> ``softmax_rows`` -> PV GEMM, as
    ``VAEAttention.run`` does with the switch off), which rounds the scores to the storage dtype before the softmax;
  * ``err_new <= 2 ulp-halves``: rel-L2 <= 2^-8 (bf16) / 2^-11 (fp16).  The kernel rounds twice, P where it enters the PV product and O once at the
    end, each by at most half an ulp = 2^-9 / 2^-12 relative; everything between is fp32 (errors ~1e-6).  Two independent roundings of that size
    add up to at most sqrt(2) of it, below the bound.

Buffers are filled with NaN outside the elements the contract says are read (pitch padding, gaps between batch items, V^T columns past len0), so
a masked key that is multiplied by zero instead of never being read shows up as NaN in the result; ``out`` is filled with a sentinel that must
survive outside [n_q, heads * head_dim] of every batch item.

The VAE cases use the bound the existing VAE tests state for that plan and dtype (tests/test_hotpath_gpu.py: ``net_tol``, max 6e-2 / 1.5e-2 and
rel-L2 half of it).  With ``TG_ATTN_WIDE_ERR_JSON`` set, the per-case error pairs are also written to that file (the table of
profiles/attn_wide_findings.md).
"""
import ctypes as C
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
SENTINEL = 7.0
NQS, LENS = (8, 40, 136), (8, 72, 200)
_ROWS = []


def fmt_bound(dtype):
    return 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11


def _record(row):
    _ROWS.append(row)
    path = os.environ.get("TG_ATTN_WIDE_ERR_JSON")
    if path:
        old = json.load(open(path)) if os.path.exists(path) else []
        with open(path, "w") as f:
            json.dump([r for r in old if r["case"] != row["case"]] + [row], f, indent=1)


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

    def run_wide(self):
        from theatergen_amd import ops
        out = torch.full((self.B * self.out_bs,), SENTINEL, dtype=self.dtype, device=DEV)
        ops.attention_wide(self.qb, self.q_ld, self.q_bs, self.kb, self.k_ld, self.k_bs, self.vb, self.vt_ld, self.vt_bs, self.len0,
                           self.B, self.H, self.D, self.n_q, self.scale, out, self.out_ld, self.out_bs)
        torch.cuda.synchronize()
        out = out.cpu()
        inner = self.H * self.D
        got = torch.stack([out[b * self.out_bs:b * self.out_bs + self.out_rows * self.out_ld].view(self.out_rows, self.out_ld)[:self.n_q, :inner]
                           for b in range(self.B)])
        guard = out.clone()
        for b in range(self.B):
            guard[b * self.out_bs:b * self.out_bs + self.out_rows * self.out_ld].view(self.out_rows, self.out_ld)[:self.n_q, :inner] = SENTINEL
        return got, bool((guard == SENTINEL).all())

    def run_materialised(self):
        """today's route of ``VAEAttention.run``, per batch item and head, on dense copies of the same stored values"""
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
        return got


def _check(c, what, fails):
    got, guard_ok = c.run_wide()
    err_new = rel_l2(got, c.ref)
    err_mat = rel_l2(c.run_materialised(), c.ref)
    print(f"{what}: err_new={err_new:.3e} err_materialised={err_mat:.3e} bound={fmt_bound(c.dtype):.3e} guard_ok={guard_ok}")
    _record(dict(case=what, err_new=err_new, err_materialised=err_mat))
    if not bool(torch.isfinite(got.float()).all()):
        fails.append(f"{what}: non-finite output")
    if not guard_ok:
        fails.append(f"{what}: wrote outside [n_q, heads * head_dim]")
    if not err_new <= err_mat:
        fails.append(f"{what}: err_new {err_new:.3e} > err_materialised {err_mat:.3e}")
    if not err_new <= fmt_bound(c.dtype):
        fails.append(f"{what}: err_new {err_new:.3e} > {fmt_bound(c.dtype):.3e}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("D,H", [(256, 1), (256, 2), (512, 1)])
def test_contract_cases_vs_fp64(D, H, dtype):
    fails = []
    for i, n_q in enumerate(NQS):
        for j, len0 in enumerate(LENS):
            c = Case(dtype, 2, H, D, n_q, len0, seed=1000 + 100 * i + 10 * j + H)
            _check(c, f"d{D} h{H} {str(dtype)[6:]} n_q{n_q} len{len0}", fails)
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


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [256, 512])
def test_forced_rescale_vs_fp64(D, dtype):
    """the running max moves at EVERY key tile (by 12 nats = 17 in exp2 units, above the kernel's lazy-rescale threshold of 8), and a layout whose
    one dominant key sits in the last, partial tile"""
    fails = []
    c = Case(dtype, 2, 1, D, 40, 104, seed=7, fill=_rising(12.0))                     # 3 full tiles + a partial one
    s = (c.q.double() @ c.k.double().transpose(1, 2) * c.scale)
    tile_max = torch.stack([s[..., t * 32:(t + 1) * 32].max(-1).values for t in range(4)], -1)
    assert bool((tile_max[..., 1:] - tile_max[..., :-1] > 8.0 * 0.6931471805599453).all()), "the case does not force a rescale at every tile"
    _check(c, f"rising d{D} {str(dtype)[6:]}", fails)

    def dominant(q, k, g):
        qm = q.mean(1)                                                               # [B, D]: every query gets the shared component below
        qdir = qm / qm.norm(dim=-1, keepdim=True)
        q = 0.5 * q + qdir[:, None, :] * (D ** 0.25) * 4.0
        k = 0.5 * k
        k[:, 70] = qdir * (15.0 * (D ** 0.25) / 4.0)                                  # scale * (q . k_70) ~ 15 nats; the others ~ N(0, 1/16)
        return q, k
    c = Case(dtype, 2, 1, D, 40, 72, seed=8, fill=dominant)                           # key 70 lives in the partial tile [64, 72)
    s = (c.q.double() @ c.k.double().transpose(1, 2) * c.scale)
    assert bool((s.argmax(-1) == 70).all()) and bool((s[..., 70] - s[..., :64].max(-1).values > 8.0 * 0.6931471805599453).all())
    _check(c, f"dominant-last d{D} {str(dtype)[6:]}", fails)
    assert not fails, "\n".join(fails)


def test_refusals_leave_out_untouched():
    from theatergen_amd import _lib
    h = _lib.lib()
    B, D, n_q, len0 = 1, 256, 40, 72
    q = torch.randn(B * n_q, D).to(torch.bfloat16).to(DEV)
    k = torch.randn(B * len0, D).to(torch.bfloat16).to(DEV)
    vt = torch.randn(B * D, len0).to(torch.bfloat16).to(DEV)
    extra = torch.zeros(n_q * len0, dtype=torch.float32, device=DEV)
    out = torch.full((B * n_q, D), SENTINEL, dtype=torch.bfloat16, device=DEV)

    def desc(hd=D, **over):
        d = _lib.AttnDesc()
        d.dtype, d.batch, d.heads, d.head_dim, d.n_q, d.len0 = 0, B, 1, hd, n_q, len0
        d.q, d.k0, d.vt0, d.out = q.data_ptr(), k.data_ptr(), vt.data_ptr(), out.data_ptr()
        d.q_ld, d.q_bs, d.k0_ld, d.k0_bs, d.vt0_ld, d.vt0_bs = D, n_q * D, D, len0 * D, len0, D * len0
        d.out_ld, d.out_bs, d.scale = D, n_q * D, D ** -0.5
        for f, v in over.items():
            setattr(d, f, v)
        return d
    st = torch.cuda.current_stream().cuda_stream
    cases = {"head_dim 192": desc(hd=192), "len1 > 0": desc(len1=8, k1=k.data_ptr(), vt1=vt.data_ptr(), k1_ld=D, vt1_ld=len0),
             "causal": desc(causal=1), "mask": desc(mask=extra.data_ptr()), "w1_dev": desc(w1_dev=extra.data_ptr())}
    for what, d in cases.items():
        rc = h.tg_attention_wide(C.byref(d), st)
        assert rc == -3, f"{what}: returned {rc}, TG_ERR_UNSUPPORTED is -3"
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert h.tg_attention_wide(C.byref(desc()), st) == 0                               # the same descriptor without the refused field runs
    torch.cuda.synchronize()
    assert not bool((out == SENTINEL).any())


# ---- the VAE route -------------------------------------------------------------------------------------------------------------------
def _set_flash(vae, on):
    for m in (vae.encoder, vae.decoder):
        if m is not None:
            m.mid_block.attentions[0].flash = on


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_vae_tiny_plan_flash_vs_oracle(dtype):
    """C = 128: the flash route runs on ``tg_attention`` (one launch for the batch); decode and encode against the in-repo oracle"""
    from oracle import vae as ov
    from tests.test_hotpath_gpu import _build_vae_full, close, net_tol
    from theatergen_amd.vae import tiny_vae_config
    cfg = tiny_vae_config()
    vae, sd_r = _build_vae_full(cfg, dtype)
    _set_flash(vae, True)
    assert vae.decoder.mid_block.attentions[0].flash_route() and vae.encoder.mid_block.attentions[0].flash_route()
    g = torch.Generator().manual_seed(6)
    lat = torch.randn(2, 4, 8, 8, generator=g) * cfg.scaling_factor
    close(vae.decode_latents(lat.to(DEV))[0], ov.decode(cfg, sd_r, lat), net_tol(dtype), "vae decode tiny, flash")
    img = torch.rand(2, 3, 64, 64, generator=g) * 2 - 1
    close(vae.encode(img.to(DEV, dtype)).latent_dist.parameters, ov.encode_moments(cfg, sd_r, img.to(dtype).float()), net_tol(dtype),
          "vae encode tiny, flash")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("C_", [256, 512])
def test_vae_reduced_plan_flash_on_vs_off_vs_oracle(C_, dtype):
    """block_out_channels (128, C): mid block at the 16 x 16 latent (N = 256), B = 2; the flash route runs on ``tg_attention_wide``"""
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
    got = {}
    for on in (False, True):
        _set_flash(vae, on)
        ops.gemm_profile_start()
        got[on] = (vae.decode_latents(lat.to(DEV))[0], vae.encode(img.to(DEV, dtype)).latent_dist.parameters)
        torch.cuda.synchronize()
        names = [r["kernel"] for r in ops.gemm_profile_stop()]
        assert names.count(f"attention_wide_kernel<d{C_}>") == (2 if on else 0), names        # one launch per call: decode + encode
        close(got[on][0], ref_d, net_tol(dtype), f"reduced vae decode C={C_}, flash {on}")
        close(got[on][1], ref_e, net_tol(dtype), f"reduced vae encode C={C_}, flash {on}")
    close(got[True][0], got[False][0].cpu(), net_tol(dtype), f"reduced vae decode C={C_}: flash on vs off")
    close(got[True][1], got[False][1].cpu(), net_tol(dtype), f"reduced vae encode C={C_}: flash on vs off")


def _attn_module(C_, dtype, seed=3):
    from theatergen_amd.vae import VAEAttention
    torch.manual_seed(seed)
    m = VAEAttention(C_, flash=True)
    for p in m.parameters():
        p.requires_grad_(False)
    return m.to(DEV, dtype)


def _act(x, B, h, w, C_):
    from theatergen_amd.unet import _Act
    return _Act(x, B, h, w, C_)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("C_", [256, 512])
def test_batch_items_are_independent(C_, dtype):
    """row 1 of a B = 2 call equals a B = 1 call bit for bit (the attention launch itself, and the whole block)"""
    from theatergen_amd import ops
    c = Case(dtype, 2, 1, C_, 136, 200, seed=21)
    got2, _ = c.run_wide()
    out1 = torch.empty((c.n_q, C_), dtype=dtype, device=DEV)
    ops.attention_wide(c.qb[c.q_bs:], c.q_ld, c.q_bs, c.kb[c.k_bs:], c.k_ld, c.k_bs, c.vb[c.vt_bs:], c.vt_ld, c.vt_bs, c.len0,
                       1, 1, C_, c.n_q, c.scale, out1, C_, c.n_q * C_)
    assert torch.equal(out1.cpu(), got2[1])
    m = _attn_module(C_, dtype)
    x = torch.randn(2 * 256, C_, generator=torch.Generator().manual_seed(22)).to(dtype).to(DEV)
    y2 = m.run(_act(x, 2, 16, 16, C_)).t
    y1 = m.run(_act(x[256:].contiguous(), 1, 16, 16, C_)).t
    assert torch.equal(y2[256:], y1)


def test_no_n_by_n_buffer_and_launches_do_not_grow_with_batch():
    """C = 512, N = 4096, B = 1: the call's peak allocation stays below the N x N scores tensor today's route allocates (32 MiB in bf16);
    the number of recorded launches is the same for B = 1 and B = 4"""
    from theatergen_amd import ops
    dtype, C_, N = torch.bfloat16, 512, 4096
    m = _attn_module(C_, dtype)
    x = torch.randn(N, C_, generator=torch.Generator().manual_seed(23)).to(dtype).to(DEV)
    m.run(_act(x, 1, 64, 64, C_))                                                  # warm-up: packed weights, persistent workspaces
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y = m.run(_act(x, 1, 64, 64, C_)).t
    torch.cuda.synchronize()
    delta = torch.cuda.max_memory_allocated() - base
    print(f"peak allocation of one flash call at N = {N}: {delta / 2**20:.1f} MiB (N x N scores: {N * N * 2 / 2**20:.0f} MiB)")
    assert delta < N * N * x.element_size(), delta
    assert bool(torch.isfinite(y.float()).all())
    counts = {}
    for B in (1, 4):
        xb = torch.randn(B * 256, C_, generator=torch.Generator().manual_seed(24)).to(dtype).to(DEV)
        ops.gemm_profile_start()
        m.run(_act(xb, B, 16, 16, C_))
        torch.cuda.synchronize()
        names = [r["kernel"] for r in ops.gemm_profile_stop()]
        counts[B] = len(names)
        assert names.count("attention_wide_kernel<d512>") == 1, names
    assert counts[1] == counts[4] == 3, counts                                      # projection GEMM, attention, to_out


def test_graph_capture_replays_bit_equal_to_eager():
    """flash on, B = 2, C = 256, N = 64: captured once, replayed twice with new input contents"""
    dtype, C_, B = torch.bfloat16, 256, 2
    m = _attn_module(C_, dtype)
    g = torch.Generator().manual_seed(25)
    xs = [torch.randn(B * 64, C_, generator=g).to(dtype).to(DEV) for _ in range(3)]
    eager = [m.run(_act(x, B, 8, 8, C_)).t.clone() for x in xs]
    static_in = xs[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.run(_act(static_in, B, 8, 8, C_))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = m.run(_act(static_in, B, 8, 8, C_)).t
    for x, want in zip(xs[1:], eager[1:]):
        static_in.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_out, want)
