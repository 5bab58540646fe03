"""GPU: the DPM-Solver++ multistep step on the device — ``tg_step_epilogue_dpm`` per step against the direct-form fp64 restatement
(tests/dpm_solver_reference.py), order 1 against the DDIM epilogue, ``scheduler.step`` as a drop-in, the graph-replayed engine (eager parity, the
oracle loop), the two stage functions and ``generate`` / ``decode`` with the scheduler handed in.

Per-step tolerance (derived, not tuned): |got - ref64| <= 2^-20 (|A x| + |B| (|cx x| + |ce m|) + |C p|) elementwise — 16 fp32 rounding units of the
terms' magnitudes for at most 11 roundings (5 coefficients rounded to fp32 once, 6 operations).  The model outputs of the kernel tests are multiples of
2^-6 below 4 in magnitude and the guidance scale is 7.5, so the CFG combine u + g (c - u) is exact in fp32 (with or without a fused multiply-add) and m
is the same number on both sides."""
import numpy as np
import pytest
import torch

from tests import dpm_solver_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -20
G = 7.5
SHAPES = [(2, 4, 8, 12), (1, 4, 5, 3)]          # 768 elements: three blocks of 256; 60: less than one block
_MI = [torch.bfloat16, torch.float16, torch.float32]


def _sched(**kw):
    from theatergen_amd.scheduler import DPMSolverMultistepScheduler
    return DPMSolverMultistepScheduler(**kw)


def _quantised(shape, g):
    return (torch.randn(shape, generator=g).clamp(-3.9, 3.9) * 64).round() / 64


def _bound(row, x, m, p):
    cx, ce, A, B, C = [float(v) for v in row[:5]]
    b = np.abs(A * x) + abs(B) * (np.abs(cx * x) + np.abs(ce * m))
    return U * (b + (np.abs(C * p) if C != 0.0 else 0.0))


def _walk(shape, cfg, pred, frozen_mode, mi_dtype, nan_state=False, steps=4, frozen_steps=2):
    """all rows of a ``steps``-step table on the device; every step is compared on its own, starting from the device's fp32 state"""
    from theatergen_amd import ops
    n, C, h, w = shape
    s = _sched(prediction_type=pred)
    ts = [int(t) for t in s.set_timesteps(steps).tolist()]
    tab64 = s.coef_table(dtype=torch.float64).numpy()
    coef = s.coef_table().to(DEV)
    a = R.alphas_cumprod()
    g = torch.Generator().manual_seed(1000 * n + h)
    lat = torch.randn(shape, generator=g).to(DEV)
    x0p = torch.full(shape, float("nan"), device=DEV) if nan_state else torch.zeros(shape, device=DEV)
    idx = torch.zeros(1, dtype=torch.int32, device=DEV)
    hist = torch.zeros((steps + 1,) + shape, device=DEV)
    model_in = torch.zeros((2 * n, C, h, w), dtype=mi_dtype, device=DEV)
    frozen = mask = None
    if frozen_mode != "off":
        frozen = torch.randn((steps + 1,) + shape, generator=g).to(DEV)
        mask = (torch.rand((n, h, w) if frozen_mode == "per_image" else (h, w), generator=g) > 0.5).float().to(DEV)
    worst = 0.0
    for i in range(steps):
        out = _quantised((2 * n if cfg else n, C, h, w), g)
        m = (out[:n] + G * (out[n:] - out[:n])) if cfg else out
        assert torch.equal(m.double(), (out[:n].double() + G * (out[n:].double() - out[:n].double())) if cfg else out.double()), "CFG inputs are exact in fp32"
        x_b, p_b = lat.cpu().double().numpy(), x0p.cpu().double().numpy()
        ops.step_epilogue_dpm(out.to(DEV), lat, x0p, G if cfg else 0.0, coef, idx, has_cfg=cfg, advance=True, frozen=frozen, frozen_mask=mask,
                              frozen_steps=frozen_steps if frozen is not None else 0, history=hist, model_in=model_in)
        torch.cuda.synchronize()
        ref, d0 = R.step(a, ts, i, x_b, m.double().numpy(), p_b, prediction_type=pred)
        if frozen is not None and i < frozen_steps:
            mk = mask.cpu().double().numpy().reshape((n if frozen_mode == "per_image" else 1, 1, h, w))
            ref = frozen[i + 1].cpu().double().numpy() * mk + ref * (1.0 - mk)
        got = lat.cpu().double().numpy()
        bound = _bound(tab64[i], x_b, m.double().numpy(), p_b)
        err = np.abs(got - ref)
        assert np.isfinite(got).all(), f"step {i}: non-finite latents"
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), f"step {i}: max err / bound = {float((err / bound).max()):.3f} (bound = 16 fp32 units)"
        # the state the next step reads: this step's data prediction (the model's, not the blended latents), 3 roundings + 2 coefficients
        cx, ce = tab64[i, 0], tab64[i, 1]
        d_err = np.abs(x0p.cpu().double().numpy() - d0)
        assert (d_err <= U * (np.abs(cx * x_b) + np.abs(ce * m.double().numpy()))).all(), f"step {i}: x0_prev"
        assert torch.equal(hist[i + 1], lat), f"step {i}: history row"
        want_in = lat.to(mi_dtype)
        assert torch.equal(model_in[:n], want_in) and torch.equal(model_in[n:], want_in), f"step {i}: model input = cat([x'] * 2), one rounding"
        assert int(idx.item()) == i + 1
    return worst


@pytest.mark.parametrize("frozen_mode", ["off", "shared", "per_image"])
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("cfg", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_vs_restatement_per_step(shape, cfg, pred, frozen_mode):
    """orders 1, 2, 2, 1 of a 4-step table; model_in in bf16 / fp16 / fp32"""
    if frozen_mode == "per_image" and shape[0] == 1:
        frozen_mode = "shared"                # one image: a per-image mask IS the shared one
    for mi in _MI:
        worst = _walk(shape, cfg, pred, frozen_mode, mi)
        print(f"{shape} cfg={cfg} {pred} frozen={frozen_mode} {mi}: worst err / bound {worst:.3f}")


def test_advance_false_leaves_the_counter():
    from theatergen_amd import ops
    s = _sched()
    s.set_timesteps(4)
    coef = s.coef_table().to(DEV)
    g = torch.Generator().manual_seed(2)
    lat = torch.randn(1, 4, 5, 3, generator=g).to(DEV)
    x0p = torch.zeros_like(lat)
    idx = torch.full((1,), 2, dtype=torch.int32, device=DEV)
    before = lat.clone()
    ops.step_epilogue_dpm(_quantised((1, 4, 5, 3), g).to(DEV), lat, x0p, 0.0, coef, idx, has_cfg=False, advance=False)
    assert int(idx.item()) == 2 and not torch.equal(lat, before)
    with pytest.raises(ValueError):
        ops.step_epilogue_dpm(before, lat, x0p.to(torch.bfloat16), 0.0, coef, idx, has_cfg=False, advance=False)
    with pytest.raises(ValueError):
        ops.step_epilogue_dpm(before, lat, x0p, 0.0, coef[:, :4].contiguous(), idx, has_cfg=False, advance=False)
    with pytest.raises(RuntimeError, match="x0_prev"):
        ops.step_epilogue_dpm(before, lat, lat, 0.0, coef, idx, has_cfg=False, advance=False)


@pytest.mark.parametrize("shape", SHAPES)
def test_row_0_never_reads_the_state(shape):
    """x0_prev full of NaN before step 0: C = 0 rows skip the load (0 * NaN would be NaN); the walk stays finite and within the per-step bound"""
    _walk(shape, True, "epsilon", "off", torch.bfloat16, nan_state=True)


@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
def test_order_1_is_ddim_on_the_device(pred):
    """one step, same inputs: an order-1 row on DDIM's grid vs ``tg_step_epilogue``.  Both are within one bound of the same real number -> 2 bounds."""
    from theatergen_amd import ops
    from theatergen_amd.scheduler import DDIMScheduler
    d = DDIMScheduler(prediction_type=pred)
    d.set_timesteps(4)
    s = _sched(solver_order=1, prediction_type=pred)
    s.set_timesteps(timesteps=d.timesteps.tolist())
    assert s.timesteps.tolist() == R.timesteps(4, spacing="leading").tolist()
    tab64 = s.coef_table(dtype=torch.float64).numpy()
    assert (tab64[:, 4] == 0).all()
    g = torch.Generator().manual_seed(5)
    shape = (2, 4, 8, 12)
    for i in (0, 1, 3):
        x = torch.randn(shape, generator=g)
        out = _quantised((4, 4, 8, 12), g)
        idx = torch.full((1,), i, dtype=torch.int32, device=DEV)
        la, lb = x.to(DEV), x.to(DEV)
        ops.step_epilogue(out.to(DEV), la, G, d.coef_table().to(DEV), idx, advance=False, prediction_type=0 if pred == "epsilon" else 1)
        ops.step_epilogue_dpm(out.to(DEV), lb, torch.zeros_like(lb), G, s.coef_table().to(DEV), idx, advance=False)
        m = (out[:2] + G * (out[2:] - out[:2])).double().numpy()
        bound = _bound(tab64[i], x.double().numpy(), m, 0.0)
        err = np.abs(la.cpu().double().numpy() - lb.cpu().double().numpy())
        print(f"{pred} step {i}: max diff / bound {float((err / bound).max()):.3f} (allowed 2)")
        assert (err <= 2 * bound).all(), (i, float((err / bound).max()))


def test_scheduler_step_drop_in():
    """a host loop of ``scheduler.step`` over random model outputs == the restatement, per step; ``set_timesteps`` clears the state"""
    s = _sched()
    a = R.alphas_cumprod()
    g = torch.Generator().manual_seed(9)
    shape = (2, 4, 8, 12)
    x0 = torch.randn(shape, generator=g).to(DEV)
    outs = [torch.randn(shape, generator=g).to(DEV) for _ in range(4)]
    runs = []
    for rep in range(2):
        ts = s.set_timesteps(4)
        tab64 = s.coef_table(dtype=torch.float64).numpy()
        x, rows = x0, []
        for i, t in enumerate(ts):
            x_b = x.cpu().double().numpy()
            p_b = s._x0_prev.cpu().double().numpy() if i else np.zeros(shape)
            nx = s.step(outs[i], t, x).prev_sample
            assert nx.dtype == x.dtype and nx.shape == x.shape and nx.data_ptr() != x.data_ptr()
            m = outs[i].cpu().double().numpy()
            ref, _ = R.step(a, ts.tolist(), i, x_b, m, p_b)
            err = np.abs(nx.cpu().double().numpy() - ref)
            assert (err <= _bound(tab64[i], x_b, m, p_b)).all(), (rep, i)
            rows.append(nx)
            x = nx
        runs.append(torch.stack(rows))
    assert torch.equal(runs[0], runs[1]), "set_timesteps starts the same chain again, bit for bit"
    s.set_timesteps(4)
    first = s.step(outs[0], s.timesteps[0], x0, return_dict=False)
    assert isinstance(first, tuple) and torch.equal(first[0], runs[0][0])
    with pytest.raises(ValueError, match="in order"):
        s.step(outs[0], s.timesteps[2], x0)
    with pytest.raises(ValueError, match="not in the schedule"):
        s.step(outs[0], 7, x0)
    # a storage-dtype sample comes back in its dtype
    s.set_timesteps(4)
    assert s.step(outs[0].half(), s.timesteps[0], x0.half()).prev_sample.dtype == torch.float16


# ---- the engine ---------------------------------------------------------------------------------------------------------------------------------------
def _unet(variant, dtype):
    """a fresh tiny UNet per test (the IP scale is state on it): (cfg, unet, the storage-rounded weights the oracle sees)"""
    from tests.test_hotpath_gpu import _build
    from theatergen_amd import config
    cfg = {"conv": config.tiny(), "linear": config.tiny(linear=True), "xl": config.tiny(xl=True)}[variant]
    return (cfg,) + _build(cfg, dtype)


def _engine(unet, sched, use_graph, n=2, steps=5, **kw):
    from theatergen_amd.pipelines import DenoiseEngine
    return DenoiseEngine(unet, sched, n_img=n, height=128, width=128, num_inference_steps=steps, guidance_scale=G, enc_len=81, use_graph=use_graph, **kw)


def _oracle_dpm_loop(cfg, sd_r, lat, enc, dtype, ts, pred="epsilon", ip_scale=0.4, frozen=None, mask=None, frozen_steps=0, extra=None):
    """the free-running host loop: oracle UNet on the storage-rounded input, CFG, the restated step (+ the frozen-mask blend); fp64 state"""
    from oracle import unet as ou
    a = R.alphas_cumprod(beta_schedule="scaled_linear")
    x, d0, rows = lat.double().numpy(), None, [lat.double().numpy()]
    n = lat.shape[0]
    for i, t in enumerate(ts):
        xt = torch.from_numpy(x).float()
        mi = torch.cat([xt] * 2).to(dtype).float()
        if extra is not None:
            out = extra(mi, t)
        else:
            out = ou.unet_forward(cfg, sd_r, mi, t, enc.to(dtype).float().cpu(), ip_scale=ip_scale)
        m = (out[:n] + G * (out[n:] - out[:n])).double().numpy()
        x, d0 = R.step(a, ts, i, xt.double().numpy(), m, d0, prediction_type=pred)
        if frozen is not None and i < frozen_steps:
            mk = mask.double().numpy()
            x = frozen[i + 1].double().numpy() * mk + x * (1.0 - mk)
        rows.append(x)
    return torch.from_numpy(x).float(), torch.from_numpy(np.stack(rows)).float()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_engine_graph_replay_is_eager_and_tracks_the_oracle_loop(dtype):
    """5 steps (orders 1, 2, 2, 2, 1), 2 images.  Yardstick of the oracle comparison: ``net_tol`` of tests/test_hotpath_gpu.py, allowance 2 x it: a 2M
    row weights TWO UNet outputs by |B| + |C| <= 1 + 1 / r0 ~ 2 at equal lambda spacing where DDIM weights one."""
    from tests import parity_metrics as pm
    from tests.test_hotpath_gpu import close, net_tol
    cfg, unet, sd_r = _unet("conv", dtype)
    g = torch.Generator().manual_seed(8)
    n, steps = 2, 5
    lat = torch.randn(n, 4, 16, 16, generator=g)
    enc = torch.randn(2 * n, 81, cfg.cross_attention_dim, generator=g) * 0.5
    sched = _sched()
    hist = {}
    for use_graph in (False, True):
        eng = _engine(unet, sched, use_graph)
        assert eng.kind == "dpm" and eng.coef.shape == (steps, 8) and eng.x0_prev.data_ptr() != eng.latents.data_ptr()
        eng.set_conditioning(enc.to(DEV, dtype))
        h = eng.run(lat).clone()
        assert h.shape == (steps + 1, n, 4, 16, 16) and torch.equal(h[0].cpu(), lat)
        hist[use_graph] = h
        if use_graph:
            state = eng.x0_prev.data_ptr()
            again = eng.run(lat).clone()
            assert torch.equal(again, h), "a second replay (the state tensor still holds the first run's last prediction) differs"
            assert eng.x0_prev.data_ptr() == state
            enc2 = torch.randn(2 * n, 81, cfg.cross_attention_dim, generator=g) * 0.5
            eng.set_conditioning(enc2.to(DEV, dtype))
            h2 = eng.run(lat).clone()
            eng_e = _engine(unet, sched, False)
            eng_e.set_conditioning(enc2.to(DEV, dtype))
            assert torch.equal(h2, eng_e.run(lat)), "graph replay with refreshed conditioning != eager"
    assert torch.equal(hist[False], hist[True]), "graph replay is not bit-identical to eager launches"
    ref, _ = _oracle_dpm_loop(cfg, sd_r, lat, enc, dtype, [int(t) for t in sched.timesteps.tolist()])
    m = pm.metrics(hist[True][-1], ref)
    print(f"DPM engine vs oracle loop, {dtype}: rel-L2 {m['rel_l2']:.3e} max-rel {m['max_rel']:.3e} (allowed {net_tol(dtype):.1e} / {2 * net_tol(dtype):.1e})")
    close(hist[True][-1], ref, 2 * net_tol(dtype), f"dpm denoise loop vs oracle {dtype}")


def test_engine_frozen_mask():
    from tests.test_hotpath_gpu import close, net_tol
    dtype = torch.bfloat16
    cfg, unet, sd_r = _unet("conv", dtype)
    g = torch.Generator().manual_seed(21)
    steps = 5
    lat = torch.randn(2, 4, 16, 16, generator=g)
    enc = torch.randn(4, 81, cfg.cross_attention_dim, generator=g) * 0.5
    frozen = torch.randn(steps + 1, 2, 4, 16, 16, generator=g)
    mask = (torch.rand(16, 16, generator=g) > 0.5).float()
    sched = _sched()
    hs = []
    for use_graph in (False, True):
        eng = _engine(unet, sched, use_graph)
        eng.set_conditioning(enc.to(DEV, dtype))
        eng.set_frozen(frozen.to(DEV), mask.to(DEV), 2)
        hs.append(eng.run(lat).clone())
    assert torch.equal(hs[0], hs[1])
    mb = mask.bool()
    for i in (1, 2):
        assert torch.equal(hs[1][i][:, :, mb].cpu(), frozen[i][:, :, mb]), "inside the mask the frozen latents are copied verbatim"
    assert not torch.equal(hs[1][3][:, :, mb].cpu(), frozen[3][:, :, mb])
    ref, _ = _oracle_dpm_loop(cfg, sd_r, lat, enc, dtype, [int(t) for t in sched.timesteps.tolist()], frozen=frozen, mask=mask, frozen_steps=2)
    close(hs[1][-1], ref, 2 * net_tol(dtype), "dpm frozen-mask loop vs oracle")


def test_engine_fast_schedule_subset():
    """``timesteps=`` is the walked list: the table's t and r0 follow the kept timesteps"""
    from theatergen_amd.schedule import get_fast_schedule
    dtype = torch.bfloat16
    cfg, unet, sd_r = _unet("conv", dtype)
    g = torch.Generator().manual_seed(23)
    lat = torch.randn(2, 4, 16, 16, generator=g)
    enc = torch.randn(4, 81, cfg.cross_attention_dim, generator=g) * 0.5
    sched = _sched()
    sched.set_timesteps(8)
    fast = get_fast_schedule(sched.timesteps, 2, 2)
    assert len(fast) == 5
    hs = []
    for use_graph in (False, True):
        eng = _engine(unet, sched, use_graph, steps=8, timesteps=fast)
        assert eng.steps == 5 and torch.equal(eng.coef.cpu(), sched.coef_table(fast))
        eng.set_conditioning(enc.to(DEV, dtype))
        hs.append(eng.run(lat).clone())
    assert hs[0].shape[0] == 6 and torch.equal(hs[0], hs[1])
    from tests.test_hotpath_gpu import close, net_tol
    ref, _ = _oracle_dpm_loop(cfg, sd_r, lat, enc, dtype, [int(t) for t in fast.tolist()])
    close(hs[1][-1], ref, 2 * net_tol(dtype), "dpm fast-schedule loop vs oracle")


@pytest.mark.parametrize("variant", ["linear", "xl"])
def test_engine_other_plans(variant):
    """``tiny(linear=True)`` with v-prediction (the SD-2.1 shape of things) and ``tiny(xl=True)`` with ``added_cond_kwargs``: graph == eager"""
    dtype = torch.bfloat16
    cfg, unet, sd_r = _unet(variant, dtype)
    g = torch.Generator().manual_seed(29)
    lat = torch.randn(2, 4, 16, 16, generator=g)
    enc = torch.randn(4, 81, cfg.cross_attention_dim, generator=g) * 0.5
    added = None
    if variant == "xl":
        added = {"text_embeds": torch.randn(4, 64, generator=g).to(DEV, dtype), "time_ids": torch.tensor([[128., 128., 0., 0., 128., 128.]] * 4, device=DEV)}
    sched = _sched(prediction_type="v_prediction" if variant == "linear" else "epsilon")
    hs = []
    for use_graph in (False, True):
        eng = _engine(unet, sched, use_graph)
        eng.set_conditioning(enc.to(DEV, dtype), added)
        hs.append(eng.run(lat).clone())
    assert torch.isfinite(hs[0]).all() and torch.equal(hs[0], hs[1])
    assert not torch.equal(hs[0][-1], hs[0][0])


def test_unknown_scheduler_is_a_type_error():
    from theatergen_amd.pipelines import DenoiseEngine
    cfg, unet, _ = _unet("conv", torch.bfloat16)

    class PNDMScheduler:
        config = type("C", (), {"prediction_type": "epsilon"})()
        timesteps = torch.arange(5)

        def set_timesteps(self, n):
            pass
    with pytest.raises(TypeError, match="DPMSolverMultistepScheduler"):
        DenoiseEngine(unet, PNDMScheduler(), n_img=1, height=128, width=128, num_inference_steps=5)


# ---- the stage functions and generate / decode ---------------------------------------------------------------------------------------------------------
def _stage_setup(monkeypatch, full_vae=False):
    from tests.test_hotpath_gpu import _build_vae, _build_vae_full
    from tests.test_round6_gpu import _FakeTextPipe, _image_tokens_of
    from theatergen_amd.ip_adapter import IPAdapter
    from theatergen_amd.vae import tiny_vae_config
    dtype = torch.bfloat16
    cfg, unet, sd_r = _unet("conv", dtype)
    vcfg = tiny_vae_config()
    vae, vsd = (_build_vae_full if full_vae else _build_vae)(vcfg, dtype)
    pipe = _FakeTextPipe(unet, vae, cfg.cross_attention_dim)
    pipe.scheduler = _sched()
    ad = IPAdapter(pipe, None, None, DEV, num_tokens=4)
    monkeypatch.setattr(ad, "get_image_embeds", lambda pil_image=None, clip_image_embeds=None: _image_tokens_of(pil_image, cfg.cross_attention_dim, DEV, dtype))
    return dtype, cfg, unet, sd_r, vcfg, vae, vsd, pipe, ad


def test_generate_semantic_guidance_with_the_dpm_scheduler(tmp_path, monkeypatch):
    """the round-6 stage-1 test's host loop with the restated multistep step swapped in; 4 steps, and the fast schedule"""
    from PIL import Image
    from tests.test_hotpath_gpu import close, net_tol
    from tests.test_round6_gpu import _image_tokens_of
    from theatergen_amd import pipelines
    from theatergen_amd.schedule import get_fast_schedule
    dtype, cfg, unet, sd_r, vcfg, vae, vsd, pipe, ad = _stage_setup(monkeypatch)
    monkeypatch.chdir(tmp_path)
    Image.fromarray(np.full((32, 32, 3), 90, np.uint8)).save("model.png")
    db = str(tmp_path) + "/db_"
    lat = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(31)).to(dtype)

    def enc_of(prompt, pil):
        pos, neg = pipe.encode_prompt(prompt, negative_prompt=pipelines.SINGLE_OBJECT_NEGATIVE_PROMPT)
        img, unc = _image_tokens_of(pil, cfg.cross_attention_dim, DEV, dtype)
        return torch.cat([torch.cat([neg, unc], 1), torch.cat([pos, img], 1)], 0)

    kw = dict(guidance_scale=G, return_saved_cross_attn=True, return_box_vis=True, save_all_latents=True, obj_id=7)
    out = pipelines.generate_semantic_guidance("story", 123, "1.5", "a red fox", db, 0, ad, None, lat.to(DEV), None, 4, None, None, None, **kw)
    latents, image, saved, image2, latents_all = out
    assert saved == [{}] * 4 and latents_all.shape == (5, 1, 4, 16, 16) and latents.dtype == dtype
    ts = [int(t) for t in pipe.scheduler.timesteps.tolist()]
    assert ts == R.timesteps(4).tolist()
    ref, rows = _oracle_dpm_loop(cfg, sd_r, lat.float(), enc_of("full-body picture of a red fox", Image.open("model.png")), dtype, ts, ip_scale=0.0)
    close(latents, ref, 2 * net_tol(dtype), "generate_semantic_guidance (DPM): first appearance")
    close(latents_all, rows, 2 * net_tol(dtype), "generate_semantic_guidance (DPM): latents_all")
    # the fast schedule: a subset of the 6-step grid, walked as its own list
    out3 = pipelines.generate_semantic_guidance("story", 123, "1.5", "a red fox", db, 0, ad, None, lat.to(DEV), None, 6, None, None, None,
                                                **{**kw, "fast_after_steps": 2, "fast_rate": 2})
    fast = get_fast_schedule(torch.from_numpy(R.timesteps(6)), 2, 2)
    assert out3[4].shape[0] == len(fast) + 1
    ref3, _ = _oracle_dpm_loop(cfg, sd_r, lat.float(), enc_of("full-body picture of a red fox", Image.open(db + "7.png")), dtype, [int(t) for t in fast.tolist()],
                               ip_scale=0.4)
    close(out3[0], ref3, 2 * net_tol(dtype), "generate_semantic_guidance (DPM): fast schedule")
    with pytest.raises(NotImplementedError):                       # the 'xl' branch keeps requiring Euler
        pipelines.generate_semantic_guidance("story", 1, "xl", "x", db, 0, ad, None, lat.to(DEV), None, 4, None, None, None, obj_id=7)


def test_final_image_generation_with_the_dpm_scheduler(monkeypatch):
    """the round-6 stage-2 test's host loop (ControlNet + UNet + frozen-mask replace) with the restated multistep step swapped in"""
    from PIL import Image
    from oracle import controlnet as oc
    from oracle import unet as ou
    from tests.test_hotpath_gpu import _build_controlnet, close, net_tol
    from tests.test_round6_gpu import _image_tokens_of
    from theatergen_amd import pipelines
    dtype, cfg, unet, sd_u, vcfg, vae, vsd, pipe, ad = _stage_setup(monkeypatch, full_vae=True)
    net, sd_c = _build_controlnet(cfg, dtype)
    cnpipe = type("CNPipe", (), {"controlnet": net})()
    H = W = 128
    steps, frozen_steps, bg_seed = 4, 3, 11
    g = torch.Generator().manual_seed(41)
    pasted = Image.fromarray((torch.rand(H, W, 3, generator=g) * 255).to(torch.uint8).numpy())
    m512 = np.full((H, W), 255, np.uint8)
    m512[40:100, 24:80] = 0
    inp_mask = Image.fromarray(m512, mode="L")
    char_img = Image.fromarray(np.full((32, 32, 3), 140, np.uint8))
    text = (torch.randn(2, 77, cfg.cross_attention_dim, generator=g) * 0.5).to(DEV, dtype)
    latents_all = torch.zeros(steps + 1, 1, 4, H // 8, W // 8, device=DEV)
    processor = lambda arr: Image.fromarray(255 - arr)
    latents, images = pipelines.final_image_generation("1.5", processor, cnpipe, 1, "two foxes in a park", "lowres", "a park", [char_img], None, 0, H, W,
                                                       bg_seed, inp_mask, pasted, ad, None, latents_all, torch.ones(16, 16), None, (text, text[:1], text[1:]),
                                                       steps, frozen_steps, guidance_scale=G)
    assert images.shape == (1, H, W, 3) and images.dtype == np.uint8 and latents.shape == (1, 4, 16, 16)
    ts = [int(t) for t in pipe.scheduler.timesteps.tolist()]
    assert ts == R.timesteps(steps).tolist()
    # the frozen rows are the scheduler's add_noise at ITS timesteps: sqrt(a_t) x0 + sqrt(1 - a_t) noise, so row k+1 / row j+1 differ as the grid says
    mask = torch.from_numpy(1 - (np.array(inp_mask.resize((16, 16)).convert("L")).astype(np.float32) / 255.0 > 0).astype(np.float32))
    pos, neg = pipe.encode_prompt("two foxes in a park", negative_prompt="lowres")
    img_t, unc_t = _image_tokens_of(char_img, cfg.cross_attention_dim, DEV, dtype)
    ip_rows = torch.cat([torch.cat([neg, unc_t], 1), torch.cat([pos, img_t], 1)], 0)
    cond = torch.from_numpy(np.asarray(Image.fromarray(255 - np.asarray(pasted)).resize((W, H), resample=Image.LANCZOS)).astype(np.float32) / 255.0).permute(2, 0, 1)[None]
    cond = torch.cat([cond] * 2).to(dtype).float()
    frozen = latents_all.cpu()

    def net_out(mi, t):
        rd, rm = oc.controlnet_forward(cfg, sd_c, mi, t, text.float().cpu(), cond, 1.0, cross_mode="cn")
        rd = [d.to(dtype).float() for d in rd]
        return ou.unet_forward(cfg, sd_u, mi, t, ip_rows.float().cpu(), ip_scale=0.1, down_block_additional_residuals=rd,
                               mid_block_additional_residual=rm.to(dtype).float())
    ref, _ = _oracle_dpm_loop(cfg, sd_u, frozen[0], None, dtype, ts, frozen=frozen, mask=mask, frozen_steps=frozen_steps, extra=net_out)
    close(latents, ref, 2 * net_tol(dtype), "final_image_generation (DPM): ControlNet + UNet + frozen-mask loop")


def test_generate_and_decode(monkeypatch):
    """``generate`` returns ``(latents, uint8 images)``; the images are the restated ``(x / 2 + 0.5).clamp(0, 1) * 255`` rounding of the VAE output"""
    from tests.test_hotpath_gpu import close, net_tol
    from theatergen_amd import pipelines
    dtype, cfg, unet, sd_r, vcfg, vae, vsd, pipe, ad = _stage_setup(monkeypatch)
    ad.set_scale(0.4)
    g = torch.Generator().manual_seed(51)
    lat = torch.randn(2, 4, 16, 16, generator=g).to(DEV, dtype)
    text = (torch.randn(4, 81, cfg.cross_attention_dim, generator=g) * 0.5).to(DEV, dtype)
    latents, images = pipelines.generate(ad, None, lat, (text, text[:2], text[2:]), 4, guidance_scale=G)
    assert latents.shape == lat.shape and latents.dtype == dtype
    assert images.shape == (2, 128, 128, 3) and images.dtype == np.uint8
    ts = [int(t) for t in pipe.scheduler.timesteps.tolist()]
    assert ts == R.timesteps(4).tolist()
    ref, _ = _oracle_dpm_loop(cfg, sd_r, lat.float().cpu(), text.cpu(), dtype, ts)
    close(latents, ref, 2 * net_tol(dtype), "generate (DPM) vs the host loop")
    dec = vae.decode(1 / 0.18215 * latents).sample
    want = ((dec.float() / 2 + 0.5).clamp(0, 1).cpu().permute(0, 2, 3, 1).numpy() * 255).round().astype("uint8")
    assert np.array_equal(images, want) and np.array_equal(pipelines.decode(vae, latents), want)
    # no_set_timesteps: the scheduler's own grid is walked and left in place; a count mismatch is a ValueError
    lead = R.timesteps(4, spacing="leading").tolist()
    pipe.scheduler.set_timesteps(timesteps=lead)
    lat2, _ = pipelines.generate(ad, None, lat, (text, text[:2], text[2:]), 4, guidance_scale=G, no_set_timesteps=True)
    assert pipe.scheduler.timesteps.tolist() == lead
    ref2, _ = _oracle_dpm_loop(cfg, sd_r, lat.float().cpu(), text.cpu(), dtype, lead)
    close(lat2, ref2, 2 * net_tol(dtype), "generate (DPM, no_set_timesteps) vs the host loop")
    with pytest.raises(ValueError, match="num_inference_steps"):
        pipelines.generate(ad, None, lat, (text, text[:2], text[2:]), 5, no_set_timesteps=True)
