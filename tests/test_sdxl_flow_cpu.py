"""CPU (no GPU): the host side of the SDXL flow — Euler / Euler-ancestral scheduler tables against the check values and a step-by-step
restatement (the fast-schedule index quirk included), the refusals, the T2I-Adapter-XL module names against the diffusers key list, and the
new C-ABI symbols."""
import pytest
import torch

from tests import sdxl_flow_reference as R


@pytest.mark.parametrize("n, t0, s0, s1, init", [(30, 958, 11.476857, 9.5435915, 11.520341), (50, 981, 13.120423, None, 13.158477)])
def test_euler_tables_match_the_check_values(n, t0, s0, s1, init):
    from theatergen_amd.scheduler import EulerAncestralDiscreteScheduler, EulerDiscreteScheduler
    for cls in (EulerDiscreteScheduler, EulerAncestralDiscreteScheduler):
        s = cls()
        ts = s.set_timesteps(n)
        assert ts.dtype == torch.float32 and ts.numel() == n and float(ts[0]) == t0 and float(ts[-1]) == 1.0
        assert torch.equal(ts[:-1] - ts[1:], torch.full((n - 1,), float(1000 // n)))
        assert s.sigmas.dtype == torch.float32 and s.sigmas.numel() == n + 1 and float(s.sigmas[-1]) == 0.0
        # the check values come from a float64 restatement; the scheduler's alphas_cumprod is fp32 as in diffusers (rel. 6e-7 apart)
        assert float(s.sigmas[0]) == pytest.approx(s0, rel=2e-6)
        if s1 is not None:
            assert float(s.sigmas[1]) == pytest.approx(s1, rel=2e-6)
        assert float(s.sigmas[-2]) == pytest.approx(0.04131448, rel=2e-6)
        assert float(s.init_noise_sigma) == pytest.approx(init, rel=2e-6)
        ts_r, sig_r, init_r = R.euler_tables(n)
        assert torch.equal(ts, ts_r) and torch.allclose(s.sigmas, sig_r, rtol=1e-6, atol=0)
        assert float(s.init_noise_sigma) == pytest.approx(init_r, rel=1e-6)
        assert s.config.prediction_type == "epsilon"


@pytest.mark.parametrize("spacing", ["linspace", "trailing"])
def test_other_spacings(spacing):
    from theatergen_amd.scheduler import EulerDiscreteScheduler
    s = EulerDiscreteScheduler(timestep_spacing=spacing, steps_offset=0)
    ts = s.set_timesteps(25)
    ts_r, sig_r, init_r = R.euler_tables(25, spacing)
    assert torch.equal(ts, ts_r) and torch.allclose(s.sigmas, sig_r, rtol=1e-6, atol=0)
    assert float(s.init_noise_sigma) == pytest.approx(float(sig_r.max()), rel=1e-6)


def test_add_noise_scale_model_input_and_ancestral_identity():
    from theatergen_amd.scheduler import EulerAncestralDiscreteScheduler, EulerDiscreteScheduler
    s = EulerDiscreteScheduler()
    s.set_timesteps(30)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, 4, 8, 8, generator=g)
    for i in (0, 7, 29):
        t = s.timesteps[i]
        want = x / ((s.sigmas[i] ** 2 + 1) ** 0.5)
        assert torch.equal(s.scale_model_input(x, t), want)
        assert s.model_input_divisor(i) == pytest.approx(R.scale_div(s.sigmas, i))
    a = EulerAncestralDiscreteScheduler()
    a.set_timesteps(30)
    for i in range(30):
        up, down = R.ancestral_sigmas(a.sigmas[i], a.sigmas[i + 1])
        assert float(up ** 2 + down ** 2) == pytest.approx(float(a.sigmas[i + 1] ** 2), rel=1e-5, abs=1e-9)
        assert 0.0 <= float(up) <= float(a.sigmas[i + 1]) + 1e-6
    assert float(a.sigmas[-1]) == 0.0 and float(R.ancestral_sigmas(a.sigmas[-2], a.sigmas[-1])[0]) == 0.0
    # add_noise: x0 + sigma(t) * noise, sigma looked up by the position of t (the host side; the device launch is tested on the GPU)
    idx = [s.index_for_timestep(t) for t in s.timesteps.tolist()]
    assert idx == list(range(30))
    with pytest.raises(ValueError):
        s.index_for_timestep(500.0)


def test_fast_schedule_walks_the_full_sigma_table():
    """models/pipelines.py:381-384 replaces ``timesteps`` and leaves ``sigmas``: step i of a fast schedule uses sigmas[i], sigmas[i + 1] of
    the FULL table (not the sigma of its own timestep)"""
    from theatergen_amd.schedule import get_fast_schedule
    from theatergen_amd.scheduler import EulerAncestralDiscreteScheduler, EulerDiscreteScheduler
    for cls, anc in ((EulerDiscreteScheduler, False), (EulerAncestralDiscreteScheduler, True)):
        s = cls()
        s.set_timesteps(30)
        fast = get_fast_schedule(s.timesteps, 10, 2)
        assert len(fast) < 30 and float(fast[11]) != float(s.timesteps[11])
        tab = s.coef_table(fast)
        assert tab.shape == (len(fast), 4) and tab.dtype == torch.float32
        for i in range(len(fast)):
            assert float(tab[i, 3]) == float(s.sigmas[i])                  # sigma_i of the full table, by position
            if anc:
                up, down = R.ancestral_sigmas(s.sigmas[i], s.sigmas[i + 1])
                assert float(tab[i, 0]) == float(down - s.sigmas[i]) and float(tab[i, 1]) == float(up)
            else:
                assert float(tab[i, 0]) == float(s.sigmas[i + 1] - s.sigmas[i]) and float(tab[i, 1]) == 0.0
            assert float(tab[i, 2]) == float(1.0 / (s.sigmas[i + 1] ** 2 + 1) ** 0.5)


@pytest.mark.parametrize("ancestral", [False, True])
def test_coef_table_against_a_step_by_step_restatement(ancestral):
    """the table applied row by row (what the device epilogue does) = the restated Euler / Euler-ancestral step per step"""
    from theatergen_amd.scheduler import EulerAncestralDiscreteScheduler, EulerDiscreteScheduler
    s = (EulerAncestralDiscreteScheduler if ancestral else EulerDiscreteScheduler)()
    s.set_timesteps(12)
    tab = s.coef_table()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 4, 8, 8, generator=g) * float(s.init_noise_sigma)
    x_r = x.clone()
    for i in range(12):
        eps = torch.randn(1, 4, 8, 8, generator=g)
        nz = torch.randn(1, 4, 8, 8, generator=g)
        x = x + eps * tab[i, 0] + tab[i, 1] * nz
        x_r = R.euler_step(x_r, eps, s.sigmas, i, ancestral, nz)
        assert torch.allclose(x, x_r, rtol=1e-6, atol=1e-6)
        if i + 1 < 12:
            assert float(tab[i, 2]) == pytest.approx(1.0 / R.scale_div(s.sigmas, i + 1), rel=1e-7)
    assert float(tab[-1, 2]) == 1.0                                      # after the last step: sigma = 0


def test_refusals():
    from theatergen_amd.scheduler import EulerAncestralDiscreteScheduler, EulerDiscreteScheduler
    for cls in (EulerDiscreteScheduler, EulerAncestralDiscreteScheduler):
        with pytest.raises(NotImplementedError, match="v_prediction"):
            cls(prediction_type="v_prediction")
        with pytest.raises(NotImplementedError, match="Karras"):
            cls(use_karras_sigmas=True)
        with pytest.raises(NotImplementedError, match="spacing"):
            cls(timestep_spacing="custom")
    s = EulerDiscreteScheduler()
    s.set_timesteps(10)
    x = torch.zeros(1, 4, 8, 8)
    with pytest.raises(NotImplementedError, match="s_churn"):
        s.step(x, s.timesteps[0], x, s_churn=1.0)


def test_t2i_adapter_module_names_match_diffusers():
    from theatergen_amd import weights
    from theatergen_amd.t2i_adapter import T2IAdapter
    with torch.device("meta"):
        m = T2IAdapter(in_channels=3, channels=(320, 640, 1280, 1280), num_res_blocks=2, downscale_factor=16)
    names = [n for n, _ in m.named_parameters()]
    assert names == R.T2I_KEYS_XL
    shapes = weights.t2i_adapter_param_shapes()
    assert list(shapes) == R.T2I_KEYS_XL
    assert {n: tuple(p.shape) for n, p in m.named_parameters()} == dict(shapes)
    assert shapes["adapter.conv_in.weight"] == (320, 768, 3, 3) and shapes["adapter.body.2.in_conv.weight"] == (1280, 640, 1, 1)
    assert m.adapter.body[2].down and not m.adapter.body[3].down and m.adapter.body[3].in_conv is None and m.total_downscale_factor == 32
    tiny = weights.random_t2i_adapter_state_dict(seed=1, channels=(64, 128, 256, 256))
    assert tiny["adapter.body.1.in_conv.weight"].shape == (128, 64, 1, 1) and tiny["adapter.conv_in.weight"].shape == (64, 768, 3, 3)
    with pytest.raises(NotImplementedError):
        T2IAdapter(adapter_type="light_adapter")


def test_new_symbols_are_exported_and_bound():
    import os
    from theatergen_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    h = _lib.lib()
    assert _lib.ABI_VERSION == 308 and h.tg_version() == 308
    for name in ("tg_step_epilogue_sigma", "tg_pixel_unshuffle", "tg_relu", "tg_avgpool2x2", "tg_scale_repeat"):
        assert name in _lib.SIGNATURES and getattr(h, name) is not None
    # host-side argument validation (no launch): null pointers / bad factors are refused
    assert h.tg_step_epilogue_sigma(None, None, 1, 16, 4, 1, 7.5, None, None, 1, None, 0, None, None, 0, 0, None, None, 0, None) == -1
    assert b"tg_step_epilogue_sigma" in h.tg_last_error()
    assert h.tg_pixel_unshuffle(0, 16, 1, 3, 30, 32, 16, 32, None) == -1
    assert h.tg_scale_repeat(0, 16, 8, 0.8, 0, 32, None) == -1
