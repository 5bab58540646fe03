"""GPU: the production plans, one GEMM / attention launch at a time, against the fp64 restatement of the C-ABI contract.

The network tests (test_hotpath_gpu.py, test_parity_fullsize_gpu.py) check whole UNets at rel-L2 1e-2; the kernel tests check hand-picked
shapes on fresh iid operands.  Here every ``ops.gemm`` / ``ops.attention`` call of the real plans goes through ``tests.launch_check``:
read extents, A / W alignment, read-write overlap and stray writes on every launch; the fp64 reference, the ``ln_rows`` / ``gn_out``
side outputs and a replay on NaN-filled outputs and workspace on the first launch of every distinct key.  Plans run eagerly (the
wrapper synchronises; no graph capture).  At the end the families the plans reached are checked against a frozen list, so that a
planner change that silently moves a family out of this test's reach fails here and names it.
"""
import gc as _gc

import pytest
import torch

from tests import launch_check as lc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEEN = {}                  # plan -> families reached (filled by the plan tests, checked by test_families_reached)

# Families the six plans reach, as observed on MI355X (kernel kind 0 GEMM, 1 implicit-GEMM conv, 2 LDS-halo conv, 4 slab conv, 6 LayerNorm-folded
# projection, 7 ping-pong).  Kind 3 (the 256 x 256 big tile) is not reached: it takes only GEGLU launches with M >= 16384 and 1024 tiles, and the
# ping-pong kernel takes those first; kind 5 no longer exists.  No launch of these plans passes res IS out (the checker allows it, nothing
# requires it).
REQUIRED = {
    "kind0", "kind1", "kind2", "kind4", "kind6", "kind7", "pp256", "pp160",
    "slab_split_whole_row", "slab_split_patch", "slab_whole_row", "slab_patch",
    "gn_out_written", "ln_fold", "ln_fold_rows", "geglu", "n_split", "a_coef", "two_source", "batched_a", "padded_pitch", "bvec",
    "stride2", "upsample", "pad_mode",
    "attention", "attn_self_n>=4096", "attn_two_segments",
}
PLANS = ["sd15_b16", "sd15_b2", "sd21_b2_fwd_bwd", "sdxl_b2", "controlnet_b2", "vae_512"]


def _unet(cfg, dtype, T):
    from theatergen_amd import weights as W
    from theatergen_amd.unet import UNet2DConditionModel
    sd = W.random_unet_state_dict(cfg, seed=0)
    return UNet2DConditionModel.from_state_dict(cfg, sd, device=DEV, dtype=dtype, num_tokens=T, ip_scale=0.4)


def _unet_forward(cfg, dtype, T, batch, seed):
    unet = _unet(cfg, dtype, T)
    g = torch.Generator().manual_seed(seed)
    s = cfg.sample_size
    x = torch.randn(batch, 4, s, s, generator=g)
    enc = torch.randn(batch, 77 + T, cfg.cross_attention_dim, generator=g) * 0.5
    added = None
    if cfg.addition_embed_type:
        added = {"text_embeds": torch.randn(batch, 1280, generator=g).to(DEV),
                 "time_ids": torch.tensor([[float(8 * s), float(8 * s), 0., 0., float(8 * s), float(8 * s)]] * batch).to(DEV)}
    with torch.no_grad():
        out = unet(x.to(DEV, dtype), 621, enc.to(DEV, dtype), added_cond_kwargs=added, out_dtype=torch.float32).sample
    assert torch.isfinite(out).all()
    return unet, x, enc


def _run(plan):
    from theatergen_amd import config
    if plan == "sd15_b16":
        _unet_forward(config.sd15(), torch.bfloat16, 4, 16, 21)
    elif plan == "sd15_b2":
        _unet_forward(config.sd15(), torch.bfloat16, 4, 2, 2)
    elif plan == "sd21_b2_fwd_bwd":
        from tests.golden import gen_common as gcm
        from theatergen_amd.backward import latent_backward_guidance
        from theatergen_amd.scheduler import DDIMScheduler
        unet, x, enc = _unet_forward(config.sd21(), torch.bfloat16, 4, 2, 12)
        sch = DDIMScheduler()
        sch.set_timesteps(50)
        lat = x[:1].to(DEV, torch.bfloat16)
        new_lat, loss = latent_backward_guidance(None, sch, unet, enc[1:].to(DEV, torch.bfloat16), 0, gcm.GUIDANCE_BOXES[2], gcm.GUIDANCE_POSITIONS[2],
                                                 741, lat, 1e6, loss_scale=30.0, loss_threshold=0.0, max_iter=1, use_ratio_based_loss=True)
        assert torch.isfinite(new_lat).all()
    elif plan == "sdxl_b2":
        _unet_forward(config.sdxl(), torch.float16, 16, 2, 12)
    elif plan == "controlnet_b2":
        from theatergen_amd import weights as W
        from theatergen_amd.controlnet import ControlNetModel
        cfg = config.sd15()
        net = ControlNetModel.from_state_dict(cfg, W.random_controlnet_state_dict(cfg, seed=3), device=DEV, dtype=torch.bfloat16,
                                              cn_processors=True, num_tokens=4)
        g = torch.Generator().manual_seed(4)
        x = torch.randn(2, 4, 64, 64, generator=g)
        enc = torch.randn(2, 77, 768, generator=g) * 0.5
        cond = torch.rand(1, 3, 512, 512, generator=g).repeat(2, 1, 1, 1)
        with torch.no_grad():
            down, mid = net(x.to(DEV, torch.bfloat16), 401, enc.to(DEV, torch.bfloat16), cond.to(DEV, torch.bfloat16), return_dict=False)
        assert torch.isfinite(mid).all()
    elif plan == "vae_512":
        from theatergen_amd import weights as W
        from theatergen_amd.vae import AutoencoderKL, sd_vae_config
        cfg = sd_vae_config()
        vae = AutoencoderKL.from_state_dict(cfg, W.random_vae_state_dict(cfg, seed=2), device=DEV, dtype=torch.bfloat16)
        g = torch.Generator().manual_seed(17)
        img = torch.rand(1, 3, 512, 512, generator=g) * 2 - 1
        with torch.no_grad():
            lat = vae.encode(img.to(DEV, torch.bfloat16)).latent_dist.mode()
            rec = vae.decode_latents(lat.to(DEV))[0]
        assert torch.isfinite(rec).all()


@pytest.mark.parametrize("plan", PLANS)
def test_plan_launch_by_launch(plan, monkeypatch):
    chk = lc.LaunchChecker(plan).install(monkeypatch)
    try:
        _run(plan)
    finally:
        summary = chk.report()
        monkeypatch.undo()
        _gc.collect()
        torch.cuda.empty_cache()
    assert chk.launches > 0 and summary["checked_keys"] == summary["distinct_keys"]
    SEEN[plan] = set(chk.families)
    print(f"{plan}: {chk.launches} wrapped launches, {len(chk.counts)} distinct keys; not wrapped: {dict(chk.unwrapped)}")


def test_families_reached():
    if set(SEEN) != set(PLANS):
        pytest.skip("needs every plan of test_plan_launch_by_launch in the same session")
    reached = set().union(*SEEN.values())
    missing = sorted(REQUIRED - reached)
    assert not missing, f"no production launch of these families any more: {missing} (reached: {sorted(reached)})"
