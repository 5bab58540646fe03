"""fp32 / float64 restatements of the SDXL flow for the tests: the diffusers 0.21.4 Euler / Euler-ancestral schedulers (SDXL base config),
T2I-Adapter-XL, and the UNet forward in T2I-Adapter mode (built from ``oracle.unet``'s block functions; ``oracle/`` itself is not changed).
Third-party semantics restated from their definitions, independent of ``theatergen_amd``."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import unet as ou

T_TRAIN = 1000


def alphas_cumprod():
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, T_TRAIN, dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - betas, dim=0)


def euler_tables(n, spacing="leading", steps_offset=1):
    """(timesteps fp32 [n], sigmas fp32 [n + 1], init_noise_sigma float) by the formulas of the SDXL base scheduler"""
    if spacing == "leading":
        ts = (np.arange(0, n) * (T_TRAIN // n)).round()[::-1].astype(np.float64) + steps_offset
    elif spacing == "linspace":
        ts = np.linspace(0, T_TRAIN - 1, n)[::-1]
    else:
        ts = np.arange(T_TRAIN, 0, -T_TRAIN / n).round().astype(np.float64) - 1
    ac = alphas_cumprod().numpy()
    sig = np.interp(ts, np.arange(T_TRAIN), ((1 - ac) / ac) ** 0.5)
    sig = np.concatenate([sig, [0.0]]).astype(np.float32)
    m = float(sig.max())
    init = m if spacing in ("linspace", "trailing") else float(np.float32(np.sqrt(np.float32(m) ** 2 + 1)))
    return torch.from_numpy(ts.astype(np.float32)), torch.from_numpy(sig), init


def ancestral_sigmas(s, s_to):
    s, s_to = torch.as_tensor(s, dtype=torch.float32), torch.as_tensor(s_to, dtype=torch.float32)
    up = (s_to ** 2 * (s ** 2 - s_to ** 2) / s ** 2) ** 0.5
    down = (s_to ** 2 - up ** 2) ** 0.5
    return up, down


def euler_step(x, eps, sigmas, i, ancestral=False, noise=None):
    """one step at index i of the (full) sigma table, fp32: x + eps (sigma_{i+1} - sigma_i)  |  x + eps (sigma_down - sigma_i) + sigma_up noise"""
    s, s_to = sigmas[i], sigmas[i + 1]
    if not ancestral:
        return x + eps * (s_to - s)
    up, down = ancestral_sigmas(s, s_to)
    return x + eps * (down - s) + up * noise


def scale_div(sigmas, i):
    return float((sigmas[i] ** 2 + 1) ** 0.5)


# ---- T2I-Adapter-XL ---------------------------------------------------------------------------------------------------------------------
T2I_KEYS_XL = (["adapter.conv_in.weight", "adapter.conv_in.bias"]
               + [f"adapter.body.{k}.{n}" for k in range(4) for n in
                  ((["in_conv.weight", "in_conv.bias"] if k in (1, 2) else [])
                   + [f"resnets.{j}.block{b}.{p}" for j in range(2) for b in (1, 2) for p in ("weight", "bias")])])


def t2i_adapter_forward(sd, x, downscale_factor=16, num_res_blocks=2):
    """fp32 diffusers ``FullAdapterXL.forward``: the four body-block outputs"""
    x = F.pixel_unshuffle(x, downscale_factor)
    x = F.conv2d(x, sd["adapter.conv_in.weight"], sd["adapter.conv_in.bias"], padding=1)
    feats = []
    for k in range(4):
        p = f"adapter.body.{k}"
        if k == 2:
            x = F.avg_pool2d(x, 2, 2, ceil_mode=True)
        if p + ".in_conv.weight" in sd:
            x = F.conv2d(x, sd[p + ".in_conv.weight"], sd[p + ".in_conv.bias"])
        for j in range(num_res_blocks):
            q = f"{p}.resnets.{j}"
            h = F.relu(F.conv2d(x, sd[q + ".block1.weight"], sd[q + ".block1.bias"], padding=1))
            x = F.conv2d(h, sd[q + ".block2.weight"], sd[q + ".block2.bias"]) + x
        feats.append(x)
    return feats


# ---- UNet forward in T2I-Adapter mode ----------------------------------------------------------------------------------------------------
def unet_forward_adapter(cfg, sd, sample, timestep, enc, features, added_cond_kwargs=None, ip_scale=1.0, num_tokens=4, cross_mode="ip"):
    """diffusers 0.21 ``UNet2DConditionModel.forward`` with ``down_block_additional_residuals=features`` and no mid residual (CPU fp32)"""
    g = ou.cfg_get
    boc = tuple(g(cfg, "block_out_channels"))
    nb = len(boc)
    down_types, up_types = tuple(g(cfg, "down_block_types")), tuple(g(cfg, "up_block_types"))
    lpb = ou._tuple(g(cfg, "layers_per_block", 2), nb)
    heads_t = ou._tuple(g(cfg, "attention_head_dim", 8), nb)
    tl_t = ou._tuple(g(cfg, "transformer_layers_per_block", 1), nb)
    lin = bool(g(cfg, "use_linear_projection", False))
    groups, eps = g(cfg, "norm_num_groups", 32), g(cfg, "norm_eps", 1e-5)
    ca = {}
    feats = list(features)
    B = sample.shape[0]
    t = torch.as_tensor(timestep).reshape(-1).expand(B)
    emb = ou._lin(sd, "time_embedding.linear_2", F.silu(ou._lin(sd, "time_embedding.linear_1",
                                                                ou.timestep_sinusoid(t, boc[0], g(cfg, "flip_sin_to_cos", True), g(cfg, "freq_shift", 0)))))
    if g(cfg, "addition_embed_type") == "text_time":
        te = ou.timestep_sinusoid(added_cond_kwargs["time_ids"].flatten(), g(cfg, "addition_time_embed_dim", 256), True, 0)
        add = torch.cat([added_cond_kwargs["text_embeds"], te.reshape(B, -1)], dim=-1)
        emb = emb + ou._lin(sd, "add_embedding.linear_2", F.silu(ou._lin(sd, "add_embedding.linear_1", add)))
    x = F.conv2d(sample, sd["conv_in.weight"], sd["conv_in.bias"], padding=1)
    res = [x]
    for i, bt in enumerate(down_types):
        cross = bt == "CrossAttnDownBlock2D"
        extra = feats.pop(0) if cross and feats else None
        for j in range(lpb[i]):
            x = ou.resnet_block(sd, f"down_blocks.{i}.resnets.{j}", x, emb, groups, eps)
            if cross:
                x = ou.transformer_2d(sd, f"down_blocks.{i}.attentions.{j}", x, enc, heads_t[i], tl_t[i], lin, groups, ca, ip_scale, num_tokens, cross_mode)
                if j == lpb[i] - 1 and extra is not None:
                    x = x + extra
            res.append(x)
        if i != nb - 1:
            x = F.conv2d(x, sd[f"down_blocks.{i}.downsamplers.0.conv.weight"], sd[f"down_blocks.{i}.downsamplers.0.conv.bias"], stride=2, padding=1)
            res.append(x)
        if not cross and feats:
            x = x + feats.pop(0)
            res[-1] = x                                       # `sample += ...` in place: the block's last skip is the same tensor
    x = ou.resnet_block(sd, "mid_block.resnets.0", x, emb, groups, eps)
    x = ou.transformer_2d(sd, "mid_block.attentions.0", x, enc, heads_t[-1], tl_t[-1], lin, groups, ca, ip_scale, num_tokens, cross_mode)
    x = ou.resnet_block(sd, "mid_block.resnets.1", x, emb, groups, eps)
    if feats and feats[0].shape == x.shape:
        x = x + feats.pop(0)
    rheads, rtl, rlpb = tuple(reversed(heads_t)), tuple(reversed(tl_t)), tuple(reversed(lpb))
    for i, bt in enumerate(up_types):
        n = rlpb[i] + 1
        skips, res = res[-n:], res[:-n]
        for j in range(n):
            x = torch.cat([x, skips[-1 - j]], dim=1)
            x = ou.resnet_block(sd, f"up_blocks.{i}.resnets.{j}", x, emb, groups, eps)
            if bt == "CrossAttnUpBlock2D":
                x = ou.transformer_2d(sd, f"up_blocks.{i}.attentions.{j}", x, enc, rheads[i], rtl[i], lin, groups, ca, ip_scale, num_tokens, cross_mode)
        if i != nb - 1:
            x = F.interpolate(x, scale_factor=2.0, mode="nearest")
            x = F.conv2d(x, sd[f"up_blocks.{i}.upsamplers.0.conv.weight"], sd[f"up_blocks.{i}.upsamplers.0.conv.bias"], padding=1)
    x = F.silu(ou._gn(sd, "conv_norm_out", x, groups, eps))
    return F.conv2d(x, sd["conv_out.weight"], sd["conv_out.bias"], padding=1)
