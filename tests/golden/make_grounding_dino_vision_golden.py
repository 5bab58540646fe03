"""Regenerate tests/golden/grounding_dino_vision.npz from a tiny ``transformers.GroundingDinoModel`` (fp32, CPU): its ``backbone`` and
``input_proj_vision``, the part ``theatergen_amd.grounding_dino.GroundingDinoVisionFront`` runs.

Swin ``embed_dim 32, depths [2,2,2,2], num_heads [1,2,4,8], window 7, out_indices [2,3,4]``; ``d_model 64``, 4 feature levels.  The weights are NOT
stored: ``make_weights`` draws them from numpy's legacy ``RandomState`` in sorted-name order — parameter = base + s * randn, base 1 for norm weights
and 0 otherwise, s = 0.25 for the relative-position bias tables and 0.05 for everything else, rounded to fp16-representable values.  The file keeps
(sum, sum of squares) per parameter in float64, so a drifted generator fails loudly.  The input is the closed-form image

    x[c, i, j] = ((131 i + 71 j + 53 c) mod 251) / 125 - 1                    3 x 232 x 200

with a pixel mask that is zero for rows >= 200 and columns >= 180.  The stage grids are 58 x 50, 29 x 25, 15 x 13 and 8 x 7: every stage pads to a
multiple of 7, every merge sees an odd side, and the last stage is as small as a stage may be.

Stored, float32: the three raw feature maps, the four projected levels, the four position embeddings and masks, and the hidden state after block 0
(unshifted) and block 1 (shifted) of stage 1 at the grid rows ``ROWS`` (all 50 columns each: the first and last rows, which wrap into one window
under the shift, both sides of the window seams at 7 / 14 and 49 / 56, and the rows of the last, padded window row).

    python tests/golden/make_grounding_dino_vision_golden.py
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "grounding_dino_vision.npz")
SEED = 2024
EMBED, DEPTHS, HEADS, OUT_INDICES, D_MODEL = 32, (2, 2, 2, 2), (1, 2, 4, 8), (2, 3, 4), 64
IMAGE_HW, MASK_HW = (232, 200), (200, 180)
ROWS = (0, 1, 2, 3, 6, 7, 13, 14, 48, 49, 52, 53, 54, 55, 56, 57)
BB = "backbone.conv_encoder.model."


def config(decoder_layers=1):
    from transformers import GroundingDinoConfig
    return GroundingDinoConfig(
        backbone_config=dict(model_type="swin", embed_dim=EMBED, depths=list(DEPTHS), num_heads=list(HEADS), window_size=7, out_indices=list(OUT_INDICES)),
        d_model=D_MODEL, num_feature_levels=4, encoder_layers=1, decoder_layers=decoder_layers, encoder_attention_heads=2, decoder_attention_heads=2,
        encoder_ffn_dim=64, decoder_ffn_dim=64, num_queries=10, disable_custom_kernels=True,
        text_config=dict(model_type="bert", hidden_size=32, num_hidden_layers=1, num_attention_heads=2, intermediate_size=64, vocab_size=100,
                         max_position_embeddings=64))


def param_shapes():
    """{GroundingDinoModel parameter name: shape} under ``backbone.`` and ``input_proj_vision.``"""
    sw = BB + "swin."
    sh = {sw + "embeddings.patch_embeddings.projection.weight": (EMBED, 3, 4, 4), sw + "embeddings.patch_embeddings.projection.bias": (EMBED,),
          sw + "embeddings.norm.weight": (EMBED,), sw + "embeddings.norm.bias": (EMBED,)}
    for i, depth in enumerate(DEPTHS):
        C = EMBED * 2 ** i
        for j in range(depth):
            p = f"{sw}encoder.layers.{i}.blocks.{j}."
            for lin in ("q_proj", "k_proj", "v_proj", "o_proj"):
                sh[p + f"attention.{lin}.weight"], sh[p + f"attention.{lin}.bias"] = (C, C), (C,)
            sh[p + "attention.relative_position_bias.relative_position_bias_table"] = (169, HEADS[i])
            for ln in ("layernorm_before", "layernorm_after"):
                sh[p + ln + ".weight"], sh[p + ln + ".bias"] = (C,), (C,)
            sh[p + "mlp.fc1.weight"], sh[p + "mlp.fc1.bias"] = (4 * C, C), (4 * C,)
            sh[p + "mlp.fc2.weight"], sh[p + "mlp.fc2.bias"] = (C, 4 * C), (C,)
        if i + 1 < len(DEPTHS):
            d = f"{sw}encoder.layers.{i}.downsample."
            sh[d + "reduction.weight"], sh[d + "norm.weight"], sh[d + "norm.bias"] = (2 * C, 4 * C), (4 * C,), (4 * C,)
    Cl = EMBED * 2 ** (len(DEPTHS) - 1)
    sh[sw + "layernorm.weight"], sh[sw + "layernorm.bias"] = (Cl,), (Cl,)
    for idx in OUT_INDICES:
        C = EMBED * 2 ** (idx - 1)
        sh[f"{BB}hidden_states_norms.stage{idx}.weight"], sh[f"{BB}hidden_states_norms.stage{idx}.bias"] = (C,), (C,)
    for level, idx in enumerate(OUT_INDICES):
        sh[f"input_proj_vision.{level}.0.weight"] = (D_MODEL, EMBED * 2 ** (idx - 1), 1, 1)
    sh[f"input_proj_vision.{len(OUT_INDICES)}.0.weight"] = (D_MODEL, Cl, 3, 3)
    for level in range(len(OUT_INDICES) + 1):
        sh[f"input_proj_vision.{level}.0.bias"] = (D_MODEL,)
        sh[f"input_proj_vision.{level}.1.weight"], sh[f"input_proj_vision.{level}.1.bias"] = (D_MODEL,), (D_MODEL,)
    return sh


def _is_norm_weight(name):
    """LayerNorm weights, and the GroupNorm of a projection level: ``input_proj_vision.<level>.1.weight`` (``.<level>.0.`` is its convolution)"""
    if name.startswith("input_proj_vision."):
        return name.split(".")[2:] == ["1", "weight"]
    return name.endswith(".weight") and "norm" in name


def make_weights(seed=SEED):
    """{name: float32 array of fp16-representable values}, drawn in sorted-name order from RandomState(seed)."""
    rs = np.random.RandomState(seed)
    out = {}
    for name, shape in sorted(param_shapes().items()):
        base = 1.0 if _is_norm_weight(name) else 0.0
        s = 0.25 if name.endswith("relative_position_bias_table") else 0.05
        out[name] = (base + s * rs.standard_normal(shape)).astype(np.float16).astype(np.float32)
    return out


def golden_image():
    h, w = IMAGE_HW
    i = np.arange(h, dtype=np.int64)[None, :, None]
    j = np.arange(w, dtype=np.int64)[None, None, :]
    c = np.arange(3, dtype=np.int64)[:, None, None]
    return (((131 * i + 71 * j + 53 * c) % 251).astype(np.float32) / np.float32(125.0) - np.float32(1.0))[None]


def golden_mask():
    m = np.zeros((1,) + IMAGE_HW, np.int64)
    m[:, :MASK_HW[0], :MASK_HW[1]] = 1
    return m


def weight_checksums(w):
    return np.array([[v.astype(np.float64).sum(), (v.astype(np.float64) ** 2).sum()] for _, v in sorted(w.items())])


def load_model(dtype=None):
    """the tiny ``GroundingDinoModel`` with the golden vision weights (the rest keeps transformers' seeded initialisation)"""
    import torch
    from transformers import GroundingDinoModel
    torch.manual_seed(0)
    m = GroundingDinoModel(config()).eval().float()
    w = make_weights()
    sd = m.state_dict()
    vision = {k for k in sd if k.startswith("backbone.") or k.startswith("input_proj_vision.")}
    assert vision == set(w) and all(tuple(sd[k].shape) == w[k].shape for k in w), "param_shapes() is out of step with transformers"
    from theatergen_amd.grounding_dino import expected_names
    assert expected_names(m.config) == vision, "GroundingDinoVisionFront.expected_names is out of step with transformers"
    missing, unexpected = m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
    assert not unexpected and not any(k in w for k in missing)
    return m if dtype is None else m.to(dtype)


def make(path=PATH):
    import torch
    m = load_model()
    hs = []
    blocks = m.backbone.conv_encoder.model.swin.encoder.layers[0].blocks
    hooks = [b.register_forward_hook(lambda _m, _i, o: hs.append((o[0] if isinstance(o, tuple) else o).detach().clone())) for b in blocks]
    pv, pm = torch.from_numpy(golden_image()), torch.from_numpy(golden_mask())
    with torch.no_grad():
        feats, pos = m.backbone(pv, pm)
        proj = [m.input_proj_vision[i](f) for i, (f, _) in enumerate(feats)]
        proj.append(m.input_proj_vision[3](feats[-1][0]))
        mask3 = torch.nn.functional.interpolate(pm[None].float(), size=proj[3].shape[-2:]).to(torch.bool)[0]
        pos = list(pos) + [m.backbone.position_embedding(proj[3], mask3)]
    for h in hooks:
        h.remove()
    masks = [mk for _, mk in feats] + [mask3]
    H, W = IMAGE_HW[0] // 4, IMAGE_HW[1] // 4
    assert len(hs) == 2 and hs[0].shape == (1, H * W, EMBED)
    assert [tuple(f.shape[-2:]) for f, _ in feats] == [(29, 25), (15, 13), (8, 7)] and tuple(proj[3].shape[-2:]) == (4, 4)
    rows = list(ROWS)
    out = dict(rows=np.array(rows), weight_checksums=weight_checksums(make_weights()),
               hidden0=hs[0].reshape(H, W, EMBED)[rows].numpy(), hidden1=hs[1].reshape(H, W, EMBED)[rows].numpy())
    for i in range(3):
        out[f"feature{i}"] = feats[i][0][0].numpy()
    for i in range(4):
        out[f"proj{i}"], out[f"pos{i}"], out[f"mask{i}"] = proj[i][0].numpy(), pos[i][0].float().numpy(), masks[i][0].numpy()
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    import sys
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    make()
