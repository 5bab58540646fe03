"""Regenerate tests/golden/grounding_dino_encoder.npz from ``transformers``' ``GroundingDinoEncoder`` (fp32, CPU): the part
``theatergen_amd.grounding_dino_encoder.GroundingDinoFusionEncoder`` runs.

``d_model 128, encoder_attention_heads 4, encoder_ffn_dim 1024, encoder_layers 2``, 4 levels, ``encoder_n_points 4``: deformable head dim 32, fusion
head dim 256 (2 heads), text-enhancer head dim 64.  The weights are NOT stored: ``make_weights`` draws them from numpy's legacy ``RandomState`` in
sorted-name order — parameter = base + s * randn, rounded to fp16-representable values, with base 1 for LayerNorm weights, base 0.4 and s 0.1 for the
layer-scale vectors ``vision_param`` / ``text_param``, s 0.3 for ``sampling_offsets.weight`` and ``attention_weights.weight``, s 1 for
``sampling_offsets.bias`` and s 0.05 for everything else.  (``transformers`` initialises the sampling weights to zero and the layer scale to 1e-4: with
that neither the query dependence of the sampling nor the fusion attention would be under test.)  The file keeps (sum, sum of squares) per parameter.

Inputs, batch 2: levels 29 x 25, 15 x 13, 8 x 7, 4 x 4 = 992 tokens of a 232 x 200 image; item 1's pixel mask is cut to 150 x 120 (nearest
interpolation per level, as ``transformers`` does); vision features ~ N(0, 1) and position embeddings ~ N(0, 0.5^2) from the seed; 9 text tokens with
2 and 5 padded, the self-attention masks and position ids of ``generate_masks_with_special_tokens_and_transfer_map``.

Stored, float32: per item ``ROWS`` vision tokens (every level; first / last rows and columns; both sides of item 1's padding boundary) after layer-0
fusion, after layer 0 and after layer 1, all text tokens at the same three points, and per quantity and storage dtype the error (rel-L2, max-rel) of a
ROUNDED EMULATION of the same forward: weights, inputs and every Linear / LayerNorm output rounded to the storage dtype inside the ``transformers``
encoder.  The GPU test's bound for a quantity is twice that error.

    python tests/golden/make_grounding_dino_encoder_golden.py
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "grounding_dino_encoder.npz")
SEED = 2025
D_MODEL, HEADS, FFN, LAYERS, POINTS = 128, 4, 1024, 2, 4
SHAPES = [(29, 25), (15, 13), (8, 7), (4, 4)]
IMAGE_HW, MASK_HW = (232, 200), (150, 120)
BATCH, TEXT_LEN = 2, 9
INPUT_IDS = [[101, 5, 6, 1012, 7, 8, 102, 0, 0], [101, 5, 1012, 102, 0, 0, 0, 0, 0]]
QUANTITIES = ["fusion0", "layer0", "layer1"]


def config():
    from transformers import GroundingDinoConfig
    return GroundingDinoConfig(
        backbone_config=dict(model_type="swin", embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8], window_size=7, out_indices=[2, 3, 4]),
        d_model=D_MODEL, num_feature_levels=len(SHAPES), encoder_layers=LAYERS, decoder_layers=1, encoder_attention_heads=HEADS,
        decoder_attention_heads=HEADS, encoder_ffn_dim=FFN, decoder_ffn_dim=64, encoder_n_points=POINTS, num_queries=10, disable_custom_kernels=True,
        text_config=dict(model_type="bert", hidden_size=32, num_hidden_layers=1, num_attention_heads=2, intermediate_size=64, vocab_size=2000,
                         max_position_embeddings=64))


def hf_encoder():
    import torch
    from transformers.models.grounding_dino.modeling_grounding_dino import GroundingDinoEncoder
    torch.manual_seed(0)
    return GroundingDinoEncoder(config()).eval().float()


def make_weights(seed=SEED, shapes=None):
    """{``encoder.`` name: float32 array of fp16-representable values}, drawn in sorted-name order from RandomState(seed)."""
    if shapes is None:
        shapes = {"encoder." + k: tuple(v.shape) for k, v in hf_encoder().state_dict().items()}
    rs = np.random.RandomState(seed)
    out = {}
    for name, shape in sorted(shapes.items()):
        base, s = 0.0, 0.05
        if name.endswith("_param"):
            base, s = 0.4, 0.1
        elif "norm" in name and name.endswith(".weight"):
            base = 1.0
        elif name.endswith("sampling_offsets.weight") or name.endswith("attention_weights.weight"):
            s = 0.3
        elif name.endswith("sampling_offsets.bias"):
            s = 1.0
        out[name] = (base + s * rs.standard_normal(shape)).astype(np.float16).astype(np.float32)
    return out


def weight_checksums(w):
    return np.array([[v.astype(np.float64).sum(), (v.astype(np.float64) ** 2).sum()] for _, v in sorted(w.items())])


def level_masks():
    """bool [B, H, W] per level, True = VALID pixel, by the nearest interpolation transformers uses"""
    import torch
    pm = torch.ones((BATCH,) + IMAGE_HW)
    pm[1, MASK_HW[0]:, :] = 0
    pm[1, :, MASK_HW[1]:] = 0
    return [torch.nn.functional.interpolate(pm[None], size=s).to(torch.bool)[0] for s in SHAPES]


def rows():
    """per item the stored vision tokens: every token of the two small levels, the border rows / columns of the two large ones and the tokens around item
    1's padding boundary (row 150 / 232 and column 120 / 200 of each level)"""
    keep, start = [], 0
    for (H, W) in SHAPES:
        if H * W <= 56:
            sel = [(r, c) for r in range(H) for c in range(W)]
        else:
            br, bc = int(np.ceil(MASK_HW[0] * H / IMAGE_HW[0])), int(np.ceil(MASK_HW[1] * W / IMAGE_HW[1]))
            rr = sorted({0, H - 1, br - 1, br, H // 3})
            cc = sorted({0, W - 1, bc - 1, bc, W // 3, 1, bc - 2, bc + 1})
            sel = [(r, c) for r in rr for c in cc]
        keep += [start + r * W + c for r, c in sel]
        start += H * W
    return np.array(sorted(set(keep)))


def inputs():
    """the keyword arguments of ``GroundingDinoEncoder.forward`` as torch tensors (fp32 / bool / long, CPU)"""
    import torch
    from transformers.models.grounding_dino.modeling_grounding_dino import generate_masks_with_special_tokens_and_transfer_map
    rs = np.random.RandomState(SEED + 1)
    Nv = sum(h * w for h, w in SHAPES)
    f16 = lambda a: torch.from_numpy(a.astype(np.float16).astype(np.float32))                       # noqa: E731
    vision = f16(rs.standard_normal((BATCH, Nv, D_MODEL)))
    pos = f16(0.5 * rs.standard_normal((BATCH, Nv, D_MODEL)))
    text = f16(rs.standard_normal((BATCH, TEXT_LEN, D_MODEL)))
    masks = level_masks()
    valid = torch.cat([m.flatten(1) for m in masks], 1)
    ratios = []
    for m in masks:                                                                                 # GroundingDinoModel.get_valid_ratio
        _, H, W = m.shape
        vh, vw = m[:, :, 0].sum(1).float() / H, m[:, 0, :].sum(1).float() / W
        ratios.append(torch.stack([vw, vh], -1))
    ids = torch.tensor(INPUT_IDS)
    allowed, position_ids = generate_masks_with_special_tokens_and_transfer_map(ids)
    spatial = torch.tensor(SHAPES, dtype=torch.long)
    return dict(vision_features=vision, vision_attention_mask=~valid, vision_position_embedding=pos, spatial_shapes=spatial,
                spatial_shapes_list=list(SHAPES), level_start_index=torch.cat((spatial.new_zeros((1,)), spatial.prod(1).cumsum(0)[:-1])),
                valid_ratios=torch.stack(ratios, 1).float(), text_features=text, text_attention_mask=ids == 0, text_position_embedding=None,
                text_self_attention_masks=~allowed, text_position_ids=position_ids)


def load_encoder():
    import torch
    enc = hf_encoder()
    w = make_weights(shapes={"encoder." + k: tuple(v.shape) for k, v in enc.state_dict().items()})
    enc.load_state_dict({k[len("encoder."):]: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    return enc, w


def run(enc, kw, round_dtype=None):
    """{quantity: (vision [B, Nv, d], text [B, Lt, d])}.  ``round_dtype``: the rounded emulation — weights, inputs and every Linear / LayerNorm output
    are rounded to that dtype (the arithmetic stays fp32)."""
    import copy

    import torch
    rnd = (lambda x: x.to(round_dtype).float()) if round_dtype is not None else (lambda x: x)
    hooks = []
    if round_dtype is not None:
        enc = copy.deepcopy(enc)
        with torch.no_grad():
            for p in enc.parameters():
                p.copy_(rnd(p))
        for m in enc.modules():
            if isinstance(m, (torch.nn.Linear, torch.nn.LayerNorm)):
                hooks.append(m.register_forward_hook(lambda _m, _i, o: rnd(o)))
        kw = {k: rnd(v) if isinstance(v, torch.Tensor) and v.dtype == torch.float32 and k != "valid_ratios" else v for k, v in kw.items()}
    got = {}
    hooks.append(enc.layers[0].fusion_layer.register_forward_hook(lambda _m, _i, o: got.__setitem__("fusion0", (o[0][0].detach(), o[1][0].detach()))))
    with torch.no_grad():
        out = enc(**kw, output_hidden_states=True, return_dict=True)
    for h in hooks:
        h.remove()
    got["layer0"] = (out.vision_hidden_states[1], out.text_hidden_states[1])
    got["layer1"] = (out.last_hidden_state_vision, out.last_hidden_state_text)
    return got


def _err(a, b):
    d = (a.double() - b.double())
    return [float(d.norm() / b.double().norm()), float(d.abs().max() / b.double().abs().max())]


def make(path=PATH):
    import torch
    enc, w = load_encoder()
    kw = inputs()
    ref = run(enc, kw)
    r = rows()
    out = dict(rows=r, weight_checksums=weight_checksums(w))
    for q in QUANTITIES:
        out[q + "_vision"] = ref[q][0][:, r].numpy()
        out[q + "_text"] = ref[q][1].numpy()
    for name, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
        emu = run(enc, kw, dt)
        for q in QUANTITIES:
            out[f"emu_{name}_{q}_vision"] = np.array(_err(emu[q][0][:, r], ref[q][0][:, r]))
            out[f"emu_{name}_{q}_text"] = np.array(_err(emu[q][1], ref[q][1]))
            print(name, q, "vision", out[f"emu_{name}_{q}_vision"], "text", out[f"emu_{name}_{q}_text"])
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(r), "vision tokens per item")


if __name__ == "__main__":
    import sys
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    make()
