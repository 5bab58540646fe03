"""Regenerate tests/golden/sam_decoder_g16.npz and sam_decoder_g64.npz from ``transformers.SamModel`` (eager attention, CPU, **float64**): prompt encoder +
mask decoder on given image embeddings and box prompts.

The decoder has 4.06 M parameters, so the weights are NOT stored: ``make_weights`` draws them from numpy's legacy ``RandomState`` (a frozen stream) in
sorted-name order — parameter = base + s * randn, base 1 for LayerNorm weights, s = 32 for the positional matrix (the scale at which coordinates rounded to
half precision move the Fourier phase by a radian), 0.1 for the token / point / no-mask embeddings, 0.04 for everything else (larger embeddings make
the float64 model itself ill-conditioned: at 0.5 even the rounding floor below is a 60 % error) — rounded to fp16-representable
values (the positional matrix stays fp32).  The test calls the same function; the file keeps (sum, sum of squares) per parameter in float64, so a drifted
generator fails loudly, not as a tolerance miss.  Image embeddings: standard normal from the same stream, fp16-representable.

Cases
  g16  image_embedding_size 16 (a 256-pixel padded image), B = 2 images x nb = 2 boxes; one box lies partly outside the image.  7 tokens per prompt.
  g64  image_embedding_size 64 (1024 pixels), B = 1, nb = 1.

Stored per case: ``image_embeddings``' seed inputs are regenerated, ``boxes`` [B, nb, 4] (pixels of the padded image, what the model receives),
``pred_masks`` [B, nb, 3, 4g, 4g] and ``iou_scores`` [B, nb, 3] of the float64 run as float32, ``weight_checksums``, and per storage dtype two error
rows [rel-L2 of pred_masks, rel-L2 of iou_scores, share of pred_masks signs that differ], each against the float64 run:
  ``floor_<dtype>``     the same model with weights and embeddings rounded to the dtype, a forward hook rounding the output of every Linear / LayerNorm /
                        ConvTranspose2d / GELU / ReLU / positional embedding to the dtype, fp32 arithmetic, the positional matrix kept fp32: what a kernel
                        route with storage in the dtype and fp32 accumulation can reach;
  ``autocast_<dtype>``  ``torch.autocast('cpu', dtype)`` around the fp32 model: the reference's route (models/sam.py:39).

    python tests/golden/make_sam_decoder_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
CASES = {
    "g16": dict(g=16, seed=1601, boxes=[[[30.0, 40.0, 180.0, 200.0], [-20.5, 100.25, 90.0, 300.0]], [[5.0, 5.0, 250.0, 120.0], [100.0, 60.0, 140.0, 90.0]]]),
    "g64": dict(g=64, seed=6401, boxes=[[[211.0, 150.5, 800.0, 901.25]]]),
}
DTYPES = ("bfloat16", "float16")


def param_shapes(g):
    """{transformers parameter name: shape} of the prompt encoder, mask decoder and shared positional matrix (this package's module tree has the names)."""
    from theatergen_amd.sam_decoder import SamModel, sam_decoder_config
    m = SamModel(None, sam_decoder_config(g), with_vision=False)
    return {k: tuple(v.shape) for k, v in m.state_dict().items() if k != "prompt_encoder.shared_embedding.positional_embedding"}


def make_weights(g, seed):
    """{name: float32 array}, drawn in sorted-name order from RandomState(seed)"""
    rs = np.random.RandomState(seed)
    out = {}
    for name, shape in sorted(param_shapes(g).items()):
        if name.endswith("positional_embedding"):
            out[name] = (32.0 * rs.standard_normal(shape)).astype(np.float32)
            continue
        base = 1.0 if "layer_norm" in name and name.endswith(".weight") else 0.0
        s = 0.1 if ("token" in name or ("_embed" in name and not name.startswith("prompt_encoder.mask_embed."))) else 0.04
        out[name] = (base + s * rs.standard_normal(shape)).astype(np.float16).astype(np.float32)
    return out


def make_embeddings(g, seed, batch):
    return np.random.RandomState(seed + 7).standard_normal((batch, 256, g, g)).astype(np.float16).astype(np.float32)


def weight_checksums(w):
    return np.array([[v.astype(np.float64).sum(), (v.astype(np.float64) ** 2).sum()] for _, v in sorted(w.items())])


def errors(pm, iou, pm64, iou64):
    pm, iou = np.asarray(pm, np.float64), np.asarray(iou, np.float64)
    return np.array([np.linalg.norm(pm - pm64) / np.linalg.norm(pm64), np.linalg.norm(iou - iou64) / np.linalg.norm(iou64),
                     np.mean((pm > 0) != (pm64 > 0))])


def _hf_model(g, w):
    import torch
    from transformers import SamConfig, SamModel
    cfg = SamConfig(vision_config=dict(hidden_size=32, num_hidden_layers=1, num_attention_heads=2, mlp_dim=32, image_size=16 * g, patch_size=16,
                                       window_size=0, global_attn_indexes=[0], output_channels=256),
                    prompt_encoder_config=dict(image_size=16 * g, image_embedding_size=g, patch_size=16), attn_implementation="eager")
    m = SamModel(cfg).eval().float()
    sd = m.state_dict()
    mine = {k: v for k, v in sd.items() if not k.startswith("vision_encoder.") and k != "prompt_encoder.shared_embedding.positional_embedding"}
    assert set(mine) == set(w) and all(tuple(mine[k].shape) == w[k].shape for k in w), "param_shapes() is out of step with transformers"
    new = {k: torch.from_numpy(v) for k, v in w.items()}
    new["prompt_encoder.shared_embedding.positional_embedding"] = new["shared_image_embedding.positional_embedding"]
    m.load_state_dict(new, strict=False)
    return m


def _run(m, emb, boxes):
    import torch
    with torch.no_grad():
        o = m(image_embeddings=emb, input_boxes=boxes, multimask_output=True)
    return o.pred_masks.double().numpy(), o.iou_scores.double().numpy()


def make(tag, g, seed, boxes):
    import torch
    import torch.nn as nn
    from transformers.models.sam.modeling_sam import SamPositionalEmbedding
    w = make_weights(g, seed)
    boxes = np.asarray(boxes, np.float64)
    emb = make_embeddings(g, seed, boxes.shape[0])
    pm64, iou64 = _run(_hf_model(g, w).double(), torch.from_numpy(emb).double(), torch.from_numpy(boxes))
    rec = dict(boxes=boxes, pred_masks=pm64.astype(np.float32), iou_scores=iou64.astype(np.float32), weight_checksums=weight_checksums(w))
    for name in DTYPES:
        dt = getattr(torch, name)
        wr = {k: (v if k.endswith("positional_embedding") else torch.from_numpy(v).to(dt).float().numpy()) for k, v in w.items()}
        m = _hf_model(g, wr)
        kinds = (nn.Linear, nn.LayerNorm, nn.ConvTranspose2d, nn.GELU, nn.ReLU, SamPositionalEmbedding)
        hooks = [mod.register_forward_hook(lambda _m, _i, o, dt=dt: o.to(dt).float()) for mod in m.modules() if isinstance(mod, kinds)]
        rec["floor_" + name] = errors(*_run(m, torch.from_numpy(emb).to(dt).float(), torch.from_numpy(boxes).float()), pm64, iou64)
        for h in hooks:
            h.remove()
        m = _hf_model(g, w)
        with torch.autocast("cpu", dtype=dt):
            rec["autocast_" + name] = errors(*_run(m, torch.from_numpy(emb), torch.from_numpy(boxes).float()), pm64, iou64)
        print(tag, name, "floor", rec["floor_" + name], "autocast", rec["autocast_" + name])
    path = os.path.join(HERE, f"sam_decoder_{tag}.npz")
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    import torch
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    for tag, c in CASES.items():
        make(tag, c["g"], c["seed"], c["boxes"])
