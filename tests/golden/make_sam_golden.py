"""Regenerate tests/golden/sam_vision_d80.npz and sam_vision_d64.npz from ``transformers.SamVisionEncoder`` (eager attention, fp32, CPU).

Two tiny encoders at image 1024 / patch 16 / window 14 — hidden 160 (2 heads of 80) and hidden 128 (2 heads of 64) — with 2 layers
(layer 0 windowed, layer 1 global), mlp_dim = 2 * hidden, 32 output channels.

The weights are NOT stored: at hidden 160 they are 1.2 M values (pos_embed alone 0.65 M), 2.4 MB as float16, and a committed file stays
under 1 MiB.  ``make_weights`` draws them from numpy's legacy ``RandomState`` (a frozen stream) — parameter = base + s * randn, base 1 for
LayerNorm weights and 0 otherwise, s = 0.25 for the rel_pos tables (a bias of about one score unit) and 0.05 for everything else, rounded to
fp16-representable values so that both storage dtypes of the test start from numbers they hold exactly where possible.  The test calls the
same function; the file keeps (sum, sum of squares) per parameter in float64, so a drifted generator fails loudly, not as a tolerance miss.
The input is the closed-form image

    x[c, i, j] = ((131 i + 71 j + 53 c) mod 251) / 125 - 1

Stored, float32, for the grid rows ``ROWS`` (all 64 columns each: the first and last row, both sides of the window seams at 14, 28, 42, 56,
and row 63, whose last token sits in the corner window: 64 real and 132 padded positions): the hidden state after layer 0 (windowed, padding included) and
after layer 1 (global), [len(ROWS), 64, hidden], and the neck output at the same pixels, [32, len(ROWS), 64].

    python tests/golden/make_sam_golden.py
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROWS = (0, 13, 14, 27, 28, 41, 55, 56, 63)
VARIANTS = {"d80": dict(hidden=160, heads=2, seed=80), "d64": dict(hidden=128, heads=2, seed=64)}


def param_shapes(hidden, out_ch=32, layers=2, global_layers=(1,)):
    """{transformers parameter name: shape} of the tiny SamVisionEncoder."""
    d = hidden // 2
    sh = {"pos_embed": (1, 64, 64, hidden), "patch_embed.projection.weight": (hidden, 3, 16, 16), "patch_embed.projection.bias": (hidden,)}
    for i in range(layers):
        s = 64 if i in global_layers else 14
        p = f"layers.{i}."
        sh.update({p + "layer_norm1.weight": (hidden,), p + "layer_norm1.bias": (hidden,), p + "attn.qkv.weight": (3 * hidden, hidden),
                   p + "attn.qkv.bias": (3 * hidden,), p + "attn.proj.weight": (hidden, hidden), p + "attn.proj.bias": (hidden,),
                   p + "attn.rel_pos_h": (2 * s - 1, d), p + "attn.rel_pos_w": (2 * s - 1, d),
                   p + "layer_norm2.weight": (hidden,), p + "layer_norm2.bias": (hidden,), p + "mlp.lin1.weight": (2 * hidden, hidden),
                   p + "mlp.lin1.bias": (2 * hidden,), p + "mlp.lin2.weight": (hidden, 2 * hidden), p + "mlp.lin2.bias": (hidden,)})
    sh.update({"neck.conv1.weight": (out_ch, hidden, 1, 1), "neck.layer_norm1.weight": (out_ch,), "neck.layer_norm1.bias": (out_ch,),
               "neck.conv2.weight": (out_ch, out_ch, 3, 3), "neck.layer_norm2.weight": (out_ch,), "neck.layer_norm2.bias": (out_ch,)})
    return sh


def make_weights(hidden, seed):
    """{name: float32 array of fp16-representable values}, drawn in sorted-name order from RandomState(seed)."""
    rs = np.random.RandomState(seed)
    out = {}
    for name, shape in sorted(param_shapes(hidden).items()):
        base = 1.0 if "layer_norm" in name and name.endswith(".weight") else 0.0
        s = 0.25 if "rel_pos" in name else 0.05
        out[name] = (base + s * rs.standard_normal(shape)).astype(np.float16).astype(np.float32)
    return out


def golden_image():
    i = np.arange(1024, dtype=np.int64)[None, :, None]
    j = np.arange(1024, dtype=np.int64)[None, None, :]
    c = np.arange(3, dtype=np.int64)[:, None, None]
    return (((131 * i + 71 * j + 53 * c) % 251).astype(np.float32) / np.float32(125.0) - np.float32(1.0))[None]


def weight_checksums(w):
    return np.array([[v.astype(np.float64).sum(), (v.astype(np.float64) ** 2).sum()] for _, v in sorted(w.items())])


def make(hidden, heads, seed, path):
    import torch
    from transformers import SamVisionConfig
    from transformers.models.sam.modeling_sam import SamVisionEncoder
    cfg = SamVisionConfig(hidden_size=hidden, num_hidden_layers=2, num_attention_heads=heads, mlp_dim=2 * hidden, output_channels=32,
                          image_size=1024, patch_size=16, window_size=14, global_attn_indexes=[1], attn_implementation="eager")
    m = SamVisionEncoder(cfg).eval().float()
    w = make_weights(hidden, seed)
    sd = m.state_dict()
    assert set(sd) == set(w) and all(tuple(sd[k].shape) == w[k].shape for k in w), "param_shapes() is out of step with transformers"
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    hs = []
    hooks = [layer.register_forward_hook(lambda _m, _i, o: hs.append((o[0] if isinstance(o, tuple) else o).detach().clone())) for layer in m.layers]
    with torch.no_grad():
        out = m(pixel_values=torch.from_numpy(golden_image())).last_hidden_state
    for h in hooks:
        h.remove()
    assert len(hs) == 2 and hs[0].shape == (1, 64, 64, hidden) and out.shape == (1, 32, 64, 64)
    rows = list(ROWS)
    np.savez_compressed(path, rows=np.array(rows), hidden0=hs[0][0, rows].numpy(), hidden1=hs[1][0, rows].numpy(), neck=out[0][:, rows].numpy(),
                        weight_checksums=weight_checksums(w))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    import torch
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    for tag, v in VARIANTS.items():
        make(v["hidden"], v["heads"], v["seed"], os.path.join(HERE, f"sam_vision_{tag}.npz"))
