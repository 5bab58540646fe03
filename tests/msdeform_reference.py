"""fp64 restatement of the C-ABI contract of ``tg_msdeform_attn`` (include/theatergen_hip.h), written from the contract and not from the kernel.

Each clause of the contract is one line that can be switched off (``drop=``) to show that a test case exercises it.
"""
import numpy as np

D, P = 32, 4

# the kernel cases of the issue: (levels, heads, batch, n_q, R, has a value mask)
CASES = [
    ([(7, 5)], 1, 1, 35, 2, False),
    ([(9, 7), (5, 4), (3, 2), (2, 1)], 3, 2, 91, 2, True),
    ([(8, 7), (4, 4)], 8, 2, 10, 4, False),
    ([(29, 25), (15, 13), (8, 7), (4, 4)], 4, 2, 992, 2, True),
]
IDS = ["1lvl_h1_b1_q35_r2", "4lvl_h3_b2_q91_r2_mask", "2lvl_h8_b2_q10_r4", "4lvl_h4_b2_q992_r2_mask"]


def msdeform_reference(value, shapes, offsets, logits, ref, value_mask=None, drop=(), stats=None):
    """value [B, Nv, heads*32]; offsets [B, Nq, heads, L, 4, 2]; logits [B, Nq, heads, L*4]; ref [B, Nq, L, R]; value_mask [B, Nv] (1 = padding) or
    None -> out [B, Nq, heads*32], float64.
    ``drop``: any of "padding" (a tap outside the map reads the clamped border token), "mask", "softmax" (uniform weights), "shift" (no -0.5),
    "start" (every level starts at token 0): ablations for the test that every clause matters — never part of the contract.
    ``stats``: a dict that receives the fractions of taps outside their map (``outside``) and, of those inside, on a masked token (``masked``)."""
    value, offsets, logits, ref = (np.asarray(t, np.float64) for t in (value, offsets, logits, ref))
    B, Nv, C = value.shape
    heads = C // D
    _, Nq, _, L, _, _ = offsets.shape
    R = ref.shape[-1]
    assert C == heads * D and len(shapes) == L and offsets.shape == (B, Nq, heads, L, P, 2) and logits.shape == (B, Nq, heads, L * P)
    assert sum(h * w for h, w in shapes) == Nv and ref.shape == (B, Nq, L, R) and R in (2, 4)
    if "softmax" in drop:
        wgt = np.full(logits.shape, 1.0 / (L * P))
    else:
        e = np.exp(logits - logits.max(-1, keepdims=True))
        wgt = e / e.sum(-1, keepdims=True)
    wgt = wgt.reshape(B, Nq, heads, L, P)
    shift = 0.0 if "shift" in drop else 0.5
    vh = value.reshape(B, Nv, heads, D)
    out = np.zeros((B, Nq, heads, D))
    n_taps = n_out = n_masked = 0
    start = 0
    bi = np.arange(B)[:, None, None, None]
    hi = np.arange(heads)[None, None, :, None]
    for l, (H, W) in enumerate(shapes):
        off = offsets[:, :, :, l]                                       # [B, Nq, heads, P, 2]
        r = ref[:, :, None, l, None, :]                                 # [B, Nq, 1, 1, R]
        if R == 2:
            x = r[..., 0] * W + off[..., 0] - shift
            y = r[..., 1] * H + off[..., 1] - shift
        else:
            x = (r[..., 0] + off[..., 0] / P * r[..., 2] * 0.5) * W - shift
            y = (r[..., 1] + off[..., 1] / P * r[..., 3] * 0.5) * H - shift
        x0, y0 = np.floor(x), np.floor(y)
        fx, fy = x - x0, y - y0
        base = 0 if "start" in drop else start
        for dy in (0, 1):
            for dx in (0, 1):
                xx, yy = (x0 + dx).astype(np.int64), (y0 + dy).astype(np.int64)
                inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
                tok = base + np.clip(yy, 0, H - 1) * W + np.clip(xx, 0, W - 1)
                ok = np.ones_like(inside) if "padding" in drop else inside.copy()
                n_taps += inside.size
                n_out += int((~inside).sum())
                if value_mask is not None:
                    hit = np.asarray(value_mask)[bi, tok].astype(bool)
                    n_masked += int((hit & inside).sum())
                    if "mask" not in drop:
                        ok &= ~hit
                bw = (fx if dx else 1.0 - fx) * (fy if dy else 1.0 - fy)
                tapw = np.where(ok, wgt[:, :, :, l] * bw, 0.0)          # [B, Nq, heads, P]
                out += (tapw[..., None] * vh[bi, tok, hi]).sum(3)
        start += H * W
    if stats is not None:
        stats["outside"] = n_out / n_taps
        stats["masked"] = n_masked / max(n_taps - n_out, 1)
    return out.reshape(B, Nq, C)


def golden_value_mask(shapes, batch):
    """The padding mask of the encoder golden (tests/golden/make_grounding_dino_encoder_golden.py): item 0 unpadded, item 1's 232 x 200 pixel mask cut to
    150 x 120, interpolated to every level by nearest, as ``transformers`` does.  uint8 [batch, Nv], 1 = padding."""
    out = []
    for b in range(batch):
        rows = []
        for (H, W) in shapes:
            m = np.zeros((H, W), np.uint8)
            if b == 1:
                ys = np.floor(np.arange(H) * (232.0 / H)).astype(int)
                xs = np.floor(np.arange(W) * (200.0 / W)).astype(int)
                m = ((ys[:, None] >= 150) | (xs[None, :] >= 120)).astype(np.uint8)
            rows.append(m.reshape(-1))
        out.append(np.concatenate(rows))
    return np.stack(out)


def make_case(case, seed, round_to=None):
    """Inputs of one kernel case as float64 arrays (+ the uint8 mask or None).  Offsets are a few pixels (standard deviation 2.5, so the small levels are
    left often: a tap of a 2 x 1 level is always partly outside), logits O(1.5), reference points the cell centres of a query grid (R = 2) or random boxes
    (R = 4).  ``round_to``: rounds an fp32 array to the storage dtype's values (the GPU tests pass the stored operands on); ``ref`` stays fp32."""
    shapes, heads, B, Nq, R, has_mask = case
    rng = np.random.RandomState(seed)
    L = len(shapes)
    Nv = sum(h * w for h, w in shapes)
    value = rng.standard_normal((B, Nv, heads * D))
    offsets = rng.standard_normal((B, Nq, heads, L, P, 2)) * 2.5
    logits = rng.standard_normal((B, Nq, heads, L * P)) * 1.5
    if R == 2:
        ref = rng.uniform(0.02, 0.98, (B, Nq, 1, 2)) * rng.uniform(0.8, 1.0, (B, 1, L, 2))
    else:
        ref = np.concatenate([rng.uniform(0.1, 0.9, (B, Nq, L, 2)), rng.uniform(0.2, 2.0, (B, Nq, L, 2))], -1)
    ref = ref.astype(np.float32).astype(np.float64)
    mask = None
    if has_mask:
        mask = golden_value_mask(shapes, B) if shapes == CASES[3][0] else (rng.uniform(size=(B, Nv)) < 0.3).astype(np.uint8)
    if round_to is not None:
        value, offsets, logits = round_to(value), round_to(offsets), round_to(logits)
    return value, offsets, logits, ref, mask
