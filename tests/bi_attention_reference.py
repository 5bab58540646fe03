"""fp64 restatement of masked wide-head attention (``ops.attention_wide(key_mask=)``, include/theatergen_hip.h: tg_attention_wide_kmask) and of the
bidirectional attention of GroundingDINO's fusion layer built from it, from the projected operands on."""
import numpy as np


def masked_attention_reference(q, k, v, scale, key_mask=None):
    """q [B, n_q, heads*d], k / v [B, len, heads*d], key_mask [B, len] (1 = masked) -> softmax(scale q k^T + (-inf where masked)) v, float64
    [B, n_q, heads*d]; ``heads`` is taken from ``d`` = 256.  A row with every key masked is outside the contract (NaN here)."""
    return _attn(q, k, v, scale, key_mask, 256)


def _attn(q, k, v, scale, key_mask, d):
    q, k, v = (np.asarray(t, np.float64) for t in (q, k, v))
    B, n_q, C = q.shape
    heads = C // d
    out = np.empty((B, n_q, C))
    for b in range(B):
        for h in range(heads):
            sl = slice(h * d, (h + 1) * d)
            s = scale * q[b, :, sl] @ k[b, :, sl].T
            if key_mask is not None:
                s = np.where(np.asarray(key_mask[b]).astype(bool)[None, :], -np.inf, s)
            with np.errstate(invalid="ignore"):
                s = s - s.max(1, keepdims=True)
                p = np.exp(s)
                out[b, :, sl] = (p / p.sum(1, keepdims=True)) @ v[b, :, sl]
    return out


def bi_attention_reference(q_vision, k_text, v_vision, v_text, head_dim, vision_mask=None, text_mask=None):
    """``GroundingDinoBiMultiHeadAttention`` between its input and output projections: q_vision / v_vision [B, Nv, E], k_text / v_text [B, Lt, E], masks
    [B, Nv] / [B, Lt] with 1 = padding -> (vision output [B, Nv, E], text output [B, Lt, E]).  The text side's scores are the transpose of the vision side's.
    The module's max subtraction and clamp to +-50 000 are softmax-invariant while a row's spread stays below 50 000 and are not restated."""
    scale = float(head_dim) ** -0.5
    return (_attn(q_vision, k_text, v_text, scale, text_mask, head_dim), _attn(k_text, q_vision, v_vision, scale, vision_mask, head_dim))
