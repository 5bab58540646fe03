"""fp64 restatement of the C-ABI contract of ``tg_attention_swin`` (include/theatergen_hip.h), written from the contract and not from the kernel.

Tokens are in image order; everything is explicit loops over windows, so each clause of the contract is one line that can be switched off
(``drop=``) to show that a test case exercises it.
"""
import numpy as np

WINDOW = 7

# the kernel cases of the issue: (H, W, shift, batch, heads)
CASES = [(7, 7, 0, 1, 1), (8, 7, 0, 2, 3), (9, 10, 3, 1, 2), (15, 13, 3, 2, 1), (29, 25, 3, 2, 3)]


def region(r, c, Hp, Wp, shift):
    """the contract's region of rolled position (r, c)"""
    return 3 * (int(r >= Hp - WINDOW) + int(r >= Hp - shift)) + (int(c >= Wp - WINDOW) + int(c >= Wp - shift))


def swin_window_reference(q, k, v, pad_q, pad_k, pad_v, table, H, W, shift, scale, drop=()):
    """q, k, v [B, H*W, heads*32]; pad_* [heads*32]; table [169, heads] -> out [B, H*W, heads*32], all float64.
    ``drop``: any of "bias", "mask", "padkeys" (padded tokens leave the softmax), "roll" (sources are read and written unrolled): ablations for the
    test that every clause matters — never part of the contract."""
    q, k, v = (np.asarray(t, np.float64) for t in (q, k, v))
    pad_q, pad_k, pad_v, table = (np.asarray(t, np.float64) for t in (pad_q, pad_k, pad_v, table))
    B, n, C = q.shape
    heads = C // 32
    assert n == H * W and C == heads * 32 and table.shape == (169, heads)
    Hp, Wp = -(-H // WINDOW) * WINDOW, -(-W // WINDOW) * WINDOW
    roll = 0 if "roll" in drop else shift
    out = np.full((B, n, C), np.nan)
    wr, wc = np.divmod(np.arange(49), WINDOW)
    bias_idx = (wr[:, None] - wr[None, :] + 6) * 13 + (wc[:, None] - wc[None, :] + 6)
    for wy in range(Hp // WINDOW):
        for wx in range(Wp // WINDOW):
            r, c = wy * WINDOW + wr, wx * WINDOW + wc                     # rolled coordinates of the 49 tokens
            sr, sc = (r + roll) % Hp, (c + roll) % Wp                     # their sources
            real = (sr < H) & (sc < W)
            src = np.where(real, sr * W + sc, 0)
            reg = np.array([region(a, b, Hp, Wp, shift) for a, b in zip(r, c)])
            m = np.where(reg[:, None] != reg[None, :], -100.0, 0.0) if shift > 0 and "mask" not in drop else np.zeros((49, 49))
            if "padkeys" in drop:
                m = m + np.where(real[None, :], 0.0, -np.inf)
            for b in range(B):
                qw = np.where(real[:, None], q[b, src], pad_q[None, :])
                kw = np.where(real[:, None], k[b, src], pad_k[None, :])
                vw = np.where(real[:, None], v[b, src], pad_v[None, :])
                for h in range(heads):
                    sl = slice(h * 32, h * 32 + 32)
                    s = scale * qw[:, sl] @ kw[:, sl].T + m
                    if "bias" not in drop:
                        s = s + table[bias_idx, h]
                    s = s - s.max(1, keepdims=True)
                    p = np.exp(s)
                    o = (p / p.sum(1, keepdims=True)) @ vw[:, sl]
                    out[b, src[real], sl] = o[real]
    assert not np.isnan(out).any()
    return out


def make_case(H, W, shift, batch, heads, seed, round_to=None):
    """Inputs of one kernel case as float64 arrays (q | k | v are columns of one [B, H*W, 3C] array).  Scales: q.k * scale has standard deviation
    ~1.4, the table ~1: bias, shift mask, padded keys and the roll each move the result well beyond the op tolerance (checked by the CPU tests).
    ``round_to``: a function that rounds an fp32 array to the storage dtype's values (the GPU tests pass the stored operands on)."""
    rng = np.random.RandomState(seed)
    C = heads * 32
    qkv = rng.standard_normal((batch, H * W, 3 * C)) * np.concatenate([np.full(C, 1.5), np.full(C, 1.5), np.full(C, 1.0)])
    pads = rng.standard_normal((3, C)) * np.array([[1.5], [1.5], [1.0]])
    table = rng.standard_normal((169, heads))
    if round_to is not None:
        qkv, pads, table = round_to(qkv), round_to(pads), round_to(table)
    return qkv, pads, table


def run_case(qkv, pads, table, H, W, shift, drop=()):
    C = qkv.shape[-1] // 3
    return swin_window_reference(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], pads[0], pads[1], pads[2], table, H, W, shift, 32 ** -0.5, drop)
