"""Host side of the row-chain kernels (csrc/tg_rowchain.hip): weight preprocessing for ``tg_rc_xattn`` — norm2 + attn2 + residual of a
first-level ``BasicTransformerBlock`` (models/attention.py:206-224; ``IPAttnProcessor`` ip_adapter/attention_processor.py:445-529) in one
launch for SD-1.5's geometry (320 channels = 8 heads x 40).  Load-time plumbing only: permutations of ``to_q`` rows / ``to_out`` columns
so that the kernel's register-resident q / O pieces line up with its MFMA operands, the LayerNorm fold of ``pack_ln_linear``, and the
softmax scale (x log2 e: the kernel uses exp2) folded into ``to_q``."""
import math
import os

import torch

from . import ops
from .weights_pack import rc_pack, rc_pack_tiles

# TG_RC: 0 = the row-chain kernels are never selected (old-path A/B), 1 = default.  TG_RC_MIN_ROWS: below this many token rows the
# LDS-tiled GEMMs / the three-launch cross-attention stay (a row-chain workgroup is a long serial chain: it needs a full chip of them)
ENABLED = os.environ.get("TG_RC", "1") != "0"
# dev A/B bits: 0 tg_rc_linear swaps (K = 320), 1 tg_rc_xattn, 2 tg_rc_ff, 3 tg_rc_front.  (Bit 4 was round 4's K = 640 kernel, bit 5 chose between
# tg_rc_ff's two kernels until the one-wave kernel was retired: higher bits are ignored, 47 in an old job file means 15.)
MODE = int(os.environ.get("TG_RC_MODE", "15"))
FF_TWO_WAVE = ops._lib.RC_FF_TWO_WAVE          # TG_RC_FF_TWO_WAVE of include/theatergen_hip.h: the stream-format tag in the ``dbg`` word of tg_rc_ff_desc
MIN_ROWS = int(os.environ.get("TG_RC_MIN_ROWS", "8192"))
# rc_linear / rc_front / rc_ff are one long serial chain per workgroup (a lone rc_ff workgroup needs ~95 us): below one full round of 128-token
# workgroups (256 CUs x 128 rows) the LDS-tiled launches are as fast or faster (8192 rows: rc_ff 95 us vs 64 us, rc_front 51 + 16 vs 59 us)
MIN_ROWS_CHAIN = int(os.environ.get("TG_RC_MIN_ROWS_CHAIN", "32768"))
TRACE = os.environ.get("TG_RC_TRACE") == "1"


def trace(*a):
    if TRACE:
        print("[tg_rc]", *a, flush=True)

HEADS, DH, C = 8, 40, 320


def _q_slot_channels():
    """q channel (head * 40 + d) held by slot n' = 64 c + 32 hi + 8 i + j of the kernel's 20 q k-steps (k-step 4 c + i, lane half hi, element j)"""
    out = torch.empty(C, dtype=torch.long)
    for n in range(C):
        c, hi, i, j = n // 64, (n // 32) & 1, (n // 8) & 3, n & 7
        s = 4 * c + i
        m, w5 = s // 5, s % 5
        if w5 == 0:
            head, d = 2 * m, 8 * hi + j
        elif w5 == 1:
            head, d = 2 * m, 16 + 8 * hi + j
        elif w5 == 2:
            head, d = (2 * m, 32 + j) if hi == 0 else (2 * m + 1, j)
        elif w5 == 3:
            head, d = 2 * m + 1, 8 + 8 * hi + j
        else:
            head, d = 2 * m + 1, 24 + 8 * hi + j
        out[n] = head * DH + d
    assert sorted(out.tolist()) == list(range(C))
    return out


def _o_slot_channels():
    """attention-output channel held by slot n' of the kernel's 20 O k-steps (what ``to_out`` contracts over)"""
    out = torch.empty(C, dtype=torch.long)
    for n in range(C):
        c, hi, i, j = n // 64, (n // 32) & 1, (n // 8) & 3, n & 7
        t = 4 * c + i
        m, t5 = t // 5, t % 5
        if t5 in (0, 1):
            head, d = 2 * m, 16 * t5 + 8 * (j >> 2) + 4 * hi + (j & 3)
        elif t5 == 2:
            head, d = (2 * m, 32 + 4 * hi + j) if j < 4 else (2 * m + 1, 32 + 4 * hi + j - 4)
        else:
            head, d = 2 * m + 1, 16 * (t5 - 3) + 8 * (j >> 2) + 4 * hi + (j & 3)
        out[n] = head * DH + d
    assert sorted(out.tolist()) == list(range(C))
    return out


_QS, _OS = None, None



def pack_xattn_q(wq, bq, gamma, beta, scale):
    """``to_q`` [320, 320] (+ bias) behind LayerNorm(gamma, beta), times softmax scale * log2(e) -> rc chunk stream (uint8).
    q' = rstd * (x W'^T - mean u) + v with W' = s W gamma rounded to the storage dtype, u = row sums of the ROUNDED W', v = s (W beta + b)."""
    global _QS
    if _QS is None:
        _QS = _q_slot_channels()
    s = float(scale) * math.log2(math.e)
    w32 = wq.detach().float()
    wp = (w32 * gamma.detach().float()[None, :] * s).to(wq.dtype)
    u = wp.float().sum(dim=1)
    v = w32 @ beta.detach().float()
    if bq is not None:
        v = v + bq.detach().float()
    v = v * s
    perm = _QS.to(wq.device)
    return rc_pack_tiles(wp[perm].contiguous(), v[perm], u[perm])


def pack_xattn_out(wo, bo):
    """``to_out[0]`` [320, 320] + bias -> rc chunk stream with the input columns in the kernel's O-piece order"""
    global _OS
    if _OS is None:
        _OS = _o_slot_channels()
    perm = _OS.to(wo.device)
    w2 = wo.detach()[:, perm].contiguous()
    return rc_pack_tiles(w2, bo.detach().float() if bo is not None else None)


def linear320(x2d, lin_weight, bias, res, owner, name, cached, pair_out=None):
    """``x @ W^T + b (+ res)`` through ``tg_rc_linear`` when the shape pays — K = 320, rows >= MIN_ROWS_CHAIN, N % 64 == 0 —, else None.
    ``cached(owner, name, tensors, build)`` is the caller's packed-weight cache."""
    M, K = x2d.shape
    N = lin_weight.shape[0]
    if not ENABLED or x2d.stride(1) != 1 or lin_weight.shape[1] != K:
        return None
    ts = [lin_weight] + ([bias] if bias is not None else [])
    if K == 320 and (MODE & 1) and N % 64 == 0 and M >= MIN_ROWS_CHAIN:
        trace("linear320 yes", name, M, N)
        wpk = cached(owner, "rc_" + name, ts, lambda: rc_pack(lin_weight.detach(), bias.detach().float() if bias is not None else None))
        return ops.rc_linear(x2d, wpk, N, res=res, pair_out=pair_out)
    trace("linear_rc no", name, M, K, N)
    return None


def xattn_eligible(attn, C, B, N, L, T, dtype):
    inner = attn.to_q.weight.shape[0]
    return (ENABLED and (MODE & 2) and C == 320 and inner == 320 and int(attn.heads) == 8 and L == 77 and T in (0, 4, 16) and N % 128 == 0
            and B * N >= MIN_ROWS and dtype in (torch.bfloat16, torch.float16) and attn.to_out[0].weight.shape[0] == 320)


# ---- tg_rc_ff: norm3 + FeedForward (GEGLU) + residual (+ proj_out + residual) of a first-level block in one launch --------------------
# rc_ff2_kernel: 16 tokens per wave on 16x16x32 MFMAs (A fragment: lane (r = lane & 15, g = lane >> 4) holds row r, k = 8 g + e)
def _ff2_out_row():
    """MFMA row r of output tile t = 2 s + u -> offset of its channel inside the 32-channel group s, per u: accumulator register i of lane group g
    (row 4 g + i) holds channel 32 s + 8 g + 4 u + i — elements 4 u + i of the rows' 16-byte B piece s"""
    r = torch.arange(16)
    return torch.stack([8 * (r >> 2) + 4 * u + (r & 3) for u in range(2)])                            # [u, r]


def pack_ff2(w1, b1, gamma, beta, w2, b2):
    """``GEGLU.proj`` [2 * inner, 320] (+ bias) behind LayerNorm(gamma, beta) and ``net.2`` [320, inner] (+ bias) -> the streams of ``tg_rc_ff``
    (``rc_ff2_kernel``; reference models/attention.py:226-236, 328-338; inner = 1280): 41 KiB + 20 KiB per 32-channel hidden slice j, 3 KiB pad.
    W' = W * gamma rounded once to the storage dtype, bias + W beta folded into the page; the kernel normalises the rows itself ((x - mean) * rstd
    rounded to the storage dtype: what ``norm3`` hands to ``ff``):
      * w1 stream: 20 VALUE fragments k = 2 s + u, 20 GATE fragments, lane (r, g), element e = W'[32 j + 16 u + r (+ inner), 32 s + 8 g + e]; then the
        1-KiB page: fp32 bias_a[32], bias_g[32] in hidden-channel order;
      * w2 stream: 20 fragments, tile t = 2 s + u: lane (r, g), element e = net.2[32 s + 8 (r >> 2) + 4 u + (r & 3), 32 j + 16 (e >> 2) + 4 g + (e & 3)]
        (the hidden piece a lane group holds after GEGLU: registers i of the two 16-channel value tiles);
      * b2: fp32 [320]."""
    inner = w2.shape[1]
    assert w1.shape == (2 * inner, C) and w2.shape == (C, inner) and inner % 32 == 0
    dev, dt = w1.device, w1.dtype
    ar = lambda k: torch.arange(k, device=dev)
    w1f = w1.detach().float()
    w1g = (w1f * gamma.detach().float()[None, :]).to(dt)                                 # rounded once, like pack_ln_linear
    v1 = w1f @ beta.detach().float() + (b1.detach().float() if b1 is not None else 0.0)  # [2 * inner]
    ns = inner // 32
    # frag[slice, which, s, u, g, r, e]
    rows = (inner * ar(2)[None, :, None, None, None, None, None] + 32 * ar(ns)[:, None, None, None, None, None, None]
            + 16 * ar(2)[None, None, None, :, None, None, None] + ar(16)[None, None, None, None, None, :, None])
    cols = 32 * ar(10)[None, None, :, None, None, None, None] + 8 * ar(4)[None, None, None, None, :, None, None] + ar(8)
    fb = w1g[rows, cols].contiguous().reshape(ns, -1).view(torch.uint8)                  # [slice, 40 KiB]
    page = torch.zeros(ns, 256, dtype=torch.float32, device=dev)
    page[:, :32] = v1[:inner].reshape(ns, 32)
    page[:, 32:64] = v1[inner:].reshape(ns, 32)
    s1 = torch.cat([fb, page.view(torch.uint8)], dim=1).reshape(-1)
    s1 = torch.cat([s1, torch.zeros(3 * 1024, dtype=torch.uint8, device=dev)])
    orow = _ff2_out_row().to(dev)                                                        # [u, r]
    out_rows = (32 * ar(10)[:, None, None] + orow[None]).reshape(20, 16)                 # [t = 2 s + u, r]
    e = ar(8)
    kcol = (32 * ar(ns)[:, None, None] + 4 * ar(4)[None, :, None] + (16 * (e >> 2) + (e & 3))[None, None, :])   # [slice, g, e]
    f2 = w2.detach()[out_rows[None, :, None, :, None], kcol[:, None, :, None, :]].contiguous()                  # [slice, t, g, r, e]
    s2 = f2.reshape(-1).view(torch.uint8)
    bb2 = (b2.detach().float() if b2 is not None else torch.zeros(C, device=dev)).contiguous()
    return s1.contiguous(), s2.contiguous(), bb2


def pack_po2(w, b=None):
    """``proj_out`` [320, 320] (+ bias) -> the tail stream of ``rc_ff2_kernel``: per 32-channel output group st 20 fragments k = 2 s + u (lane (r, g),
    element e = W[32 st + 8 (r >> 2) + 4 u + (r & 3), 32 s + 8 g + e]) and a 1-KiB page with the fp32 bias in tile order (index 16 u + r); 3 KiB of
    zero padding behind the last group (every 21-KiB group is fetched as a 24-KiB stage)."""
    assert w.shape == (C, C)
    dev = w.device
    ar = lambda k: torch.arange(k, device=dev)
    orow = _ff2_out_row().to(dev)                                                        # [u, r]
    # frag[st, s, u, g, r, e]
    rows = 32 * ar(10)[:, None, None, None, None, None] + orow[None, None, :, None, :, None]
    cols = 32 * ar(10)[None, :, None, None, None, None] + 8 * ar(4)[None, None, None, :, None, None] + ar(8)
    fb = w.detach()[rows, cols].contiguous().reshape(10, -1).view(torch.uint8)           # [st, 20 KiB]
    page = torch.zeros(10, 256, dtype=torch.float32, device=dev)
    if b is not None:
        page[:, :32] = b.detach().float()[(32 * ar(10)[:, None, None] + orow[None]).reshape(10, 32)]
    out = torch.cat([fb, page.view(torch.uint8)], dim=1).contiguous().reshape(-1)
    return torch.cat([out, torch.zeros(3 * 1024, dtype=torch.uint8, device=dev)])
