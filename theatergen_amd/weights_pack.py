"""Weight layout conversion (load-time plumbing, host side): diffusers state-dict tensors -> the layouts
the HIP kernels read.  Token-major activations want K-contiguous weights:
  Linear  [N, K]            -> unchanged
  Conv1x1 [N, C, 1, 1]      -> [N, C]
  Conv3x3 [N, C, 3, 3]      -> [N, 9*C] tap-major (ky, kx, c)  (implicit-GEMM K order of tg_gemm mode 1)
  Upsample2D's conv         -> [4, N, 4*C] parity-class-major, folded taps (ty, tx, c)  (tg_conv_up2)
  ConvTranspose2d 3x3 s2    -> the same [4, N, 4*C] with zero weights on the unused taps, or [4*N, 9*C] for a pad-1 conv on the low-resolution grid
  Conv7x7 (lineart)         -> fp32 [C*49, N] / [49, C]
"""
import torch


def pack_conv3x3(w: torch.Tensor) -> torch.Tensor:
    n, c, kh, kw = w.shape
    assert kh == 3 and kw == 3
    return w.permute(0, 2, 3, 1).reshape(n, 9 * c).contiguous()


_UP2_ROWS = (((0,), (1, 2)), ((0, 1), (2,)))      # [parity][folded tap] -> original taps: nearest x2 maps them onto one input row / column


def pack_conv3x3_up2(w: torch.Tensor) -> torch.Tensor:
    """Upsample2D's conv3x3 with the nearest x2 folded in (tg_conv_up2): [N, C, 3, 3] -> [4, N, 4*C] in w's dtype.  Output pixel
    (2i+py, 2j+px) sees only the 2 x 2 input pixels (i+py+ty-1, j+px+tx-1), ty, tx in {0, 1}; class cls = 2*py + px holds, tap-major
    (ty, tx, c), the sums of the original taps that land on each of them.  Summed in fp32 (fp64 stays fp64), rounded once."""
    n, c, kh, kw = w.shape
    assert kh == 3 and kw == 3
    acc = w.detach().to(torch.float64 if w.dtype == torch.float64 else torch.float32)
    out = torch.empty(4, n, 2, 2, c, dtype=acc.dtype, device=w.device)
    for py in range(2):
        for px in range(2):
            for ty in range(2):
                for tx in range(2):
                    out[2 * py + px, :, ty, tx] = sum(acc[:, :, ky, kx] for ky in _UP2_ROWS[py][ty] for kx in _UP2_ROWS[px][tx])
    return out.reshape(4, n, 4 * c).to(w.dtype).contiguous()


_CONVT_TAPS = ((None, 1), (2, 0))                 # [parity][2x2 tap] -> tap of the transposed conv's 3x3 kernel (None: the tap is not used)


def pack_convT3x3_s2_up2(w: torch.Tensor) -> torch.Tensor:
    """``ConvTranspose2d(C, N, 3, stride=2, padding=1, output_padding=1)`` weight [C, N, 3, 3] -> tg_conv_up2's layout [4, N, 4*C] in w's dtype.
    Output row 2i takes tap ky = 1 at input row i; row 2i + 1 takes ky = 2 at row i and ky = 0 at row i + 1 (columns alike).  In tg_conv_up2's 2x2-tap
    classes, (ty, tx) of output pixel (2i + py, 2j + px) reads input pixel (i + py + ty - 1, j + px + tx - 1): the taps a class does not use are zero
    weights, and the kernel's zero padding past the last row / column is ``output_padding=1``'s.  A permutation with zeros: nothing is summed or rounded."""
    c, n, kh, kw = w.shape
    assert kh == 3 and kw == 3
    out = torch.zeros(4, n, 2, 2, c, dtype=w.dtype, device=w.device)
    wd = w.detach()
    for py in range(2):
        for px in range(2):
            for ty in range(2):
                for tx in range(2):
                    ky, kx = _CONVT_TAPS[py][ty], _CONVT_TAPS[px][tx]
                    if ky is not None and kx is not None:
                        out[2 * py + px, :, ty, tx] = wd[:, :, ky, kx].transpose(0, 1)
    return out.reshape(4, n, 4 * c).contiguous()


def pack_convT3x3_s2_conv3x3(w: torch.Tensor) -> torch.Tensor:
    """The same transposed conv for geometries tg_conv_up2 does not take: [C, N, 3, 3] -> [4*N, 9*C], the tap-major weight of a stride-1 pad-1 3x3 conv
    (tg_gemm mode 1) on the LOW-resolution grid with 4 N output channels; channel (2 py + px) N + n of low-resolution pixel (i, j) is output pixel
    (2i + py, 2j + px), channel n (layout 2 of tg_lineart_instnorm).  Conv tap (dy, dx) in {0, 1, 2} reads input pixel (i + dy - 1, j + dx - 1): row i is
    dy = 1, row i + 1 is dy = 2 and dy = 0 stays zero; the conv's zero padding past the last row / column is ``output_padding=1``'s."""
    c, n, kh, kw = w.shape
    assert kh == 3 and kw == 3
    out = torch.zeros(4, n, 3, 3, c, dtype=w.dtype, device=w.device)
    wd = w.detach()
    taps = (((1, 1),), ((1, 2), (2, 0)))           # [parity] -> (conv tap, transposed-conv tap) pairs
    for py in range(2):
        for px in range(2):
            for dy, ky in taps[py]:
                for dx, kx in taps[px]:
                    out[2 * py + px, :, dy, dx] = wd[:, :, ky, kx].transpose(0, 1)
    return out.reshape(4 * n, 9 * c).contiguous()


def pack_conv7x7_fp32(w: torch.Tensor) -> torch.Tensor:
    """Conv2d weight [N, C, 7, 7] -> fp32 [C * 49, N], row (c * 7 + ky) * 7 + kx (tg_lineart_conv7_in / _out read wave-uniform rows of output channels).
    The VALUES stay the stored ones (an exact widening)."""
    n, c, kh, kw = w.shape
    assert kh == 7 and kw == 7
    return w.detach().float().permute(1, 2, 3, 0).reshape(c * 49, n).contiguous()


def pack_conv7x7_to1_fp32(w: torch.Tensor) -> torch.Tensor:
    """Conv2d weight [1, C, 7, 7] -> fp32 [49, C], row ky * 7 + kx (tg_lineart_conv7_out: a thread's channels are contiguous)"""
    n, c, kh, kw = w.shape
    assert n == 1 and kh == 7 and kw == 7
    return w.detach().float()[0].permute(1, 2, 0).reshape(49, c).contiguous()


def pack_conv1x1(w: torch.Tensor) -> torch.Tensor:
    return w.reshape(w.shape[0], w.shape[1]).contiguous()


def pack_geglu(w: torch.Tensor, b: torch.Tensor = None):
    """GEGLU.proj weight [2*inner, C] = [a ; gate] (reference models/attention.py:328, 337) -> rows interleaved in groups
    of 32: [a(0:32) ; gate(0:32) ; a(32:64) ; gate(32:64) ; ...] so that one wave of tg_gemm holds a[c] and gate[c] of
    the same channel in the same lane (fused GEGLU epilogue).  ``inner`` must be a multiple of 32."""
    two_inner = w.shape[0]
    inner = two_inner // 2
    assert inner % 32 == 0
    a, g = w[:inner], w[inner:]
    wp = torch.stack([a.reshape(inner // 32, 32, -1), g.reshape(inner // 32, 32, -1)], dim=1).reshape(two_inner, -1).contiguous()
    bp = None
    if b is not None:
        bp = torch.stack([b[:inner].reshape(inner // 32, 32), b[inner:].reshape(inner // 32, 32)], dim=1).reshape(two_inner).contiguous()
    return wp, bp


def pack_ln_linear(w: torch.Tensor, bias, gamma: torch.Tensor, beta: torch.Tensor, scale: float = 1.0):
    """LayerNorm folded into the Linear that consumes it (tg_gemm ``ln_u`` / ``ln_v``):
        Linear(LayerNorm(x)) = rstd * (x W'^T - mean * u) + v,   W' = W * gamma  (storage dtype),
        u[n] = sum_k W'[n, k]  summed from the ROUNDED W' (so that x W'^T - mean * u = (x - mean) W'^T exactly),
        v[n] = sum_k beta[k] W[n, k] + bias[n]                     (fp32).
    One-off weight preprocessing at load / first use, like the conv repacks above; returns (W', u fp32, v fp32).
    ``scale`` multiplies W and the bias in fp32 BEFORE the rounding (tg_xq_attn: softmax scale * log2(e) folded into to_q)."""
    w32 = w.detach().float() * float(scale)
    wp = (w32 * gamma.detach().float()[None, :]).to(w.dtype).contiguous()
    u = wp.float().sum(dim=1).contiguous()
    v = w32 @ beta.detach().float()
    if bias is not None:
        v = v + bias.detach().float() * float(scale)
    return wp, u, v.contiguous()


def _rc_maps(K: int):
    """index maps of the row-chain kernels (csrc/tg_rowchain.hip): output-row permutation of a 64-row chunk and the k order"""
    r = torch.arange(32)
    pi = torch.stack([32 * ((r >> 2) & 1) + 16 * u + 4 * (r >> 3) + (r & 3) for u in range(2)])      # [u, r] -> row within the chunk
    s = torch.arange(K // 16)[:, None, None]
    hi = torch.arange(2)[None, :, None]
    j = torch.arange(8)[None, None, :]
    kap = 64 * (s >> 2) + 32 * hi + 8 * (s & 3) + j                                                   # [s, hi, j] -> input channel
    return pi, kap


def rc_pack(w: torch.Tensor, v: torch.Tensor = None, u: torch.Tensor = None) -> torch.Tensor:
    """Linear weight [N, K] (N % 64 == 0, K % 64 == 0) -> the row-chain kernels' chunk stream (uint8): per 64-row chunk c
      * 2 MFMA tiles x K / 16 k-steps x (64 lanes x 8 elements) of weight fragments: block (u, s), lane (hi, r), element j =
        W[64 c + pi(u, r), kappa(s, hi, j)]  (straight LDS-DMA, linear conflict-free fragment reads), then
      * one 1-KiB vector page: fp32 v[64 c : 64 c + 64] (bias, or W beta + bias under the LayerNorm fold), fp32 u[64 c : 64 c + 64]
        (fold: row sums of the ROUNDED W gamma), zero padding."""
    n, k = w.shape
    assert n % 64 == 0 and k % 64 == 0, (n, k)
    pi, kap = _rc_maps(k)
    rows = (64 * torch.arange(n // 64)[:, None, None] + pi[None]).to(w.device)          # [c, u, r]
    kap = kap.to(w.device)
    # frag[c, u, s, hi, r, j]
    frag = w.detach()[rows[:, :, None, None, :, None], kap[None, None, :, :, None, :]].contiguous()
    fb = frag.reshape(n // 64, -1).view(torch.uint8)                                      # [c, 128 K bytes]
    page = torch.zeros(n // 64, 256, dtype=torch.float32, device=w.device)
    if v is not None:
        page[:, :64] = v.detach().float().reshape(n // 64, 64)
    if u is not None:
        page[:, 64:128] = u.detach().float().reshape(n // 64, 64)
    return torch.cat([fb, page.view(torch.uint8)], dim=1).contiguous().reshape(-1)


def rc_pack_tiles(w: torch.Tensor, v: torch.Tensor = None, u: torch.Tensor = None, page: bool = True) -> torch.Tensor:
    """As ``rc_pack`` but one stream element per 32-row MFMA TILE (tile t = 2 c + u of chunk c): K / 16 fragment blocks, then a 1-KiB
    vector page with fp32 v[32] and u[32] in the tile's accumulator order (index 16 hi + rho <-> channel 64 c + 32 hi + 16 u + rho);
    3 KiB of zero padding behind the last tile (the consumer fetches every (K / 16 + 1)-KiB tile as a 24-KiB stage)."""
    n, k = w.shape
    assert n % 64 == 0 and k % 64 == 0, (n, k)
    pi, kap = _rc_maps(k)
    rows = (64 * torch.arange(n // 64)[:, None, None] + pi[None]).to(w.device)          # [c, u, r]
    kap = kap.to(w.device)
    frag = w.detach()[rows[:, :, None, None, :, None], kap[None, None, :, :, None, :]].contiguous()   # [c, u, s, hi, r, j]
    fb = frag.reshape(n // 32, -1).view(torch.uint8)                                      # [tile, 64 K bytes]
    if not page:                       # K = 640 streams (tg_rc_linear): four 40-KiB tiles fill the LDS, the vectors travel as plain fp32 arrays
        return fb.contiguous().reshape(-1)
    page = torch.zeros(n // 32, 256, dtype=torch.float32, device=w.device)

    def tile_order(x):      # [N] -> [tile = 2 c + u, 16 hi + rho]
        return x.detach().float().reshape(n // 64, 2, 2, 16).permute(0, 2, 1, 3).reshape(n // 32, 32)
    if v is not None:
        page[:, :32] = tile_order(v)
    if u is not None:
        page[:, 32:64] = tile_order(u)
    out = torch.cat([fb, page.view(torch.uint8)], dim=1).contiguous().reshape(-1)
    return torch.cat([out, torch.zeros(3 * 1024, dtype=torch.uint8, device=w.device)])


def convtranspose2x2_matrices(w: torch.Tensor) -> torch.Tensor:
    """ConvTranspose2d weight [Cin, Cout, 2, 2] with stride 2 -> [4, Cout, Cin]: matrix 2 a + b makes output pixel (2 i + a, 2 j + b) from input pixel
    (i, j) alone (kernel = stride: no two input pixels meet in one output pixel)."""
    cin, cout, kh, kw = w.shape
    assert kh == 2 and kw == 2
    return w.detach().permute(2, 3, 1, 0).reshape(4, cout, cin).contiguous()


def sam_upscale_k_order() -> torch.Tensor:
    """[4, 2, 8] long: the input channel of element j of lane half hi in k-step ks of tg_sam_mask_head's second GEMM = the accumulator order of its first
    (register 8 (ks & 1) + j of 32-channel tile ks >> 1): 16 ks + 8 (j >> 2) + 4 hi + (j & 3)."""
    ks = torch.arange(4)[:, None, None]
    hi = torch.arange(2)[None, :, None]
    j = torch.arange(8)[None, None, :]
    return 16 * ks + 8 * (j >> 2) + 4 * hi + (j & 3)


def pack_sam_upscale(conv1_w, conv1_b, ln_w, ln_b, conv2_w, conv2_b):
    """SAM mask decoder's ``upscale_conv1`` [256, 64, 2, 2], ``upscale_layer_norm`` [64] and ``upscale_conv2`` [64, 32, 2, 2] -> what tg_sam_mask_head reads:
      w1  [4 (a, b), 2 tiles, 16 k-steps, 64 lanes, 8]: lane (hi, l31), element j = M1[ab][32 tile + l31, 16 ks + 8 hi + j]   (A operand of a 32x32x16 MFMA)
      w2  [4 (a', b'), 4 k-steps, 64 lanes, 8]:          lane (hi, l31), element j = M2[a'b'][l31, sam_upscale_k_order()[ks, hi, j]]
      vec fp32 [224] = conv1 bias | LayerNorm weight | LayerNorm bias | conv2 bias
    with M = ``convtranspose2x2_matrices``; w1 / w2 keep the weights' dtype."""
    assert tuple(conv1_w.shape) == (256, 64, 2, 2) and tuple(conv2_w.shape) == (64, 32, 2, 2), (conv1_w.shape, conv2_w.shape)
    m1 = convtranspose2x2_matrices(conv1_w)                                                       # [4, 64, 256]
    w1 = m1.reshape(4, 2, 32, 16, 2, 8).permute(0, 1, 3, 4, 2, 5).contiguous().reshape(-1)       # [ab, tile, ks, hi, l31, j]
    m2 = convtranspose2x2_matrices(conv2_w)                                                       # [4, 32, 64]
    kap = sam_upscale_k_order().to(m2.device)
    w2 = m2[:, :, kap].permute(0, 2, 3, 1, 4).contiguous().reshape(-1)                           # [a'b', l31, ks, hi, j] -> [a'b', ks, hi, l31, j]
    vec = torch.cat([t.detach().float().reshape(-1) for t in (conv1_b, ln_w, ln_b, conv2_b)]).contiguous()
    assert vec.numel() == 224
    return w1, w2, vec


def skinny_pack(w: torch.Tensor) -> torch.Tensor:
    """Linear weight [N, K] (N % 32 == 0, K % 16 == 0) -> tg_skinny_gemm's fragment order: block (nt, ks) = 64 lanes x 8 elements, lane (hi, l31), element j =
    W[32 nt + l31, 16 ks + 8 hi + j] — the A operand of one 32x32x16 MFMA as ONE contiguous KiB, so the weight stream is whole-line loads in K order."""
    n, k = w.shape
    assert n % 32 == 0 and k % 16 == 0, (n, k)
    return w.detach().reshape(n // 32, 32, k // 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous().reshape(-1)
