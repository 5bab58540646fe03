"""CPU (no GPU): ``rowchain.pack_ff2`` / ``pack_po2`` against an emulation of what ``rc_ff2_kernel`` (csrc/tg_rowchain.hip) does with the streams.

The kernel runs v_mfma_f32_16x16x32: the A fragment of lane (r = lane & 15, g = lane >> 4) is row r, k = 8 g + e; the B fragment of lane (n, g) is
column n (the token), k = 8 g + e; accumulator register i of lane (n, g) is D[4 g + i, n].  The emulation walks the streams in the kernel's order —
value / gate fragment k = 2 s + u over the rows' B pieces (channel 32 s + 8 g + e), GEGLU on the registers, the registers of the two value tiles
as net.2's B piece, output tile t = 2 s + u whose registers are elements 4 u + i of the rows' piece s, the proj_out tail over those pieces — and
must reproduce the plain matrix products.
"""
import pytest
import torch
import torch.nn.functional as F

from theatergen_amd import rowchain

C = 320


def _mfma16(a_frag, b_frag):
    """a_frag [g, r, e], b_frag [g, n, e] -> D [16 rows, 16 tokens] of one 16x16x32 MFMA"""
    A = a_frag.permute(1, 0, 2).reshape(16, 32)
    B = b_frag.permute(1, 0, 2).reshape(16, 32)
    return A @ B.T


def _regs(D):
    """D [16, 16] -> registers [g, n, i] = D[4 g + i, n]"""
    return D.reshape(4, 4, 16).permute(0, 2, 1)


def _row_pieces(x):
    """rows [16, 320] -> B pieces [s, g, n, e] = x[n, 32 s + 8 g + e]"""
    return x.reshape(16, 10, 4, 8).permute(1, 2, 0, 3)


def _rows_of(pieces):
    """inverse of _row_pieces"""
    return pieces.permute(2, 0, 1, 3).reshape(16, C)


def _tiles_to_pieces(tiles):
    """20 register tiles [t = 2 s + u][g, n, i] -> the rows' pieces [s, g, n, e = 4 u + i]"""
    return torch.stack([torch.cat([tiles[2 * s], tiles[2 * s + 1]], dim=-1) for s in range(10)])


@pytest.mark.parametrize("inner,dt", [(64, torch.bfloat16), (128, torch.float16)], ids=["i64_bf16", "i128_fp16"])
def test_pack_ff2_and_po2_streams_emulated(inner, dt):
    """two and four slices (the slice stride of both streams), both 2-byte views"""
    torch.manual_seed(2)
    w1 = (torch.randn(2 * inner, C) / C ** 0.5).to(dt)
    b1 = 0.2 * torch.randn(2 * inner)
    w2 = (torch.randn(C, inner) / inner ** 0.5).to(dt)
    b2 = 0.1 * torch.randn(C)
    wp = (torch.randn(C, C) / C ** 0.5).to(dt)
    bp = 0.1 * torch.randn(C)
    gamma, beta = 1 + 0.2 * torch.randn(C), 0.1 * torch.randn(C)
    xn = torch.randn(16, C)                                          # one wave's normalised rows
    s1, s2, bb2 = rowchain.pack_ff2(w1, b1, gamma, beta, w2, b2)
    ns = inner // 32
    assert s1.numel() == ns * 41 * 1024 + 3072 and s2.numel() == ns * 20 * 1024

    HN = _row_pieces(xn)
    out = [bb2.reshape(10, 4, 2, 4)[s, :, u][:, None, :].repeat(1, 16, 1) for s in range(10) for u in range(2)]     # tile t: [g, n, i] = b2[32 s + 8 g + 4 u + i]
    for j in range(ns):
        blk = s1[j * 41 * 1024:(j + 1) * 41 * 1024]
        frag = blk[:40 * 1024].view(dt).float().reshape(2, 20, 4, 16, 8)       # [value / gate][k = 2 s + u][g][r][e]
        page = blk[40 * 1024:].view(torch.float32)
        acc = torch.zeros(2, 2, 4, 16, 4)                                                    # [value / gate][u][g, n, i]
        for which in range(2):
            for u in range(2):
                acc[which, u] = page[32 * which + 16 * u:32 * which + 16 * u + 16].reshape(4, 1, 4)    # register i of lane group g <- page[16 u + 4 g + i]
            for k in range(20):
                acc[which, k & 1] += _regs(_mfma16(frag[which, k], HN[k >> 1]))
        hid = torch.cat([acc[0, u] * F.gelu(acc[1, u]) for u in range(2)], dim=-1)          # [g, n, e = 4 u + i]
        f2 = s2[j * 20 * 1024:(j + 1) * 20 * 1024].view(dt).float().reshape(20, 4, 16, 8)
        for t in range(20):
            out[t] = out[t] + _regs(_mfma16(f2[t], hid))
    h3 = _tiles_to_pieces(out)
    w1g = (w1.float() * gamma[None, :]).to(dt).float()          # rounded once, as the stream holds it
    pr = xn @ w1g.T + (w1.float() @ beta + b1)
    ref = (pr[:, :inner] * F.gelu(pr[:, inner:])) @ w2.float().T + b2
    assert (_rows_of(h3) - ref).abs().max() < 2e-4

    # the proj_out tail over the pieces the accumulators form
    sp = rowchain.pack_po2(wp, bp)
    assert sp.numel() == 10 * 21 * 1024 + 3072
    tiles = []
    for st in range(10):
        blk = sp[st * 21 * 1024:(st + 1) * 21 * 1024]
        frag = blk[:20 * 1024].view(dt).float().reshape(20, 4, 16, 8)
        page = blk[20 * 1024:].view(torch.float32)
        acc = [page[16 * u:16 * u + 16].reshape(4, 1, 4).repeat(1, 16, 1) for u in range(2)]
        for k in range(20):
            acc[k & 1] = acc[k & 1] + _regs(_mfma16(frag[k], h3[k >> 1]))
        tiles += acc
    got = _rows_of(_tiles_to_pieces(tiles))
    assert (got - (_rows_of(h3) @ wp.float().T + bp)).abs().max() < 2e-4
    assert torch.equal(rowchain.pack_po2(wp, None)[:20 * 1024], sp[:20 * 1024])


def test_two_wave_kernel_is_the_default_and_switchable():
    """the header defines the stream-format tag ``TG_RC_FF_TWO_WAVE`` with the binding's value; every row-chain launch is on by default (``TG_RC_MODE``
    bits 0 - 3; bit 5 chose between two kernels while there were two and is ignored)"""
    import os
    if "TG_RC_MODE" not in os.environ:
        assert rowchain.MODE & 15 == 15
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "theatergen_hip.h")).read()
    assert f"#define TG_RC_FF_TWO_WAVE 0x{rowchain.FF_TWO_WAVE:x}" in header


def test_retired_switch_names_are_gone():
    """the A/B arms that lost were deleted with their switches (profiles/retired_arms_findings.md, rc_ff_one_wave_retired_findings.md): no source of
    the package names one any more.  The last three are literal strings with their bracket, so that ``pack_ff2`` and ``rc_ff2_kernel`` do not hit"""
    import glob
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    retired = ["TG_NO_GN_FUSE", "TG_NO_LN_FUSE", "TG_LN_MODE", "TG_LN_FF_MAX_ROWS", "TG_CONV_OUT_GN", "TG_FF_PAD", "TG_RESAMPLER_SIDE", "TG_CONV_IN_MFMA",
               "TG_CONV_OUT_MFMA", "TG_ATTN_NOFOLD", "TG_ATTN_PIPE", "TG_RC_DEV", "TG_RC_DEV_BUILD", "pack_ff(", "rc_ff_kernel<", "two_wave="]
    files = (glob.glob(os.path.join(root, "theatergen_amd", "**", "*.py"), recursive=True) + glob.glob(os.path.join(root, "theatergen_amd", "csrc", "*"))
             + glob.glob(os.path.join(root, "include", "*")))
    files = [f for f in files if os.path.isfile(f)]
    assert len(files) > 40
    hits = [(os.path.relpath(f, root), name) for f in files for text in [open(f, errors="replace").read()] for name in retired if name in text]
    assert not hits, hits
