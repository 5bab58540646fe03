"""CPU: the C-ABI side of the CFG pair's shared UNet prefix (second-destination stores).

The change is additive to ABI 308: three entry points (``tg_rc_linear_dup``, ``tg_conv_in_dup``, ``tg_dup_rows``) and one query
(``tg_conv_in_takes_dup``), no descriptor change.  Checked here: header, ``_lib.SIGNATURES`` and the built library agree on them, the ``*_dup``
signatures are their plain entry points' with one ``int64_t`` offset in front of the stream, the query (host code only: it runs without a GPU) answers
yes for conv_in on the matrix cores and no elsewhere, the argument errors that are decided on the host, and the row gate of ``shared_pair``.
"""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tg_rc_linear_dup", "tg_conv_in_dup", "tg_conv_in_takes_dup", "tg_dup_rows")


def _libs():
    from theatergen_amd import _lib
    return _lib, _lib.lib()


def test_dup_symbols_are_declared_bound_and_exported():
    _lib, h = _libs()
    header = open(os.path.join(ROOT, "include", "theatergen_hip.h")).read()
    for name in NEW:
        assert re.search(r"^int\s+%s\s*\(" % name, header, flags=re.M), f"{name} is not declared"
        assert name in _lib.SIGNATURES and getattr(h, name) is not None, f"{name} is not bound / exported"
    S = _lib.SIGNATURES
    for plain, dup in (("tg_rc_linear", "tg_rc_linear_dup"), ("tg_conv_in", "tg_conv_in_dup")):
        res, args = S[plain]
        assert S[dup] == (res, args[:-1] + [_lib.i64, _lib.vp]), dup
    # no descriptor grew: the version stays what the other bindings of this ABI family were built against
    assert int(re.search(r"#define TG_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == h.tg_version()


def test_conv_in_takes_dup_query():
    _lib, h = _libs()
    assert h.tg_conv_in_takes_dup(4, 320) == 1 and h.tg_conv_in_takes_dup(4, 640) == 1          # the matrix-core kernel: cin 4, cout % 160 == 0, <= 640
    assert h.tg_conv_in_takes_dup(4, 64) == 0 and h.tg_conv_in_takes_dup(8, 320) == 0 and h.tg_conv_in_takes_dup(4, 800) == 0


def test_dup_entry_points_refuse_on_the_host_before_any_launch():
    """argument errors come from host-side validation: no device is touched, so they can be checked here"""
    _lib, h = _libs()
    # cout = 64: not the matrix-core kernel, the offset is refused, never ignored
    assert h.tg_conv_in_dup(0, 16, 0, 1, 4, 16, 16, 16, None, 64, 16, 16 * 16 * 64, None) == -1 and b"tg_conv_in_dup" in h.tg_last_error()
    # the matrix-core kernel: an offset that is no multiple of 8 / that lands inside the first destination
    assert h.tg_conv_in_dup(0, 16, 0, 1, 4, 16, 16, 16, None, 320, 16, 16 * 16 * 320 + 4, None) == -1
    assert h.tg_conv_in_dup(0, 16, 0, 1, 4, 16, 16, 16, None, 320, 16, 8 * 320, None) == -1
    d = _lib.RcLinearDesc()
    d.dtype, d.x, d.ldx, d.wpk, d.out, d.ldc, d.M, d.N, d.K = 0, 16, 320, 16, 16, 320, 250, 320, 320
    assert h.tg_rc_linear_dup(C.byref(d), 249 * 320, None) == -1                                 # overlaps the last row of the first destination
    assert h.tg_rc_linear_dup(C.byref(d), 250 * 320 + 4, None) == -1                             # not a multiple of 8
    assert h.tg_dup_rows(16, 1 << 20, 4, 12, 16, 0, None) == -1                                  # cols % 8
    assert h.tg_dup_rows(16, 32, 4, 8, 8, 0, None) == -1                                         # overlap


def test_shared_pair_is_gated_on_the_row_chain_threshold():
    """the prefix is shared only where the half batch gets the kernel family the full batch gets: SD-1.5's level 0 picks the row-chain launches by row
    count, so 4 .. 7 images of 64 x 64 (full batch at or above the threshold, half below) are not shared; 1 .. 3 and 8 and more are"""
    import torch
    from theatergen_amd import config, rowchain
    from theatergen_amd.unet import UNet2DConditionModel
    with torch.device("meta"):
        sd = UNet2DConditionModel(config.UNetConfig(block_out_channels=(320, 640), down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"),
                                                    up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"), layers_per_block=1))
        tiny = UNet2DConditionModel(config.tiny())
    assert rowchain.ENABLED and rowchain.MIN_ROWS_CHAIN == 32768
    got = [sd._pair_prefix_ok({}, 2 * n * 4096) for n in range(1, 10)]
    assert got == [True, True, True, False, False, False, False, True, True], got
    assert all(tiny._pair_prefix_ok({}, 2 * n * 4096) for n in range(1, 10))                      # 64 channels: no row-chain launches to lose
    assert not sd._pair_prefix_ok({"save_attn_to_dict": {}}, 2 * 8 * 4096)
    a1 = sd.down_blocks[0].attentions[0].transformer_blocks[0].attn1
    a1.residual_connection = True
    assert not sd._pair_prefix_ok({}, 2 * 8 * 4096)
