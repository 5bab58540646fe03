"""CPU (no GPU): the host side of the annotator's two cv2 resizes: the per-axis tables of theatergen_amd/cv_resize.py against the NumPy restatement of
tests/cv_resize_reference.py, the restatement itself on hand-computed cases, the detector's resize planner, and the C-ABI declarations.

The 1e-3 thresholds of the INTER_AREA table.  For 1000 -> 999 every head entry has s1 - f1 = 1 - 0.001001 d >= 0.001001 and every tail entry f2 - s2 =
0.001001 (d + 1) >= 0.001001: the entries come down to within 1.1e-6 of the threshold but none falls below it, so no entry is dropped at that size
(checked below: the smallest kept overlap is within 2e-6 of 1e-3).  2001 -> 2000 (scale 1.0005) is added for the other side: the tail of d = 0 overlaps its
source pixel by 0.0005 and is dropped, which the test asserts."""
import math
import os
import re

import numpy as np
import pytest

from tests import cv_resize_reference as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("tg_cv_area_u8", "tg_cv_linear_u8")
AREA_CASES = [(1024, 384), (64, 24), (53, 20), (1000, 999), (2001, 2000)]


def _plan_entries(plan):
    return [(d, int(plan.first[d]) + t, plan.alpha[d, t]) for d in range(plan.out_size) for t in range(int(plan.count[d]))]


def _overlaps(ssize, dsize):
    """the head and tail overlaps (s1 - f1, f2 - s2) of every destination index, in the table's own double arithmetic"""
    scale, heads, tails = ssize / dsize, [], []
    for d in range(dsize):
        f1 = d * scale
        f2 = f1 + scale
        s2 = min(math.floor(f2), ssize - 1)
        s1 = min(math.ceil(f1), s2)
        heads.append(s1 - f1)
        tails.append(f2 - s2)
    return np.array(heads), np.array(tails)


@pytest.mark.parametrize("ssize,dsize", AREA_CASES)
def test_area_tables_equal_the_restatement(ssize, dsize):
    from theatergen_amd import cv_resize
    plan = cv_resize.area_plan(ssize, dsize)
    want = CR.area_entries(ssize, dsize)
    got = _plan_entries(plan)
    assert len(got) == len(want)
    assert [(d, s) for d, s, _ in got] == [(d, s) for d, s, _ in want]
    assert np.array_equal(np.array([a for *_, a in got], dtype=np.float32).view(np.uint32), np.array([a for *_, a in want], dtype=np.float32).view(np.uint32))
    assert plan.alpha.dtype == np.float32 and plan.first.dtype == np.int32 and plan.count.dtype == np.int32
    assert not plan.integer and plan.in_size == ssize and plan.out_size == dsize
    # every destination index reads consecutive source pixels inside the axis
    assert (plan.first >= 0).all() and (plan.first + plan.count <= ssize).all() and (plan.count >= 1).all()
    assert cv_resize.area_plan(ssize, dsize) is plan                               # cached


def test_area_table_thresholds():
    heads, tails = _overlaps(1000, 999)
    kept = np.concatenate([heads[heads > 1e-3], tails[tails > 1e-3]])
    assert 1e-3 < kept.min() < 1e-3 + 2e-6                                        # entries straddle the threshold from above ...
    assert not ((heads > 0) & (heads <= 1e-3)).any() and not ((tails > 0) & (tails <= 1e-3)).any()      # ... and none is dropped at this size
    heads, tails = _overlaps(2001, 2000)
    dropped = int(((heads > 0) & (heads <= 1e-3)).sum() + ((tails > 0) & (tails <= 1e-3)).sum())
    assert dropped >= 1                                                            # here the threshold does drop entries
    # d = 0: one whole source pixel, the 0.0005 tail gone: the weights no longer sum to one
    assert [e for e in CR.area_entries(2001, 2000) if e[0] == 0] == [(0, 0, np.float32(1.0 / 1.0005))]


def test_area_plan_limits():
    from theatergen_amd import _lib, cv_resize
    assert cv_resize.area_is_integer(1024, 64) and cv_resize.area_is_integer(512, 512) and not cv_resize.area_is_integer(1024, 384)
    assert cv_resize.area_plan(48, 24).integer and cv_resize.area_plan(48, 24).iscale == 2
    with pytest.raises(NotImplementedError, match="grows"):
        cv_resize.area_plan(20, 53)
    with pytest.raises(NotImplementedError, match=str(_lib.CV_AREA_MAX_TAPS)):
        cv_resize.area_plan(1000, 64)                                              # 15.6 source pixels per destination pixel
    assert cv_resize.area_plan(1024, 384).alpha.shape[1] == 4                      # the SDXL call: at most 4 entries per axis
    assert cv_resize.area_stage_rows(cv_resize.area_plan(1024, 384)) <= _lib.CV_AREA_STAGE_ROWS


@pytest.mark.parametrize("ssize,dsize", [(384, 1024), (24, 64), (20, 53), (96, 36), (3, 8), (8, 3), (7, 7)])
def test_linear_tables_equal_the_restatement(ssize, dsize):
    from theatergen_amd import cv_resize
    plan = cv_resize.linear_plan(ssize, dsize)
    assert plan.table.dtype == np.int32 and plan.table.shape == (dsize, 4)
    for col, want in enumerate(CR.linear_table(ssize, dsize)):
        assert np.array_equal(plan.table[:, col], want), col
    assert (plan.table[:, :2] >= 0).all() and (plan.table[:, :2] <= ssize - 1).all()


# ---- the restatement itself, on cases computed by hand -----------------------------------------------------------------------------------------------

def test_restatement_integer_blocks():
    # 2 x 2: (a + b + c + d + 2) >> 2; a sum of 2 rounds UP to 1 (round-half-even of 0.5 would give 0)
    img = np.array([[1, 2, 1, 1], [3, 5, 0, 0]], dtype=np.uint8)[:, :, None].repeat(3, axis=2)
    assert CR.area_u8(img, 1, 2)[0, :, 0].tolist() == [(1 + 2 + 3 + 5 + 2) >> 2, 1]
    # 3 x 4 (3 rows, 4 columns per block): rint(float32(sum) * float32(1 / 12))
    blk = np.zeros((3, 8, 1), dtype=np.uint8)
    blk[:, :4, 0] = [[10, 10, 10, 10], [5, 5, 5, 5], [10, 10, 10, 10]]             # sum 100 -> 8.33 -> 8
    blk[:, 4:, 0] = 255                                                            # sum 3060 -> 255
    assert CR.area_u8(blk, 1, 2)[0, :, 0].tolist() == [8, 255]
    blk[:, :4, 0] = [[50, 50, 50, 50], [0, 0, 0, 0], [0, 0, 0, 0]]                 # sum 200 -> 16.67 -> 17
    assert CR.area_u8(blk, 1, 2)[0, 0, 0] == 17
    same = np.arange(24, dtype=np.uint8).reshape(2, 4, 3)
    assert np.array_equal(CR.area_u8(same, 2, 4), same)                            # equal sizes: the copy


@pytest.mark.parametrize("value", [0, 1, 127, 200, 255])
def test_restatement_keeps_a_constant_image_constant(value):
    img = np.full((53, 64, 3), value, dtype=np.uint8)
    for hd, wd in ((20, 24), (53, 24), (20, 64), (52, 63)):
        assert (CR.area_u8(img, hd, wd) == value).all(), (hd, wd)
    for hd, wd in ((20, 24), (141, 171), (53, 171), (20, 64)):
        assert (CR.linear_u8(img, hd, wd) == value).all(), (hd, wd)
        assert (CR.annotator_tail(img, hd, wd) == 255 - value).all()


def test_restatement_general_area_by_hand():
    # 3 -> 2 on one row: scale 1.5; d = 0: (0, 1 / 1.5), (1, 0.5 / 1.5); d = 1: (1, 0.5 / 1.5), (2, 1 / 1.5)
    tab = CR.area_entries(3, 2)
    assert [(d, s) for d, s, _ in tab] == [(0, 0), (0, 1), (1, 1), (1, 2)]
    assert [a for *_, a in tab] == [np.float32(1 / 1.5), np.float32(0.5 / 1.5), np.float32(0.5 / 1.5), np.float32(1 / 1.5)]
    row = np.array([[[30], [60], [90]]], dtype=np.uint8)                           # [1, 3, 1]
    # 30 * 2/3 + 60 * 1/3 = 40, 60 * 1/3 + 90 * 2/3 = 80 (the vertical axis is the identity: beta = 1)
    assert CR.area_u8(row, 1, 2)[0, :, 0].tolist() == [40, 80]


def test_restatement_linear_edge_clamps():
    s0, s1, c0, c1 = CR.linear_table(3, 8)                                         # scale 0.375
    assert (s0[0], s1[0], c0[0], c1[0]) == (0, 1, 2048, 0)                         # f = -0.3125: s = -1 -> s = 0, f = 0
    assert (s0[7], s1[7], c0[7], c1[7]) == (2, 2, 2048, 0)                         # f = 2.3125: s = 2 >= ssize - 1 -> f = 0, second tap clamped
    assert (s0[1], s1[1], c0[1], c1[1]) == (0, 1, 2048 - 128, 128)                 # f = 0.0625
    s0, s1, c0, c1 = CR.linear_table(8, 3)                                         # scale 8 / 3
    assert (s0[0], s1[0], c0[0], c1[0]) == (0, 1, 341, 1707)                       # f = 0.8333
    assert (s0[2], s1[2], c0[2], c1[2]) == (6, 7, 1707, 341)                       # f = 6.1667: s = 6 < ssize - 1
    img = np.array([[10, 100, 250]], dtype=np.uint8).repeat(3, axis=0)[:, :, None]
    out = CR.linear_u8(img, 8, 8)
    assert out[0, 0, 0] == 10 and out[7, 7, 0] == 250                              # a coefficient of 2048 returns the byte itself
    # column 1: r = 10 * 1920 + 100 * 128 = 32000; rows are equal: ((2048 * (32000 >> 4)) >> 16) = 62 (62.5 truncated) -> (62 + 0 + 2) >> 2 = 16
    assert out[0, 1, 0] == 16


def test_inversion_does_not_commute_with_the_fixed_point_rounding():
    """why the kernel takes `invert` instead of resizing the inverted map: 255 - linear(t) differs from linear(255 - t) somewhere"""
    rng = np.random.default_rng(5)
    t = rng.integers(0, 256, size=(14, 20, 1), dtype=np.uint8)
    assert (CR.annotator_tail(t, 37, 53) != CR.linear_u8(255 - t, 37, 53)).any()


# ---- the planner ---------------------------------------------------------------------------------------------------------------------------------------

def test_planner():
    from theatergen_amd.lineart import plan_resizes
    p = plan_resizes(1024, 1024, 384, 1024)
    assert p.net == (384, 384) and p.out == (1024, 1024) and p.area and p.linear
    p = plan_resizes(512, 512, 192, 512)
    assert p.net == (192, 192) and p.out == (512, 512) and p.area and p.linear
    p = plan_resizes(512, 768, 512, 512)
    assert p.net == (512, 768) and p.out == (512, 768) and not p.area and not p.linear          # the identity: no launches
    p = plan_resizes(128, 192, 64, 64)
    assert p.net == (64, 128) and p.out == (64, 128) and p.area and not p.linear
    p = plan_resizes(512, 512, 512, 1024)
    assert p.net == (512, 512) and p.out == (1024, 1024) and not p.area and p.linear
    for h, w in ((64, 64), (500, 500)):
        with pytest.raises(NotImplementedError, match="LANCZOS4"):
            plan_resizes(h, w, 512, 512)
    with pytest.raises(NotImplementedError, match="growing"):
        plan_resizes(500, 500, 499, 512)                                           # k < 1, but 500 rounds up to 512


def test_detector_raises_before_any_device_work():
    from theatergen_amd.lineart import LineartDetector, LineartGenerator
    det = LineartDetector(LineartGenerator())                                      # a CPU module: device work would raise RuntimeError instead
    with pytest.raises(NotImplementedError, match="LANCZOS4"):
        det(np.zeros((500, 500, 3), np.uint8))
    with pytest.raises(NotImplementedError, match="LANCZOS4"):
        det.detect_many([np.zeros((64, 64, 3), np.uint8)] * 2, detect_resolution=384, image_resolution=1024)
    with pytest.raises(ValueError, match="output_type"):
        det(np.zeros((512, 512, 3), np.uint8), output_type="jpeg")


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------------------------

def test_new_symbols_are_declared_and_bound():
    from theatergen_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "theatergen_hip.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t)\s+(tg_[a-z0-9_]+)\s*\(", header, flags=re.M))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
    assert _lib.ABI_VERSION == 308 and "#define TG_ABI_VERSION 308" in header
    for macro, value in (("TG_CV_AREA_MAX_TAPS", _lib.CV_AREA_MAX_TAPS), ("TG_CV_AREA_STAGE_ROWS", _lib.CV_AREA_STAGE_ROWS),
                         ("TG_CV_RESIZE_MAX_SIZE", _lib.CV_RESIZE_MAX_SIZE)):
        assert f"#define {macro} {value}\n" in header
    assert any(sub == "cv_area_kernel<" for sub, *_ in build.HOT_GATES) and any(sub == "cv_linear_kernel<" for sub, *_ in build.HOT_GATES)
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    h = _lib.lib()
    for name in NEW_SYMBOLS:
        assert getattr(h, name) is not None


def test_bad_arguments_return_minus_one_with_the_entry_points_name():
    """host-side validation, before any launch: the pointers are never dereferenced"""
    from theatergen_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    h = _lib.lib()
    SRC, DST, U8, TAB = 4096, 8192, 12288, 16384

    def area(src=SRC, batch=1, hs=8, ws=8, hd=4, wd=4, tables=(None, None, None, 0, None, None, None, 0), rows=0, dst=DST, dtype=0, u8=None):
        return h.tg_cv_area_u8(src, batch, hs, ws, hd, wd, *tables, rows, dst, dtype, u8, None)

    def linear(src=SRC, batch=1, hs=8, ws=8, hd=16, wd=16, tv=TAB, th=TAB + 4096, invert=0, u8=U8, dst=None, dtype=0):
        return h.tg_cv_linear_u8(src, batch, hs, ws, hd, wd, tv, th, invert, u8, dst, dtype, None)

    full = (TAB, TAB, TAB, 4, TAB, TAB, TAB, 4)
    for call, text in ((lambda: area(src=None), b"null"), (lambda: area(dst=SRC), b"different"), (lambda: area(batch=0), b"size"),
                       (lambda: area(hs=9000), b"size"), (lambda: area(hd=16), b"grows"), (lambda: area(dtype=7), b"dst_dtype"),
                       (lambda: area(hd=3, wd=3), b"tables"), (lambda: area(hd=3, wd=3, tables=full[:3] + (9,) + full[4:], rows=8), b"ksize"),
                       (lambda: area(hd=3, wd=3, tables=full, rows=_lib.CV_AREA_STAGE_ROWS + 1), b"stage_rows"),
                       (lambda: area(hd=3, wd=3, tables=full, rows=0), b"stage_rows")):
        assert call() == -1
        err = h.tg_last_error()
        assert b"tg_cv_area_u8" in err and text in err, err
    for call, text in ((lambda: linear(src=None), b"null"), (lambda: linear(tv=None), b"null"), (lambda: linear(u8=None), b"no output"),
                       (lambda: linear(u8=SRC), b"different"), (lambda: linear(wd=0), b"size"), (lambda: linear(invert=2), b"invert"),
                       (lambda: linear(dst=DST, dtype=5), b"dst_dtype"), (lambda: linear(tv=TAB + 4), b"aligned")):
        assert call() == -1
        err = h.tg_last_error()
        assert b"tg_cv_linear_u8" in err and text in err, err
