"""``cv2.resize`` with INTER_AREA (shrinking) and INTER_LINEAR on uint8 images, restated in NumPy (the oracle of tests/test_cv_resize_*.py; no dependency on
cv2, which these machines do not have).

Written from OpenCV's modules/imgproc/src/resize.cpp — its portable C++ path: ``computeResizeAreaTab`` + ``ResizeArea_Invoker``, ``resizeAreaFast_`` with
``ResizeAreaFastVec`` for 2 x 2, and the INTER_LINEAR branch of ``resize`` with ``HResizeLinear`` / ``VResizeLinear<uchar, int, short, FixedPtCast<int,
uchar, 22>>`` — and NOT run against the package: an IPP build, or a compiler that contracts the float products into FMAs, may give other bytes.

The entry lists are plain Python floats (C doubles) rounded to float32 where the C code stores a float; the pixel arithmetic uses NumPy float32 / int32
arrays, where every product and every sum is one rounded operation."""
import math

import numpy as np

DBL_EPSILON = float(np.finfo(np.float64).eps)


def is_integer_scale(ssize, dsize):
    scale = ssize / dsize
    return abs(scale - int(scale)) < DBL_EPSILON


def area_entries(ssize, dsize):
    """[(destination index, source index, float32 weight)] in destination order (``computeResizeAreaTab``)"""
    assert dsize <= ssize
    scale = ssize / dsize
    tab = []
    for d in range(dsize):
        f1 = d * scale
        f2 = f1 + scale
        cell = min(scale, ssize - f1)
        s1 = math.ceil(f1)
        s2 = min(math.floor(f2), ssize - 1)
        s1 = min(s1, s2)
        if s1 - f1 > 1e-3:
            tab.append((d, s1 - 1, np.float32((s1 - f1) / cell)))
        for s in range(s1, s2):
            tab.append((d, s, np.float32(1.0 / cell)))
        if f2 - s2 > 1e-3:
            tab.append((d, s2, np.float32(min(min(f2 - s2, 1.0), cell) / cell)))
    return tab


def _round_u8(x):
    """saturate_cast<uchar>(float): round half to even, then 0 .. 255"""
    return np.clip(np.rint(x), 0, 255).astype(np.uint8)


def area_u8(img, hd, wd):
    """``cv2.resize(img, (wd, hd), interpolation=cv2.INTER_AREA)`` for uint8 ``[hs, ws, C]`` with ``hd <= hs`` and ``wd <= ws``"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3
    hs, ws, ch = img.shape
    if hd > hs or wd > ws:
        raise NotImplementedError("INTER_AREA on a growing axis")
    if (hd, wd) == (hs, ws):
        return img.copy()
    if is_integer_scale(hs, hd) and is_integer_scale(ws, wd):
        sy, sx = int(hs / hd), int(ws / wd)
        block = img[:hd * sy, :wd * sx].reshape(hd, sy, wd, sx, ch).astype(np.int32).sum(axis=(1, 3), dtype=np.int32)
        if sy == 2 and sx == 2:
            return ((block + 2) >> 2).astype(np.uint8)
        return _round_u8(block.astype(np.float32) * np.float32(1.0 / (sx * sy)))
    src = img.astype(np.float32)
    buf = np.zeros((hs, wd, ch), dtype=np.float32)                                 # the horizontal row of every source row (a row's is the same for
    for dx, sx, alpha in area_entries(ws, wd):                                     # every destination row that reads it)
        buf[:, dx] = buf[:, dx] + src[:, sx] * alpha
    out = np.zeros((hd, wd, ch), dtype=np.float32)
    prev = -1
    for dy, sy, beta in area_entries(hs, hd):
        if dy != prev:
            out[dy] = beta * buf[sy]
            prev = dy
        else:
            out[dy] = out[dy] + beta * buf[sy]
    return _round_u8(out)


def linear_table(ssize, dsize):
    """(s0, s1, c0, c1) int32 arrays [dsize]: the two taps and their 11-bit coefficients"""
    scale = ssize / dsize
    s0, s1, c0, c1 = [], [], [], []
    for d in range(dsize):
        f = np.float32((d + 0.5) * scale - 0.5)
        s = int(math.floor(f))
        f = np.float32(f - np.float32(s))
        if s < 0:
            s, f = 0, np.float32(0)
        if s >= ssize - 1:
            s, f = ssize - 1, np.float32(0)
        s0.append(s)
        s1.append(min(s + 1, ssize - 1))
        c0.append(int(np.clip(np.rint(np.float32(np.float32(1) - f) * np.float32(2048)), -32768, 32767)))
        c1.append(int(np.clip(np.rint(f * np.float32(2048)), -32768, 32767)))
    return tuple(np.asarray(a, dtype=np.int32) for a in (s0, s1, c0, c1))


def linear_u8(img, hd, wd):
    """``cv2.resize(img, (wd, hd), interpolation=cv2.INTER_LINEAR)`` for uint8 ``[hs, ws, C]``, any direction"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3
    hs, ws, _ = img.shape
    x0, x1, a0, a1 = linear_table(ws, wd)
    y0, y1, b0, b1 = linear_table(hs, hd)
    src = img.astype(np.int32)
    rows = src[:, x0] * a0[None, :, None] + src[:, x1] * a1[None, :, None]         # int32 [hs, wd, C]
    r0, r1 = rows[y0], rows[y1]
    out = (((b0[:, None, None] * (r0 >> 4)) >> 16) + ((b1[:, None, None] * (r1 >> 4)) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


def annotator_tail(map_u8, hd, wd):
    """the annotator's last two steps on the network's byte map t (uint8 [h, w, 3]): INTER_LINEAR to (hd, wd), then 255 - map"""
    return 255 - linear_u8(map_u8, hd, wd)
