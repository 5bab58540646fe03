"""Host plans of the annotator's two cv2 resizes (csrc/tg_cv_resize.hip: ``ops.cv_area_u8`` / ``ops.cv_linear_u8``): the per-axis tables of OpenCV's portable
C++ path (modules/imgproc/src/resize.cpp: ``computeResizeAreaTab`` and the INTER_LINEAR branch of ``resize``), made in float64 / integers, cached per
``(ssize, dsize)`` and, on a device, per ``(ssize, dsize, device)``.  Written from that source, not run against a cv2 build; the arithmetic the tables feed is
stated with the entry points in include/theatergen_hip.h, and tests/cv_resize_reference.py restates both in NumPy."""
import collections
import functools
import math

import numpy as np
import torch

from . import _lib

AreaPlan = collections.namedtuple("AreaPlan", "first count alpha in_size out_size integer iscale")
LinearPlan = collections.namedtuple("LinearPlan", "table in_size out_size")

_EPS = float(np.finfo(np.float64).eps)                 # DBL_EPSILON


def _sizes(ssize, dsize, who):
    ssize, dsize = int(ssize), int(dsize)
    if not (1 <= ssize <= _lib.CV_RESIZE_MAX_SIZE and 1 <= dsize <= _lib.CV_RESIZE_MAX_SIZE):
        raise ValueError(f"{who}: sizes must be in 1 .. {_lib.CV_RESIZE_MAX_SIZE}, got {ssize} -> {dsize}")
    return ssize, dsize


@functools.lru_cache(maxsize=256)
def area_plan(ssize, dsize):
    """INTER_AREA on one axis, ``ssize`` -> ``dsize <= ssize`` pixels: ``AreaPlan(first int32 [dsize], count int32 [dsize], alpha float32 [dsize, ksize])``:
    destination ``d`` has ``count[d]`` entries on consecutive source indices from ``first[d]``.  ``integer`` / ``iscale``: OpenCV's test for its block-sum
    path (which needs it on both axes and then does not read the tables).  More than ``CV_AREA_MAX_TAPS`` entries: NotImplementedError."""
    ssize, dsize = _sizes(ssize, dsize, "area_plan")
    if dsize > ssize:
        raise NotImplementedError(f"area_plan: {ssize} -> {dsize} grows the axis; INTER_AREA is built for shrinking or equal axes only")
    scale = ssize / dsize
    iscale = int(scale)
    rows = []
    for d in range(dsize):
        f1 = d * scale
        f2 = f1 + scale
        cell = min(scale, ssize - f1)
        s1, s2 = math.ceil(f1), min(math.floor(f2), ssize - 1)
        s1 = min(s1, s2)
        first, w = s1, []
        if s1 - f1 > 1e-3:
            first = s1 - 1
            w.append((s1 - f1) / cell)
        w.extend([1.0 / cell] * (s2 - s1))
        if f2 - s2 > 1e-3:
            w.append(min(min(f2 - s2, 1.0), cell) / cell)
        rows.append((first, w))
    ksize = max(len(w) for _, w in rows)
    if ksize > _lib.CV_AREA_MAX_TAPS:
        raise NotImplementedError(f"area_plan: {ssize} -> {dsize} needs {ksize} source pixels per destination pixel on this axis; the kernel holds "
                                  f"{_lib.CV_AREA_MAX_TAPS} (integer ratios on both axes take the block-sum path and have no such limit)")
    first = np.array([f for f, _ in rows], dtype=np.int32)
    count = np.array([len(w) for _, w in rows], dtype=np.int32)
    alpha = np.zeros((dsize, ksize), dtype=np.float32)
    for d, (_, w) in enumerate(rows):
        alpha[d, :len(w)] = np.asarray(w, dtype=np.float64).astype(np.float32)
    for a in (first, count, alpha):
        a.setflags(write=False)
    return AreaPlan(first, count, alpha, ssize, dsize, abs(scale - iscale) < _EPS, iscale)


def area_is_integer(ssize, dsize):
    """OpenCV's per-axis test ``|scale - int(scale)| < DBL_EPSILON`` without building tables (an integer ratio may exceed the entry limit of ``area_plan``)"""
    ssize, dsize = _sizes(ssize, dsize, "area_is_integer")
    scale = ssize / dsize
    return abs(scale - int(scale)) < _EPS


def area_stage_rows(plan, tile_h=_lib.CV_AREA_TILE_H):
    """the largest number of source rows the entries of ``tile_h`` consecutive destination rows (one tile of the kernel) span"""
    first, end = plan.first.astype(np.int64), plan.first.astype(np.int64) + plan.count
    y0 = np.arange(0, plan.out_size, tile_h)
    y1 = np.minimum(y0 + tile_h, plan.out_size) - 1
    return int((end[y1] - first[y0]).max())


@functools.lru_cache(maxsize=256)
def linear_plan(ssize, dsize):
    """INTER_LINEAR on one axis, any direction: ``LinearPlan(table int32 [dsize, 4])`` with rows ``(s0, s1, c0, c1)``: the two source indices and their
    11-bit fixed-point coefficients (``INTER_RESIZE_COEF_SCALE`` = 2048, rounded half to even, saturated to int16)"""
    ssize, dsize = _sizes(ssize, dsize, "linear_plan")
    scale = ssize / dsize
    d = np.arange(dsize, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(np.float32)                                                   # fp32
    low, high = s < 0, s >= ssize - 1
    s = np.where(low, 0, np.where(high, ssize - 1, s))
    f = np.where(low | high, np.float32(0), f).astype(np.float32)
    c0 = np.clip(np.rint((np.float32(1) - f) * np.float32(2048)), -32768, 32767)
    c1 = np.clip(np.rint(f * np.float32(2048)), -32768, 32767)
    table = np.stack([s, np.minimum(s + 1, ssize - 1), c0.astype(np.int64), c1.astype(np.int64)], axis=1).astype(np.int32)
    table.setflags(write=False)
    return LinearPlan(table, ssize, dsize)


_device_plans = {}


def _cached(key, make):
    hit = _device_plans.get(key)
    if hit is None:
        if len(_device_plans) >= 256:
            _device_plans.clear()
        hit = _device_plans[key] = make()
    return hit


def device_area_plan(ssize, dsize, device):
    """``area_plan`` with its tables on ``device`` as well: ``(plan, first, count, alpha)``, cached per key and device"""
    device = torch.device(device)
    def make():
        plan = area_plan(int(ssize), int(dsize))
        return (plan,) + tuple(torch.from_numpy(a.copy()).to(device) for a in plan[:3])                  # the cached arrays are read-only
    return _cached(("area", int(ssize), int(dsize), device.type, device.index), make)


def device_linear_plan(ssize, dsize, device):
    """``linear_plan`` with its table on ``device`` as well: ``(plan, table)``, cached per key and device"""
    device = torch.device(device)
    def make():
        plan = linear_plan(int(ssize), int(dsize))
        return plan, torch.from_numpy(plan.table.copy()).to(device)
    return _cached(("linear", int(ssize), int(dsize), device.type, device.index), make)
