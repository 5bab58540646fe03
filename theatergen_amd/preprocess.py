"""Image preprocessing on the device: drop-in replacements for the ``transformers`` image processors that feed SAM, GroundingDINO and CLIP.

A processor call is: PIL resize of a uint8 RGB image, ``* rescale_factor``, ``(x - mean) / std``, zero padding at the bottom and right, CHW.  All of it is
one launch of ``tg_image_resample_u8`` (``ops.image_resample_u8``) on the uint8 image, writing ``pixel_values`` in the storage dtype — bit-equal to
``hf_processor(...)["pixel_values"].to(dtype)``:

* ``resample_plan``: Pillow's 8-bit resampling is integer arithmetic once its coefficients exist; the tables are made here, in float64, exactly as Pillow's
  ``precompute_coeffs`` / ``normalize_coeffs_8bpc`` make them (``src/libImaging/Resample.c``).
* ``normalise_table``: rescale + normalise depend on the byte and the channel only; the ``[3][256]`` fp32 table is made with the numpy expressions of
  ``transformers.image_transforms.rescale`` / ``normalize``.
* the size rules of the three processors are restated (``longest_edge_size``, ``shortest_longest_size``, ``shortest_edge_size``).

Everything is opt-in: ``DeviceSamProcessor`` goes where ``sam_model_dict["sam_processor"]`` goes, ``DeviceGroundingDinoProcessor`` where
``grounding_dino_model["processor"]`` goes, ``DeviceImageProcessor.from_hf(CLIPImageProcessor(), ...)`` where ``IPAdapter.clip_image_processor`` goes.
"""
import functools
from collections import namedtuple

import numpy as np
import torch

from . import _lib

BILINEAR, BICUBIC = 2, 3                              # PIL.Image.Resampling values
_FILTER_NAMES = {0: "NEAREST", 1: "LANCZOS", 2: "BILINEAR", 3: "BICUBIC", 4: "BOX", 5: "HAMMING"}
PRECISION_BITS = 22                                   # 32 - 8 - 2, Pillow's PRECISION_BITS

ResamplePlan = namedtuple("ResamplePlan", "k first count in_size out_size")      # k int32 [out, ksize], first / count int32 [out]


def _bilinear(x):
    x = np.abs(x)
    return np.where(x < 1.0, 1.0 - x, 0.0)


def _bicubic(x):
    a = -0.5
    x = np.abs(x)
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


_FILTERS = {BILINEAR: (1.0, _bilinear), BICUBIC: (2.0, _bicubic)}


def check_plan_bound(k):
    """int32 accumulation is exact when ``255 * sum |k| + 2^21 < 2^31`` for every output index: refuse a table that breaks it"""
    k = np.asarray(k)
    worst = int(np.abs(k.astype(np.int64)).sum(axis=-1).max()) if k.size else 0
    if 255 * worst + (1 << (PRECISION_BITS - 1)) >= 1 << 31:
        raise ValueError(f"resample plan: 255 * sum |k| + 2^21 = {255 * worst + (1 << (PRECISION_BITS - 1))} does not fit int32")
    return worst


@functools.lru_cache(maxsize=256)
def resample_plan(in_size, out_size, filter):
    """Pillow's coefficient tables for one axis, ``in_size`` -> ``out_size`` pixels: ``ResamplePlan(k int32 [out, ksize], first int32 [out],
    count int32 [out])``; output ``i`` is ``clip8((2^21 + sum_t p[first[i] + t] * k[i, t]) >> 22)``.  float64 throughout, in Pillow's order of operations
    (the weight sum runs tap by tap).  The arrays are cached and read-only."""
    filter = int(filter)
    if filter not in _FILTERS:
        raise NotImplementedError(f"resample_plan: filter {_FILTER_NAMES.get(filter, filter)} ({filter}) is not implemented (BILINEAR = 2, BICUBIC = 3)")
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError(f"resample_plan: sizes must be >= 1, got {in_size} -> {out_size}")
    support0, fn = _FILTERS[filter]
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = support0 * fs
    ksize = int(np.ceil(support)) * 2 + 1
    centre = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    first = np.maximum((centre - support + 0.5).astype(np.int64), 0)              # a C cast: truncation towards zero
    last = np.minimum((centre + support + 0.5).astype(np.int64), in_size)
    count = last - first
    ss = 1.0 / fs
    t = np.arange(ksize, dtype=np.int64)[None, :]
    w = fn((t + first[:, None] - centre[:, None] + 0.5) * ss)
    w = np.where(t < count[:, None], w, 0.0)
    ww = np.zeros(out_size, np.float64)
    for j in range(ksize):                                                          # Pillow adds the weights one tap at a time
        ww = ww + w[:, j]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    scaled = w * float(1 << PRECISION_BITS)
    k = np.where(w < 0, (-0.5 + scaled), (0.5 + scaled)).astype(np.int64)        # truncation towards zero again
    k = np.where(t < count[:, None], k, 0).astype(np.int32)
    check_plan_bound(k)
    plan = ResamplePlan(k, first.astype(np.int32), count.astype(np.int32), in_size, out_size)
    for a in plan[:3]:
        a.setflags(write=False)
    return plan


_device_plans = {}


def device_plan(in_size, out_size, filter, device):
    """``resample_plan`` with its tables on ``device`` as well: ``(plan, k, first, count)``, cached per key and device"""
    device = torch.device(device)
    key = (int(in_size), int(out_size), int(filter), device.type, device.index)
    hit = _device_plans.get(key)
    if hit is None:
        plan = resample_plan(int(in_size), int(out_size), int(filter))
        if len(_device_plans) >= 256:
            _device_plans.clear()
        hit = _device_plans[key] = (plan,) + tuple(torch.from_numpy(a.copy()).to(device) for a in plan[:3])    # the cached arrays are read-only
    return hit


def stage_rows(plan_v, oy, oh, tile_h=_lib.RESAMPLE_TILE_H):
    """the largest number of source rows a ``tile_h``-row tile of window rows ``oy .. oy + oh`` reaches with its vertical taps"""
    first, end = plan_v.first.astype(np.int64), plan_v.first.astype(np.int64) + plan_v.count
    y0 = np.arange(0, oh, tile_h)
    y1 = np.minimum(y0 + tile_h, oh) - 1
    return int((end[oy + y1] - first[oy + y0]).max())


def resample_route(plan_v, oy, oh):
    """``("fused" | "two_launch", stage_rows)``: the fused kernel stages its rows in LDS; a tile whose rows do not fit takes two launches"""
    rows = stage_rows(plan_v, oy, oh)
    fits = rows * _lib.RESAMPLE_TILE_W * 3 <= _lib.RESAMPLE_LDS_BYTES
    return ("fused" if fits else "two_launch"), rows


def normalise_table(do_rescale, rescale_factor, do_normalize, image_mean, image_std):
    """fp32 ``[3, 256]``: what ``transformers.image_transforms.rescale`` then ``normalize`` make of every byte, per channel, with their own expressions:
    ``float32(float64(u) * rescale_factor)``, then ``(v - float32(mean)) / float32(std)`` in fp32"""
    u = np.arange(256, dtype=np.uint8)
    v = (u.astype(np.float64) * rescale_factor).astype(np.float32) if do_rescale else u.astype(np.float32)
    lut = np.repeat(v[None], 3, 0)
    if do_normalize:
        mean = np.array(_per_channel(image_mean, "image_mean"), dtype=np.float32)
        std = np.array(_per_channel(image_std, "image_std"), dtype=np.float32)
        lut = ((lut.T - mean) / std).T
    return np.ascontiguousarray(lut, dtype=np.float32)


def _per_channel(x, name):
    x = list(x) if isinstance(x, (list, tuple, np.ndarray)) else [x] * 3
    if len(x) != 3:
        raise ValueError(f"DeviceImageProcessor: {name} must have 3 entries, got {len(x)}")
    return [float(v) for v in x]


# ---- the processors' size rules, restated ------------------------------------------------------------------------------------------------------
def longest_edge_size(h, w, longest_edge):
    """SAM (``SamImageProcessor._get_preprocess_shape``)"""
    scale = longest_edge * 1.0 / max(h, w)
    return int(h * scale + 0.5), int(w * scale + 0.5)


def shortest_longest_size(h, w, size, max_size):
    """GroundingDINO (``image_transforms.get_size_with_aspect_ratio``): shortest edge ``size`` unless the longest would pass ``max_size``"""
    raw = None
    if max_size is not None:
        lo, hi = float(min(h, w)), float(max(h, w))
        if hi / lo * size > max_size:
            raw = max_size * lo / hi
            size = int(round(raw))
    if (h <= w and h == size) or (w <= h and w == size):
        return h, w
    if w < h:
        return (int(raw * h / w) if raw is not None else int(size * h / w)), size
    return size, (int(raw * w / h) if raw is not None else int(size * w / h))


def shortest_edge_size(h, w, size):
    """CLIP (``image_transforms.get_resize_output_image_size`` with ``default_to_square=False``)"""
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = size, int(size * long / short)
    return (new_long, new_short) if w <= h else (new_short, new_long)


def _field(d, key):
    """a size field of a ``SizeDict`` / dict / None"""
    if d is None:
        return None
    v = d.get(key) if hasattr(d, "get") else getattr(d, key, None)
    return None if v is None else int(v)


def _to_u8(image, device):
    """one caller's image -> uint8 [B, H, W, 3] on ``device`` (host images cross the bus as uint8)"""
    if isinstance(image, torch.Tensor):
        t = image
    elif isinstance(image, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(image))
    elif hasattr(image, "convert") and hasattr(image, "size"):                   # PIL: what the processor's do_convert_rgb does
        t = torch.from_numpy(np.array(image if image.mode == "RGB" else image.convert("RGB")))
    else:
        raise TypeError(f"DeviceImageProcessor: PIL image, uint8 HWC ndarray or uint8 tensor expected, got {type(image).__name__}")
    if t.dtype != torch.uint8 or t.dim() not in (3, 4) or t.shape[-1] != 3:
        raise ValueError(f"DeviceImageProcessor: uint8 [H, W, 3] / [B, H, W, 3] expected, got {t.dtype} {tuple(t.shape)}")
    if t.dim() == 3:
        t = t[None]
    return t.to(device).contiguous()


class DeviceImageProcessor:
    """The image side of a ``transformers`` processor on the device.  ``from_hf`` reads the processor's own fields; ``__call__`` returns what it returns:
    ``pixel_values`` (on the device, in ``dtype``), and ``original_sizes`` / ``reshaped_input_sizes`` (SAM) or ``pixel_mask`` (GroundingDINO) as CPU int64."""

    def __init__(self, rule, size, resample, lut, dtype, device, crop=None, pad=None, do_pad=False):
        self.rule, self.size, self.resample, self.crop, self.pad, self.do_pad = rule, size, int(resample), crop, pad, bool(do_pad)
        self.dtype, self.device = dtype, torch.device(device)
        if dtype not in (torch.bfloat16, torch.float16, torch.float32):
            raise ValueError(f"DeviceImageProcessor: dtype bf16 / fp16 / fp32, not {dtype}")
        if self.resample not in _FILTERS:
            raise NotImplementedError(f"DeviceImageProcessor: resample {_FILTER_NAMES.get(self.resample, self.resample)} is not implemented "
                                      "(BILINEAR = 2, BICUBIC = 3)")
        self.lut_host = np.ascontiguousarray(lut, dtype=np.float32)
        self._lut = None

    @classmethod
    def from_hf(cls, image_processor, dtype, device):
        g = lambda name, default=None: getattr(image_processor, name, default)      # noqa: E731
        if not g("do_resize", True):
            raise NotImplementedError("DeviceImageProcessor: do_resize=False is outside the three size rules")
        if not g("do_rescale", True) and not g("do_normalize", True):
            raise NotImplementedError("DeviceImageProcessor: do_rescale=False with do_normalize=False leaves uint8 pixel_values; nothing to compute")
        size = g("size")
        short, long_, hh, ww = (_field(size, k) for k in ("shortest_edge", "longest_edge", "height", "width"))
        crop = None
        if g("do_center_crop", False):
            crop = (_field(g("crop_size"), "height"), _field(g("crop_size"), "width"))
            if crop[0] is None or crop[1] is None:
                raise NotImplementedError(f"DeviceImageProcessor: crop_size {g('crop_size')} must have height and width")
        if short and long_:
            rule, sz = "shortest_longest", (short, long_)
        elif long_:
            rule, sz = "longest_edge", (long_,)
        elif short:
            rule, sz = "shortest_edge", (short,)
            if crop is None:
                raise NotImplementedError("DeviceImageProcessor: size with shortest_edge alone needs do_center_crop (the CLIP rule)")
        else:
            raise NotImplementedError(f"DeviceImageProcessor: size {dict(size) if size is not None else None} is none of longest_edge (SAM), "
                                      "shortest_edge + longest_edge (GroundingDINO), shortest_edge + centre crop (CLIP)")
        if crop is not None and rule != "shortest_edge":
            raise NotImplementedError(f"DeviceImageProcessor: do_center_crop with size {dict(size)} is outside the three size rules")
        do_pad = bool(g("do_pad", False))
        pad = None
        if do_pad and g("pad_size") is not None:
            pad = (_field(g("pad_size"), "height"), _field(g("pad_size"), "width"))
            if pad[0] is None or pad[1] is None:
                raise NotImplementedError(f"DeviceImageProcessor: pad_size {g('pad_size')} must have height and width")
        if do_pad and pad is None and rule == "longest_edge":
            raise NotImplementedError("DeviceImageProcessor: do_pad with the longest_edge rule needs pad_size")
        resample = g("resample", BILINEAR)
        lut = normalise_table(g("do_rescale", True), g("rescale_factor", 1 / 255), g("do_normalize", True), g("image_mean"), g("image_std"))
        return cls(rule, sz, BILINEAR if resample is None else int(resample), lut, dtype, device, crop=crop, pad=pad, do_pad=do_pad)

    def resized_size(self, h, w):
        if self.rule == "longest_edge":
            return longest_edge_size(h, w, self.size[0])
        if self.rule == "shortest_longest":
            return shortest_longest_size(h, w, self.size[0], self.size[1])
        return shortest_edge_size(h, w, self.size[0])

    def window(self, h, w):
        """(resized (rh, rw), window origin (oy, ox), window size (oh, ow)) for an h x w image"""
        rh, rw = self.resized_size(h, w)
        if self.crop is None:
            return (rh, rw), (0, 0), (rh, rw)
        ch, cw = self.crop
        oy, ox = (rh - ch) // 2, (rw - cw) // 2
        if oy < 0 or ox < 0:
            raise NotImplementedError(f"DeviceImageProcessor: crop_size {self.crop} larger than the resized image {(rh, rw)} (the processor would pad around it)")
        return (rh, rw), (oy, ox), (ch, cw)

    def lut(self):
        if self._lut is None:
            self._lut = torch.from_numpy(self.lut_host).to(self.device)
        return self._lut

    def __call__(self, images=None, return_tensors="pt", **kwargs):
        from transformers import BatchFeature
        from . import ops
        if images is None:
            raise ValueError("DeviceImageProcessor: images is required")
        if kwargs:
            raise NotImplementedError(f"DeviceImageProcessor: per-call overrides are not supported: {sorted(kwargs)}")
        if return_tensors not in ("pt", None):
            raise NotImplementedError(f"DeviceImageProcessor: return_tensors={return_tensors!r} (pixel_values are torch tensors on the device)")
        items = list(images) if isinstance(images, (list, tuple)) else [images]
        batches = [_to_u8(im, self.device) for im in items]
        orig, wins = [], []
        for t in batches:
            n, h, w = int(t.shape[0]), int(t.shape[1]), int(t.shape[2])
            orig += [(h, w)] * n
            wins += [self.window(h, w)] * n
        if self.pad is not None:
            canvas = self.pad
        else:
            canvas = (max(wn[2][0] for wn in wins), max(wn[2][1] for wn in wins))
            if not self.do_pad and any(wn[2] != canvas for wn in wins):
                raise ValueError("DeviceImageProcessor: images of different output sizes need do_pad")
        if any(wn[2][0] > canvas[0] or wn[2][1] > canvas[1] for wn in wins):
            raise ValueError(f"DeviceImageProcessor: pad_size {canvas} is smaller than a resized image")
        B = len(orig)
        out = torch.empty((B, 3) + tuple(canvas), dtype=self.dtype, device=self.device)
        # images of one size go in one launch: consecutive runs keep the caller's order and write adjacent rows of the batch
        groups, b = {}, 0
        for t in batches:
            groups.setdefault(tuple(t.shape[1:3]), []).append((b, t))
            b += int(t.shape[0])
        for (h, w), members in groups.items():
            (rh, rw), (oy, ox), (oh, ow) = self.window(h, w)
            pv = device_plan(h, rh, self.resample, self.device)
            ph = device_plan(w, rw, self.resample, self.device)
            runs = []
            for at, t in members:                                                  # adjacent members become one launch
                if runs and runs[-1][0] + sum(int(x.shape[0]) for x in runs[-1][1]) == at:
                    runs[-1][1].append(t)
                else:
                    runs.append((at, [t]))
            for at, ts in runs:
                src = ts[0] if len(ts) == 1 else torch.cat(ts)
                ops.image_resample_u8(src, pv, ph, self.lut(), self.dtype, window=(oy, ox, oh, ow), out=out[at:at + src.shape[0]])
        data = {"pixel_values": out}
        if self.rule == "longest_edge":
            data["original_sizes"] = torch.tensor(orig, dtype=torch.int64)
            data["reshaped_input_sizes"] = torch.tensor([wn[0] for wn in wins], dtype=torch.int64)
        elif self.rule == "shortest_longest" and self.do_pad:
            mask = torch.zeros((B,) + tuple(canvas), dtype=torch.int64)
            for i, wn in enumerate(wins):
                mask[i, :wn[2][0], :wn[2][1]] = 1
            data["pixel_mask"] = mask
        return BatchFeature(data=data)

    preprocess = __call__


class DeviceSamProcessor:
    """Goes where ``sam_model_dict["sam_processor"]`` goes.  Images take the device route; prompts, when given, are normalised by the caller's processor's
    own code (``SamProcessor._check_and_preprocess_points`` / ``_normalize_and_convert``) on the host.  ``.image_processor`` stays the caller's, for
    ``post_process_masks`` on the ``transformers`` route."""

    def __init__(self, hf_processor, dtype, device):
        self.hf = hf_processor
        self.image_processor = getattr(hf_processor, "image_processor", hf_processor)
        self.device_image_processor = DeviceImageProcessor.from_hf(self.image_processor, dtype, device)
        if self.device_image_processor.rule != "longest_edge":
            raise NotImplementedError(f"DeviceSamProcessor: size {self.image_processor.size} is not SAM's longest_edge rule")

    def __call__(self, images=None, input_points=None, input_labels=None, input_boxes=None, return_tensors="pt", point_pad_value=-10, **kwargs):
        enc = self.device_image_processor(images, return_tensors=return_tensors, **kwargs)
        if input_points is None and input_labels is None and input_boxes is None:
            return enc
        if not (hasattr(self.hf, "_check_and_preprocess_points") and hasattr(self.hf, "_normalize_and_convert")):
            raise NotImplementedError("DeviceSamProcessor: prompts need the caller's SamProcessor (its _check_and_preprocess_points / _normalize_and_convert)")
        input_points, input_labels, input_boxes = self.hf._check_and_preprocess_points(input_points=input_points, input_labels=input_labels,
                                                                                       input_boxes=input_boxes)
        return self.hf._normalize_and_convert(enc, enc["original_sizes"].numpy(), input_points=input_points, input_labels=input_labels,
                                              input_boxes=input_boxes, return_tensors=return_tensors, point_pad_value=point_pad_value)

    def post_process_masks(self, *args, **kwargs):
        return self.image_processor.post_process_masks(*args, **kwargs)


class DeviceGroundingDinoProcessor:
    """Goes where ``grounding_dino_model["processor"]`` goes.  The caller's tokenizer runs on the host and its tensors stay on the CPU (the detector's
    caption cache keys on ``input_ids``); the image side runs on the device."""

    def __init__(self, hf_processor, dtype, device):
        self.hf = hf_processor
        self.image_processor, self.tokenizer = hf_processor.image_processor, hf_processor.tokenizer
        self.device_image_processor = DeviceImageProcessor.from_hf(self.image_processor, dtype, device)
        if self.device_image_processor.rule != "shortest_longest":
            raise NotImplementedError(f"DeviceGroundingDinoProcessor: size {self.image_processor.size} is not the shortest_edge + longest_edge rule")

    def __call__(self, images=None, text=None, return_tensors="pt", **text_kwargs):
        from transformers import BatchFeature
        data = {}
        if images is not None:
            data.update(self.device_image_processor(images, return_tensors=return_tensors))
        if text is not None:
            if hasattr(self.hf, "_preprocess_input_text"):
                text = self.hf._preprocess_input_text(text)
            text_kwargs.setdefault("return_token_type_ids", True)
            data.update(self.tokenizer(text, return_tensors=return_tensors, **text_kwargs))
        return BatchFeature(data=data)

    def __getattr__(self, name):                                                   # post_process_grounded_object_detection and the like
        return getattr(self.__dict__["hf"], name)
