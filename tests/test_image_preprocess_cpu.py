"""What holds without a GPU for the device image preprocessing (``theatergen_amd/preprocess.py``, ``tg_image_resample_u8``): the numpy restatement of the
two integer passes, driven by ``resample_plan``'s tables, is Pillow byte for byte; the three size rules are the ``transformers`` processors' own; the
lookup table is their ``rescale`` + ``normalize`` bit for bit; the int32 bound holds and is enforced; the symbol is declared, bound and exported."""
import os
import re

import numpy as np
import pytest
import torch

from tests import image_resample_reference as R
from theatergen_amd import preprocess as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("fname", list(R.FILTERS))
@pytest.mark.parametrize("src,dst", R.SHAPES + R.EDGE_SHAPES)
def test_restatement_is_pillow_byte_for_byte(src, dst, fname):
    f = R.FILTERS[fname]
    for img in (R.random_image(src, 11), np.full(src + (3,), 255, np.uint8)):
        got, want = R.resize(img, dst, f), R.pil_resize(img, dst, f)
        assert got.shape == want.shape and got.dtype == np.uint8
        assert int((got != want).sum()) == 0, f"{src} -> {dst} {fname}: {(got != want).sum()} mismatching bytes"


def test_identity_axis_is_one_full_coefficient():
    for f in R.FILTERS.values():
        p = P.resample_plan(37, 37, f)
        i = np.arange(37)
        assert (p.k[i, i - p.first] == 1 << 22).all() and (np.abs(p.k).sum(1) == 1 << 22).all()      # the pixel itself, every other tap 0


def test_plan_is_cached_and_read_only_and_names_other_filters():
    a, b = P.resample_plan(512, 1024, P.BILINEAR), P.resample_plan(512, 1024, P.BILINEAR)
    assert a is b and a.k.dtype == np.int32 and a.first.dtype == np.int32 and a.count.dtype == np.int32 and a.k.shape == (1024, 3)
    with pytest.raises(ValueError):
        a.k[0, 0] = 1
    with pytest.raises(NotImplementedError, match="LANCZOS"):
        P.resample_plan(8, 4, 1)
    with pytest.raises(NotImplementedError, match="NEAREST"):
        P.resample_plan(8, 4, 0)


def _sam_rule(h, w, edge):
    from transformers.models.sam.image_processing_pil_sam import SamImageProcessorPil
    return tuple(SamImageProcessorPil()._get_preprocess_shape((h, w), edge))


def test_size_rules_equal_the_processors_own():
    from transformers.image_transforms import get_resize_output_image_size, get_size_with_aspect_ratio
    from transformers.image_utils import ChannelDimension
    sweep = R.size_sweep()
    ties = [(h, w) for h, w in sweep if (min(h, w) * 1024 / max(h, w)) % 1 == 0.5]
    capped = [(h, w) for h, w in sweep if max(h, w) / min(h, w) * 800 > 1333]
    assert len(ties) >= 8 and len(capped) >= 8 and any(h == w for h, w in sweep) and any(h > w for h, w in sweep) and any(h < w for h, w in sweep)
    for h, w in sweep:
        assert P.longest_edge_size(h, w, 1024) == _sam_rule(h, w, 1024), (h, w)
        assert P.shortest_longest_size(h, w, 800, 1333) == tuple(get_size_with_aspect_ratio((h, w), 800, 1333)), (h, w)
        want = get_resize_output_image_size(np.zeros((3, h, w), np.uint8), size=224, default_to_square=False, input_data_format=ChannelDimension.FIRST)
        assert P.shortest_edge_size(h, w, 224) == tuple(want), (h, w)


def _three_processors():
    from transformers import CLIPImageProcessor, GroundingDinoImageProcessor, SamImageProcessor
    return {"sam": SamImageProcessor(), "grounding_dino": GroundingDinoImageProcessor(), "clip": CLIPImageProcessor()}


@pytest.mark.parametrize("name", ["sam", "grounding_dino", "clip"])
def test_lookup_table_is_rescale_then_normalize_bit_for_bit(name):
    from transformers.image_transforms import normalize, rescale
    from transformers.image_utils import ChannelDimension
    ip = _three_processors()[name]
    bytes_ = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, None, :], (3, 1, 256)).copy()                # CHW, every byte in every channel
    want = normalize(rescale(bytes_, ip.rescale_factor, data_format=ChannelDimension.FIRST, input_data_format=ChannelDimension.FIRST), ip.image_mean,
                     ip.image_std, data_format=ChannelDimension.FIRST, input_data_format=ChannelDimension.FIRST)
    lut = P.normalise_table(ip.do_rescale, ip.rescale_factor, ip.do_normalize, ip.image_mean, ip.image_std)
    assert lut.dtype == np.float32 and lut.shape == (3, 256) and want.dtype == np.float32
    assert np.array_equal(lut.view(np.uint32), want[:, 0, :].view(np.uint32))
    assert np.array_equal(P.DeviceImageProcessor.from_hf(ip, torch.float32, "cpu").lut_host.view(np.uint32), lut.view(np.uint32))


def test_from_hf_reads_the_three_rules_and_names_what_it_cannot_do():
    from transformers import CLIPImageProcessor, SamImageProcessor
    ps = {k: P.DeviceImageProcessor.from_hf(v, torch.bfloat16, "cpu") for k, v in _three_processors().items()}
    assert (ps["sam"].rule, ps["sam"].size, ps["sam"].pad, ps["sam"].resample) == ("longest_edge", (1024,), (1024, 1024), P.BILINEAR)
    assert (ps["grounding_dino"].rule, ps["grounding_dino"].size, ps["grounding_dino"].pad, ps["grounding_dino"].do_pad) == ("shortest_longest", (800, 1333), None, True)
    assert (ps["clip"].rule, ps["clip"].size, ps["clip"].crop, ps["clip"].resample, ps["clip"].do_pad) == ("shortest_edge", (224,), (224, 224), P.BICUBIC, False)
    assert ps["sam"].window(200, 232) == ((883, 1024), (0, 0), (883, 1024))
    assert ps["grounding_dino"].window(200, 232) == ((800, 928), (0, 0), (800, 928))
    assert ps["clip"].window(512, 768) == ((224, 336), (0, 56), (224, 224))
    with pytest.raises(NotImplementedError, match="size"):
        P.DeviceImageProcessor.from_hf(CLIPImageProcessor(size={"height": 32, "width": 32}), torch.float32, "cpu")
    with pytest.raises(NotImplementedError, match="do_center_crop"):
        P.DeviceImageProcessor.from_hf(CLIPImageProcessor(do_center_crop=False), torch.float32, "cpu")
    with pytest.raises(NotImplementedError, match="do_resize"):
        P.DeviceImageProcessor.from_hf(SamImageProcessor(do_resize=False), torch.float32, "cpu")
    with pytest.raises(NotImplementedError, match="LANCZOS"):
        P.DeviceImageProcessor.from_hf(SamImageProcessor(resample=1), torch.float32, "cpu")


def test_int32_bound_holds_over_the_sweep_and_a_broken_table_is_refused():
    worst = 0
    pairs = [(s[0], d[0]) for s, d in R.SHAPES + R.EDGE_SHAPES] + [(s[1], d[1]) for s, d in R.SHAPES + R.EDGE_SHAPES]
    pairs += [(h, P.longest_edge_size(h, w, 1024)[0]) for h, w in R.size_sweep()] + [(8192, 1), (1, 8192), (8192, 224), (4000, 7)]
    for n_in, n_out in pairs:
        for f in R.FILTERS.values():
            p = P.resample_plan(n_in, n_out, f)
            worst = max(worst, P.check_plan_bound(p.k))
            assert (p.first >= 0).all() and (p.count >= 1).all() and (p.first + p.count <= n_in).all() and (p.count <= p.k.shape[1]).all()
            assert (np.diff(p.first) >= 0).all() and (np.diff(p.first + p.count) >= 0).all()          # what the fused tile's row range relies on
    assert 255 * worst + (1 << 21) < 1 << 31
    bad = np.full((2, 3), 1 << 22, np.int32)
    bad[1] = [1 << 23, -(1 << 22), 1 << 22]                                                               # sum |k| = 2^24: 255 * 2^24 > 2^31
    with pytest.raises(ValueError, match="int32"):
        P.check_plan_bound(bad)
    P.check_plan_bound(np.full((2, 1), 1 << 22, np.int32))


def test_route_decision_matches_the_lds_budget():
    from theatergen_amd import _lib
    header = open(os.path.join(ROOT, "include", "theatergen_hip.h")).read()
    for name, val in (("TILE_H", _lib.RESAMPLE_TILE_H), ("TILE_W", _lib.RESAMPLE_TILE_W), ("LDS_BYTES", _lib.RESAMPLE_LDS_BYTES), ("MAX_SIZE", _lib.RESAMPLE_MAX_SIZE)):
        assert re.search(rf"#define TG_RESAMPLE_{name} {val}\b", header), name
    for (n_in, n_out, f), want in (((512, 1024, P.BILINEAR), "fused"), ((512, 800, P.BILINEAR), "fused"), ((512, 224, P.BICUBIC), "fused"),
                                   ((97, 40, P.BICUBIC), "fused"), ((300, 77, P.BILINEAR), "two_launch"), ((300, 77, P.BICUBIC), "two_launch")):
        route, rows = P.resample_route(P.resample_plan(n_in, n_out, f), 0, n_out)
        assert route == want, (n_in, n_out, rows)
        assert (rows * _lib.RESAMPLE_TILE_W * 3 <= _lib.RESAMPLE_LDS_BYTES) == (route == "fused")


def test_resample_symbol_declared_bound_and_exported_at_abi_308():
    from theatergen_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "theatergen_hip.h")).read()
    assert re.search(r"#define TG_ABI_VERSION 308\b", header) and _lib.ABI_VERSION == 308, "additive symbols keep the version"
    m = re.search(r"^int\s+tg_image_resample_u8\s*\(([^;]*)\);", header, flags=re.M)
    assert m, "tg_image_resample_u8 is not declared in include/theatergen_hip.h"
    assert len(m.group(1).split(",")) == 27 == len(_lib.SIGNATURES["tg_image_resample_u8"][1])
    assert os.path.exists(os.path.join(ROOT, "theatergen_amd", "csrc", "tg_image_resample.hip"))
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    h = _lib.lib()
    assert h.tg_version() == 308 and h.tg_image_resample_u8 is not None


def test_resample_kernels_are_gated_at_zero_scratch():
    from theatergen_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    for sub in ("image_resample_fused_kernel<", "image_resample_h_kernel", "image_resample_v_kernel<"):
        gates = [g for g in build.HOT_GATES if g[0] == sub]
        assert len(gates) == 1 and gates[0][1] == 0, f"HOT_GATES entry for {sub}: {gates}"
    res = build.kernel_resources(verbose=False)
    mine = {k: v for k, v in res.items() if v["file"] == "tg_image_resample.hip"}
    assert len(mine) == 7, sorted(mine)                   # fused x 3 dtypes, horizontal, vertical x 3 dtypes
    for name, r in mine.items():
        assert r.get("scratch", 0) == 0, f"{name}: scratch {r.get('scratch')} bytes / lane"
    assert not build.check_resources(res)


def _call(h, **kw):
    a = dict(src=256, batch=1, hs=4, ws=4, kv=512, fv=768, cv=1024, ksv=3, rh=8, kh=1280, fh=1536, ch=1792, ksh=3, rw=8, oy=0, ox=0, oh=8, ow=8, lut=2048,
             dst=4096, dt=0, hp=8, wp=8, u8=None, rows=8, tmp=None)
    a.update(kw)
    return h.tg_image_resample_u8(a["src"], a["batch"], a["hs"], a["ws"], a["kv"], a["fv"], a["cv"], a["ksv"], a["rh"], a["kh"], a["fh"], a["ch"], a["ksh"],
                                  a["rw"], a["oy"], a["ox"], a["oh"], a["ow"], a["lut"], a["dst"], a["dt"], a["hp"], a["wp"], a["u8"], a["rows"], a["tmp"], None)


REFUSALS = ([{k: None} for k in ("src", "dst", "lut", "kv", "fv", "cv", "kh", "fh", "ch")] +
            [{k: v} for k in ("batch", "hs", "ws", "rh", "rw", "hp", "wp") for v in (0, 8193)] + [dict(oh=0), dict(ow=0), dict(ksv=0), dict(ksh=0),
             dict(oy=1), dict(ox=1), dict(oy=-1), dict(ox=-1, ow=4), dict(oh=9, hp=9), dict(hp=7), dict(wp=7), dict(dt=3), dict(dt=-1), dict(dst=256),
             dict(u8=256), dict(u8=4096), dict(tmp=4096), dict(rows=0), dict(rows=54)])


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """fake non-null pointers, never dereferenced: validation is on the host side of the ABI"""
    from theatergen_amd import _lib
    h = _lib.lib()
    for bad in REFUSALS:
        assert _call(h, **bad) == -1, bad
        assert b"tg_image_resample_u8" in h.tg_last_error(), bad


def test_ops_wrapper_refuses_host_tensors():
    from theatergen_amd import ops
    with pytest.raises(RuntimeError, match="GPU"):
        ops.image_resample_u8(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), None, None, None, torch.float32)
