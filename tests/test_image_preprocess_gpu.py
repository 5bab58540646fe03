"""``tg_image_resample_u8`` and the device processors on the GPU: the resized bytes are Pillow's, ``pixel_values`` are the ``transformers`` processors' bit
for bit in every storage dtype with +0 padding, every refusal leaves the destination alone, and the SAM / GroundingDINO call surfaces return the same
results with a device processor as with the host processor (bit-equal inputs leave no room for a tolerance)."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import image_resample_reference as R
from theatergen_amd import preprocess as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
LUT = P.normalise_table(True, 1 / 255, True, [0.485, 0.456, 0.406], [0.229, 0.224, 0.225])

# (source (h, w), resized (h, w)): integer upscale; non-integer upscale over many tiles with ragged last tiles; downscale, ragged in both axes; identity
# vertical pass; identity horizontal pass; the two-launch route; clamping at both borders
BYTE_SHAPES = [((64, 64), (128, 128)), ((200, 232), (800, 928)), ((97, 131), (40, 53)), ((37, 61), (37, 200)), ((61, 37), (200, 37)), ((300, 50), (77, 13)),
               ((1, 1), (5, 3)), ((5, 3), (1, 1))]


def _run(imgs, dst_hw, filter, dtype=torch.float32, window=None, pad=None, route=None):
    """imgs uint8 [B, h, w, 3] numpy -> (pixel_values, resized bytes) as host tensors / arrays"""
    from theatergen_amd import ops
    src = torch.from_numpy(imgs).to(DEV)
    pv = P.device_plan(imgs.shape[1], dst_hw[0], filter, src.device)
    ph = P.device_plan(imgs.shape[2], dst_hw[1], filter, src.device)
    out, u8 = ops.image_resample_u8(src, pv, ph, torch.from_numpy(LUT).to(DEV), dtype, window=window, pad=pad, u8_out=True, route=route)
    return out.cpu(), u8.cpu().numpy()


@pytest.mark.parametrize("fname", list(R.FILTERS))
@pytest.mark.parametrize("src,dst", BYTE_SHAPES)
def test_resized_bytes_are_pillows(src, dst, fname):
    from theatergen_amd import ops
    f = R.FILTERS[fname]
    planned, rows = P.resample_route(P.resample_plan(src[0], dst[0], f), 0, dst[0])
    assert (planned == "two_launch") == (src == (300, 50)), f"{src} -> {dst}: {planned} ({rows} staged rows)"
    for img in (R.random_image(src, 21), np.full(src + (3,), 255, np.uint8)):
        before = dict(ops.resample_launches)
        out, u8 = _run(img[None], dst, f)
        assert ops.resample_launches[planned] == before[planned] + 1, "the planned route did not run"
        want = R.pil_resize(img, dst, f)
        assert u8.shape == (1,) + want.shape and int((u8[0] != want).sum()) == 0, f"{src} -> {dst} {fname}: {(u8[0] != want).sum()} bytes differ from Pillow"
        looked_up = torch.from_numpy(np.stack([LUT[c][want[:, :, c]] for c in range(3)]))
        assert torch.equal(out[0], looked_up)
        if planned == "fused":                                                         # the other route: the same bytes
            out2, u82 = _run(img[None], dst, f, route="two_launch")
            assert np.array_equal(u82, u8) and torch.equal(out2, out)


@pytest.mark.parametrize("src,dst,f", [((97, 131), (40, 53), P.BICUBIC), ((300, 50), (77, 13), P.BILINEAR), ((64, 64), (128, 128), P.BILINEAR)])
def test_batch_items_do_not_depend_on_the_batch(src, dst, f):
    imgs = np.stack([R.random_image(src, 30 + i) for i in range(3)])
    out, u8 = _run(imgs, dst, f, dtype=torch.bfloat16, pad=(dst[0] + 3, dst[1] + 5))
    for i in range(3):
        o1, u1 = _run(imgs[i:i + 1], dst, f, dtype=torch.bfloat16, pad=(dst[0] + 3, dst[1] + 5))
        assert np.array_equal(u1[0], u8[i]) and torch.equal(o1[0].view(torch.int16), out[i].view(torch.int16))


@pytest.mark.parametrize("route", [None, "two_launch"])
def test_crop_window_is_the_window_of_the_uncropped_result(route):
    img = R.random_image((96, 64), 40)[None]
    full, full_u8 = _run(img, (48, 32), P.BICUBIC, route=route)
    oy, ox, oh, ow = 9, 3, 32, 21
    out, u8 = _run(img, (48, 32), P.BICUBIC, window=(oy, ox, oh, ow), pad=(40, 24), route=route)
    assert np.array_equal(u8, full_u8[:, oy:oy + oh, ox:ox + ow])
    assert torch.equal(out[:, :, :oh, :ow], full[:, :, oy:oy + oh, ox:ox + ow])
    pad = out.clone()
    pad[:, :, :oh, :ow] = 0
    assert int((pad.view(torch.int32) != 0).sum()) == 0, "padding must be +0 bit for bit"


# ---- pixel_values against the processors ----------------------------------------------------------------------------------------------------------
def _hf(name):
    from transformers import CLIPImageProcessor, GroundingDinoImageProcessor, SamImageProcessor
    if name == "sam":
        return SamImageProcessor()
    if name == "grounding_dino":
        return GroundingDinoImageProcessor()
    return CLIPImageProcessor(size={"shortest_edge": 32}, crop_size={"height": 32, "width": 32})


@pytest.fixture(scope="module")
def processor_reference():
    """one host processor run per case, shared by the dtypes"""
    from PIL import Image
    cases = {"sam": R.random_image((200, 232), 50), "grounding_dino": R.random_image((200, 232), 51), "clip": R.random_image((96, 64), 52)}
    ref = {}
    for name, img in cases.items():
        hf = _hf(name)
        ref[name] = (hf, img, hf(images=Image.fromarray(img), return_tensors="pt"))
    hf = _hf("grounding_dino")
    pair = [R.random_image((200, 232), 53), R.random_image((150, 100), 54)]
    ref["pair"] = (hf, pair, hf(images=[Image.fromarray(p) for p in pair], return_tensors="pt"))
    return ref


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_pixel_values(got, want, dtype, valid_hw):
    assert got.is_cuda and got.dtype == dtype and tuple(got.shape) == tuple(want.shape)
    assert torch.equal(_bits(got.cpu()), _bits(want.to(dtype))), f"{int((_bits(got.cpu()) != _bits(want.to(dtype))).sum())} elements differ"
    for i, (h, w) in enumerate(valid_hw):
        pad = got[i].clone()
        pad[:, :h, :w] = 0
        assert int((_bits(pad) != 0).sum()) == 0, "padding must be +0 bit for bit"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["sam", "grounding_dino", "clip"])
def test_pixel_values_are_the_processors_bit_for_bit(name, dtype, processor_reference):
    from PIL import Image
    hf, img, want = processor_reference[name]
    dp = P.DeviceImageProcessor.from_hf(hf, dtype, DEV)
    valid = {"sam": (883, 1024), "grounding_dino": (800, 928), "clip": (32, 32)}[name]
    for form in (Image.fromarray(img), img, torch.from_numpy(img).to(DEV), [torch.from_numpy(img)[None]]):
        got = dp(images=form, return_tensors="pt")
        _same_pixel_values(got["pixel_values"], want["pixel_values"], dtype, [valid])
        assert got.pixel_values is got["pixel_values"]
    assert set(got.keys()) == set(want.keys())
    for key in ("original_sizes", "reshaped_input_sizes", "pixel_mask"):
        if key in want:
            assert not got[key].is_cuda and got[key].dtype == torch.int64 and torch.equal(got[key], torch.as_tensor(want[key]).long()), key


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_two_sizes_share_the_processors_canvas(dtype, processor_reference):
    hf, pair, want = processor_reference["pair"]
    got = P.DeviceImageProcessor.from_hf(hf, dtype, DEV)(images=pair, return_tensors="pt")
    _same_pixel_values(got["pixel_values"], want["pixel_values"], dtype, [(800, 928), (1200, 800)])
    assert torch.equal(got["pixel_mask"], want["pixel_mask"]) and got["pixel_mask"].dtype == torch.int64
    assert tuple(got["pixel_values"].shape[-2:]) == (1200, 928)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_destination_untouched():
    from tests.test_image_preprocess_cpu import REFUSALS
    from theatergen_amd import _lib
    h = _lib.lib()
    src = torch.from_numpy(R.random_image((4, 4), 60)[None]).to(DEV)
    (_, kv, fv, cv), (_, kh, fh, ch) = P.device_plan(4, 8, P.BILINEAR, src.device), P.device_plan(4, 8, P.BILINEAR, src.device)
    lut = torch.from_numpy(LUT).to(DEV)
    dst = torch.full((4, 8, 8), 7.5, dtype=torch.float32, device=DEV)                 # the call's dense [1, 3, 8, 8] and a fourth plane behind it
    u8 = torch.full((1, 9, 8, 3), 77, dtype=torch.uint8, device=DEV)
    tmp = torch.full((4 * 8 * 3,), 55, dtype=torch.uint8, device=DEV)
    ptr = dict(src=src, kv=kv, fv=fv, cv=cv, kh=kh, fh=fh, ch=ch, lut=lut, dst=dst, u8=u8)
    alias = {256: src.data_ptr(), 4096: dst.data_ptr()}                               # the CPU test's fake pointers: 256 stands for src, 4096 for dst

    def call(**kw):
        a = dict(batch=1, hs=4, ws=4, ksv=int(kv.shape[1]), rh=8, ksh=int(kh.shape[1]), rw=8, oy=0, ox=0, oh=8, ow=8, dt=2, hp=8, wp=8, rows=8, tmp=None)
        a.update({k: v.data_ptr() for k, v in ptr.items()})
        a.update({k: (alias.get(v, v) if k in ptr or k == "tmp" else v) for k, v in kw.items()})
        return h.tg_image_resample_u8(a["src"], a["batch"], a["hs"], a["ws"], a["kv"], a["fv"], a["cv"], a["ksv"], a["rh"], a["kh"], a["fh"], a["ch"], a["ksh"],
                                      a["rw"], a["oy"], a["ox"], a["oh"], a["ow"], a["lut"], a["dst"], a["dt"], a["hp"], a["wp"], a["u8"], a["rows"], a["tmp"],
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    for bad in REFUSALS:
        assert call(**bad) == -1, bad
        assert b"tg_image_resample_u8" in h.tg_last_error(), bad
    torch.cuda.synchronize()
    assert bool((dst == 7.5).all()) and bool((u8 == 77).all()) and bool((tmp == 55).all()), "a refused call wrote"
    assert call() == 0 and call(tmp=tmp.data_ptr()) == 0                               # the same arguments, unbroken, run on either route
    torch.cuda.synchronize()
    assert bool((dst[:3] != 7.5).all()) and bool((dst[3] == 7.5).all()), "[1, 3, 8, 8] is the call's, nothing behind it"
    want = R.pil_resize(src[0].cpu().numpy(), (8, 8), P.BILINEAR)
    assert torch.equal(dst[:3].cpu(), torch.from_numpy(np.stack([LUT[c][want[:, :, c]] for c in range(3)])))
    assert bool((u8[0, 8:] == 77).all())
    assert np.array_equal(u8[0, :8].cpu().numpy(), R.pil_resize(src[0].cpu().numpy(), (8, 8), P.BILINEAR))


# ---- the call surfaces ----------------------------------------------------------------------------------------------------------------------------
def _sam_dicts(dtype=torch.bfloat16):
    """the tiny SamModel of the decoder tests behind a real SamProcessor at S = 128, once with the host processor, once with the device one"""
    from transformers import SamImageProcessor, SamProcessor
    from tests import test_sam_decoder_gpu as TS
    md, _ = TS._surface_dict(dtype)
    g = 8
    proj = torch.randn(3, 256, generator=torch.Generator().manual_seed(4)).to(DEV)
    seen = []

    def encoder(pixel_values):                                                      # a stand-in for SamVisionEncoder: rounds to its dtype first, as that does
        seen.append(pixel_values)
        x = torch.nn.functional.adaptive_avg_pool2d(pixel_values.to(DEV).to(dtype).float(), g)
        return torch.einsum("bchw,cd->bdhw", x, proj).to(dtype).contiguous()
    encoder.device = torch.device(DEV)
    hf = SamProcessor(SamImageProcessor(size={"longest_edge": 16 * g}, pad_size={"height": 16 * g, "width": 16 * g}))
    host = dict(md, sam_processor=hf, sam_encoder=encoder)
    dev = dict(md, sam_processor=P.DeviceSamProcessor(hf, dtype, DEV), sam_encoder=encoder)
    return host, dev, seen


def test_sam_routes_return_identical_results_with_either_processor():
    from theatergen_amd import sam as S
    host, dev, seen = _sam_dicts()
    images = [R.random_image((48, 64), 70), R.random_image((48, 64), 71)]
    boxes = [[[4, 6, 40, 30]], [[12.5, 3, 50, 47]]]
    a = S._sam_device(host, images, None, np.asarray(boxes, np.float64), [(6, 8), (48, 64)])
    b = S._sam_device(dev, images, None, np.asarray(boxes, np.float64), [(6, 8), (48, 64)])
    assert seen[0].dtype == torch.float32 and seen[1].is_cuda and seen[1].dtype == torch.bfloat16          # the host processor's fp32; the storage dtype
    assert torch.equal(seen[0].to(torch.bfloat16).cpu(), seen[1].cpu())
    for t in range(2):
        for i in range(2):
            assert torch.equal(a[0][t][i], b[0][t][i]) and torch.equal(a[1][t][i], b[1][t][i])
    assert np.array_equal(a[2], b[2])
    ra, rb = S.sam_refine_characters(images, boxes, host, 48, 64, 0.85, 0.2), S.sam_refine_characters(images, boxes, dev, 48, 64, 0.85, 0.2)
    for k in range(4):
        for i in range(2):
            assert np.array_equal(np.asarray(ra[k][i]), np.asarray(rb[k][i])), f"sam_refine_characters output {k}, character {i}"
    args = (boxes[0], 0, images[0], None)
    tail = (48, 64, None, None, False, None, None, None, None, 0.85, 0.2, False)
    oa, ob = S.sam_refine_attn(*args, host, *tail), S.sam_refine_attn(*args, dev, *tail)
    for k in range(4):
        assert np.array_equal(np.asarray(oa[k]), np.asarray(ob[k])), f"sam_refine_attn output {k}"
    ea, eb = S.sam_image_embeddings(host, images[0]), S.sam_image_embeddings(dev, images[0])
    assert torch.equal(ea, eb)
    assert dev["sam_processor"].image_processor is host["sam_processor"].image_processor


def test_sam_prompts_through_the_device_processor_equal_the_host_processors():
    host, dev, _ = _sam_dicts()
    img = R.random_image((48, 64), 72)
    a = host["sam_processor"](img, input_boxes=[[[4.0, 6.0, 40.0, 30.0]]], return_tensors="pt")
    b = dev["sam_processor"](img, input_boxes=[[[4.0, 6.0, 40.0, 30.0]]], return_tensors="pt")
    assert torch.equal(a["input_boxes"], b["input_boxes"]) and a["input_boxes"].dtype == b["input_boxes"].dtype
    assert torch.equal(torch.as_tensor(a["original_sizes"]), b["original_sizes"])


class _Tokenizer:
    """stands for the GroundingDINO tokenizer: the fixture's ids for any caption, CPU tensors"""

    def __call__(self, text, return_tensors="pt", padding=False, return_token_type_ids=True, **kw):
        from tests.golden import make_grounding_dino_decoder_golden as G
        n = len(text) if isinstance(text, (list, tuple)) else 1
        ids = torch.tensor(G.INPUT_IDS[:1]).repeat(n, 1)
        return {"input_ids": ids, "attention_mask": (ids != 0).long(), "token_type_ids": torch.zeros_like(ids)}


class _HostProcessor:
    """what GroundingDinoProcessor does with its two parts: the image processor's tensors and the tokenizer's, all on the host"""

    def __init__(self, image_processor, tokenizer):
        self.image_processor, self.tokenizer = image_processor, tokenizer

    def __call__(self, images, text, return_tensors="pt", **kw):
        out = dict(self.image_processor(images=images, return_tensors=return_tensors))
        out.update(self.tokenizer(text, return_tensors=return_tensors, **kw))
        return out


@pytest.mark.parametrize("dname", ["bf16"])
def test_detect_returns_identical_boxes_with_either_processor(dname):
    from transformers import GroundingDinoImageProcessor
    from tests import test_grounding_dino_decoder_gpu as TD
    from theatergen_amd.detector import detect, detect_many
    _, _, _, (_, detector) = TD._model_runs(dname)
    H, W = TD.GE.IMAGE_HW                                                              # the tiny model's query count is tied to this size
    ip = GroundingDinoImageProcessor(size={"shortest_edge": min(H, W), "longest_edge": 333})
    host = _HostProcessor(ip, _Tokenizer())
    dev = P.DeviceGroundingDinoProcessor(host, TD.DTYPES[dname], DEV)
    images = [R.random_image((H // 2, W // 2), 80 + i) for i in range(2)]
    assert dev.device_image_processor.window(H // 2, W // 2)[2] == (H, W)
    a = dev(images=images[0], text="cat.", return_tensors="pt")
    assert a["pixel_values"].is_cuda and not a["input_ids"].is_cuda and not a["pixel_mask"].is_cuda
    want = [detect({"model": detector, "processor": host}, "cat", im) for im in images]
    hits = detector.cache_hits
    got = [detect({"model": detector, "processor": dev}, "cat", im) for im in images]
    assert detector.cache_hits == hits + 2, "the caption cache must still hit: input_ids stay on the CPU"
    many_host = detect_many({"model": detector, "processor": host}, ["cat", "cat"], images)
    many_dev = detect_many({"model": detector, "processor": dev}, ["cat", "cat"], images)
    for (bw, okw), (bg, okg) in zip(want + many_host, got + many_dev):
        assert okw == okg and np.array_equal(bw, bg), f"{bw} vs {bg}"
