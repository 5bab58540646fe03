"""What holds without a GPU for the batched stage 2 (``pipelines.generate_final_images``) and its image-boundary kernels (``tg_image_from_u8`` /
``tg_image_to_u8``): the two symbols are declared, bound and exported at the unchanged ABI version; the host restatement the GPU tests compare against
really contains the cases that tell the right arithmetic from the near-miss (ties for the rounding mode, byte values for division vs reciprocal); the
refusals of the public function come before any device work or side effect."""
import os
import re

import numpy as np
import pytest
import torch

from tests import image_boundary_reference as ibr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_image_symbols_declared_bound_and_exported_at_abi_308():
    from theatergen_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "theatergen_hip.h")).read()
    assert re.search(r"#define TG_ABI_VERSION 308\b", header) and _lib.ABI_VERSION == 308, "additive symbols keep the version"
    for name, nargs in (("tg_image_from_u8", 9), ("tg_image_to_u8", 7)):
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", header, flags=re.M)
        assert m, f"{name} is not declared in include/theatergen_hip.h"
        assert len(m.group(1).split(",")) == nargs
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, f"{name} is not bound with {nargs} arguments"
    assert os.path.exists(os.path.join(ROOT, "theatergen_amd", "csrc", "tg_image.hip"))
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    h = _lib.lib()
    assert h.tg_version() == 308
    assert h.tg_image_from_u8 is not None and h.tg_image_to_u8 is not None


def test_image_entry_points_refuse_bad_arguments_before_any_launch():
    """fake non-null pointers, never dereferenced: validation is on the host side of the ABI"""
    from theatergen_amd import _lib
    h = _lib.lib()
    ok = dict(src=256, batch=1, h=4, w=4, mode=1, copies=1, dst=512, dt=0)

    def from_u8(**kw):
        a = {**ok, **kw}
        return h.tg_image_from_u8(a["src"], a["batch"], a["h"], a["w"], a["mode"], a["copies"], a["dst"], a["dt"], None)
    for bad in (dict(copies=0), dict(copies=-1), dict(dt=3), dict(dt=-1), dict(src=None), dict(dst=None), dict(h=0), dict(w=0), dict(batch=0), dict(mode=2)):
        assert from_u8(**bad) == -1, bad
        assert b"tg_image_from_u8" in h.tg_last_error()
    for args in ((None, 0, 1, 4, 4, 512), (256, 0, 1, 4, 4, None), (256, 3, 1, 4, 4, 512), (256, 0, 0, 4, 4, 512), (256, 0, 1, 0, 4, 512), (256, 0, 1, 4, 0, 512)):
        assert h.tg_image_to_u8(*args, None) == -1, args
        assert b"tg_image_to_u8" in h.tg_last_error()
    with pytest.raises(RuntimeError, match="theatergen_hip error"):
        _lib.check(h.tg_image_to_u8(None, 0, 1, 4, 4, 512, None))


def test_image_kernels_are_gated_at_zero_scratch():
    from theatergen_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    for sub in ("image_from_u8_kernel<", "image_to_u8_kernel<"):
        gates = [g for g in build.HOT_GATES if g[0] == sub]
        assert len(gates) == 1 and gates[0][1] == 0, f"HOT_GATES entry for {sub}: {gates}"
    res = build.kernel_resources(verbose=False)
    mine = {k: v for k, v in res.items() if v["file"] == "tg_image.hip"}
    assert len(mine) == 12, sorted(mine)                  # {from, to} x {bf16, f16, float} x {4 pixels, 1 pixel} per thread
    for name, r in mine.items():
        assert r.get("scratch", 0) == 0, f"{name}: scratch {r.get('scratch')} bytes / lane"
    assert not build.check_resources(res)


def test_tie_search_finds_ties_of_both_parities():
    """without them the GPU test could not tell round-half-to-even (numpy's ``.round()``) from round-half-away (``roundf``)"""
    t = ibr.ties()
    ks = [k for k, _ in t]
    assert len(t) >= 150, len(t)
    assert any(k % 2 == 0 for k in ks) and any(k % 2 == 1 for k in ks)
    x = np.array([x for _, x in t], np.float32)
    assert x.dtype == np.float32 and np.all(np.abs(x) <= 1)
    np.testing.assert_array_equal(ibr.to_u8_chain(x), np.array(ks, np.float32) + np.float32(0.5))
    got = ibr.to_u8_host(torch.from_numpy(x).reshape(1, 1, 1, -1).expand(1, 3, 1, -1))[0, 0, :, 0]
    np.testing.assert_array_equal(got, np.array([k if k % 2 == 0 else k + 1 for k in ks], np.uint8))       # half to even
    away = np.array([k + 1 for k in ks], np.uint8)
    assert int((got != away).sum()) == sum(k % 2 == 0 for k in ks) > 0


def test_division_and_reciprocal_multiply_differ_for_many_bytes():
    """the fp32 output of ``tg_image_from_u8`` is where a multiply by 1 / 255 in place of the division shows"""
    d = ibr.division_vs_reciprocal()
    assert len(d) >= 100, len(d)
    imgs = ibr.all_bytes_images(2, 16, 24, seed=3)
    for b in range(2):
        for c in range(3):
            assert set(imgs[b, :, :, c].ravel().tolist()) == set(range(256))
    assert not np.array_equal(imgs[0, :, :, 0], imgs[0, :, :, 1]) and not np.array_equal(imgs[0], imgs[1])
    want = ibr.from_u8_host(imgs, torch.float32, 1, 2)
    assert want.shape == (4, 3, 16, 24) and torch.equal(want[:2], want[2:])
    assert float(want.min()) == -1.0 and float(want.max()) == 1.0


class _Untouchable:
    """stands where the adapter goes: any read of it (``.pipe``, ``.set_scale``) is a side effect the refusals must come before"""

    def __getattr__(self, name):
        raise AssertionError(f"generate_final_images touched adapter.{name} before refusing")


def _call(basever="1.5", n=2, **over):
    from PIL import Image
    from theatergen_amd import pipelines
    lat = [torch.full((5, 1, 4, 16, 16), float(i + 1)) for i in range(n)]
    kept = [t.clone() for t in lat]
    text = torch.zeros(2, 77, 32)
    a = dict(prompts=["p"] * n, negs=["n"] * n, chars=[[Image.new("RGB", (8, 8))] for _ in range(n)], seeds=list(range(n)),
             masks=[Image.new("L", (128, 128), 255) for _ in range(n)], imgs=[Image.new("RGB", (128, 128)) for _ in range(n)], lat=lat,
             emb=[(text, text[:1], text[1:])] * n)
    a.update(over)

    def processor(arr):
        raise AssertionError("generate_final_images called the processor before refusing")
    try:
        pipelines.generate_final_images(basever, processor, _Untouchable(), a["prompts"], a["negs"], a["chars"], 128, 128, a["seeds"], a["masks"], a["imgs"],
                                        _Untouchable(), a["lat"], a["emb"], 4, 3)
    finally:
        for t, k in zip(lat, kept):
            assert torch.equal(t, k), "latents_all_list was written before the refusal"


def test_generate_final_images_refuses_before_any_device_work_or_side_effect():
    from PIL import Image
    with pytest.raises(NotImplementedError, match="xl"):
        _call(basever="xl")
    with pytest.raises(ValueError, match="one entry per turn"):
        _call(n=0)
    for key, short in (("prompts", ["p"]), ("negs", ["n"]), ("seeds", [1]), ("chars", [[Image.new("RGB", (8, 8))]]), ("masks", [Image.new("L", (128, 128))]),
                       ("imgs", [Image.new("RGB", (128, 128))]), ("lat", [torch.zeros(5, 1, 4, 16, 16)]), ("emb", [(torch.zeros(2, 77, 32),) * 3])):
        with pytest.raises(ValueError, match="one entry per turn"):
            _call(**{key: short})
    with pytest.raises(ValueError, match="images differ in size"):
        _call(imgs=[Image.new("RGB", (128, 128)), Image.new("RGB", (128, 120))])
    with pytest.raises(ValueError, match="masks differ in size"):
        _call(masks=[Image.new("L", (128, 128)), Image.new("L", (64, 64))])
    with pytest.raises(ValueError, match="uint8 RGB"):
        _call(imgs=[Image.new("L", (128, 128)), Image.new("L", (128, 128))])
    with pytest.raises(ValueError, match="text embeddings differ"):
        _call(emb=[(torch.zeros(2, 77, 32),) * 3, (torch.zeros(2, 60, 32),) * 3])


def test_sample_takes_a_noise_argument_and_keeps_its_default_signature():
    import inspect
    from theatergen_amd.vae import DiagonalGaussianDistribution
    p = inspect.signature(DiagonalGaussianDistribution.sample).parameters
    assert list(p) == ["self", "generator", "scale", "noise"] and p["noise"].default is None and p["scale"].default == 1.0
    d = DiagonalGaussianDistribution(torch.zeros(2, 8, 4, 4), torch.bfloat16)
    with pytest.raises(ValueError, match="noise shape"):
        d.sample(noise=torch.zeros(1, 4, 4, 4))


def test_ops_wrappers_refuse_wrong_tensors_without_a_gpu():
    from theatergen_amd import ops
    with pytest.raises(RuntimeError, match="GPU"):
        ops.image_from_u8(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), torch.float32)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.image_to_u8(torch.zeros(1, 3, 4, 4))
