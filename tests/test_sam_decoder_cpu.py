"""CPU: SAM's prompt / mask head kernels (``tg_sam_posenc`` / ``tg_sam_mask_head`` / ``tg_sam_mask_post``, csrc/tg_sam_head.hip), their weight packing, the fp64
post-processing reference and the device route of ``theatergen_amd/sam.py`` — what can be pinned without a device.

  * the three symbols are declared in the header, bound in ``_lib.SIGNATURES`` and exported by the library; the ABI version did not move;
  * ``build.HOT_GATES`` has an unshadowed 0-scratch entry for each kernel and every built instance passes it;
  * host validation runs before any launch (fake non-null pointers, never read; stream NULL); the ``ops`` wrappers refuse CPU tensors;
  * ``weights_pack.pack_sam_upscale``: the matrices equal ``conv_transpose2d`` in fp64, the fragments hold them in the order the kernel reads;
  * tests/sam_post_reference.py equals transformers' ``post_process_masks`` + the reference's resize; the OR rule equals the float resize;
  * with stubs that count calls, ``sam_refine_attn`` on the device route runs the processor, the encoder and the decoder once each; constructor refusals.
"""
import ctypes as C
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TG_ERR_ARG, TG_ERR_UNSUPPORTED = -1, -3
SYMBOLS = ("tg_sam_posenc", "tg_sam_mask_head", "tg_sam_mask_post")
FAKE = 64                                                             # a non-null, 16-byte aligned "pointer": validation never reads it


def _lib_built():
    from theatergen_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib


def test_symbols_are_declared_bound_and_exported_at_abi_308():
    _lib = _lib_built()
    header = open(os.path.join(ROOT, "include", "theatergen_hip.h")).read()
    assert re.search(r"^int tg_sam_posenc\(int32_t out_dtype, const float\* coords, int64_t n, const float\* gauss, int32_t F, const int32_t\* labels,", header, flags=re.M)
    assert re.search(r"^int tg_sam_mask_head\(int32_t dtype, const void\* x, int32_t images, int32_t g, const void\* w1, const void\* w2,", header, flags=re.M)
    assert re.search(r"^int tg_sam_mask_post\(const float\* logits, int32_t planes, int32_t L, int32_t S, int32_t hr, int32_t wr,", header, flags=re.M)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for sym in SYMBOLS:
        assert sym in _lib.SIGNATURES, f"{sym} is not bound"
        assert re.search(rf"\bT {sym}$", nm, flags=re.M), f"libtheatergen_hip.so does not export {sym}"
        assert getattr(_lib.lib(), sym) is not None
    assert re.search(r"#define TG_ABI_VERSION 308\b", header) and _lib.ABI_VERSION == 308 and _lib.lib().tg_version() == 308
    from theatergen_amd import ops
    assert all(callable(getattr(ops, n)) for n in ("sam_posenc", "sam_mask_head", "sam_mask_post"))


def test_resource_gates_cover_every_instance_at_zero_scratch():
    from theatergen_amd import build
    _lib_built()
    if not os.path.exists(os.path.join(build.OBJ, "tg_sam_head.o.res")):
        build.build(verbose=False)
    res = build.kernel_resources(verbose=False)
    want = {"sam_mask_head_kernel<": {"sam_mask_head_kernel<bf16>", "sam_mask_head_kernel<f16>"},
            "sam_posenc_kernel<": {"sam_posenc_kernel<float>", "sam_posenc_kernel<bf16>", "sam_posenc_kernel<f16>"},
            "sam_mask_post_kernel": {"sam_mask_post_kernel"}}
    for sub, names in want.items():
        gates = [g for g in build.HOT_GATES if g[0] == sub]
        assert len(gates) == 1 and gates[0][1] == 0, f"HOT_GATES entry for {sub}: {gates}"
        assert not any(g[0] in sub for g in build.HOT_GATES[:build.HOT_GATES.index(gates[0])]), f"an earlier gate shadows {sub}"
        mine = {n: r for n, r in res.items() if sub in n}
        assert set(mine) == names and {r["file"] for r in mine.values()} == {"tg_sam_head.hip"}, sorted(mine)
        for n, r in mine.items():
            assert r.get("scratch", 0) == 0 and r.get("vgpr_spill", 0) == 0 and r.get("sgpr_spill", 0) == 0, f"{n}: {r}"
    assert not [b for b in build.check_resources(res) if "sam_" in b]


# ---- host validation -----------------------------------------------------------------------------------------------------------------
def _call(name, a):
    _lib = _lib_built()
    h = _lib.lib()
    assert h.tg_gemm(C.byref(_lib.GemmDesc()), None) == -1 and b"tg_gemm" in h.tg_last_error()      # another call's message, to be replaced
    rc = getattr(h, name)(*a)
    return rc, h.tg_last_error()


POSENC = dict(out_dtype=2, coords=FAKE, n=7, gauss=FAKE, F=128, labels=None, table=None, out=FAKE)
POSENC_REFUSALS = [("bad dtype", dict(out_dtype=3)), ("n 0", dict(n=0)), ("n < 0", dict(n=-1)), ("F 0", dict(F=0)), ("null coords", dict(coords=None)),
                   ("null gauss", dict(gauss=None)), ("null out", dict(out=None)), ("labels without table", dict(labels=FAKE)),
                   ("table without labels", dict(table=FAKE))]


@pytest.mark.parametrize("what,over", POSENC_REFUSALS, ids=[r[0] for r in POSENC_REFUSALS])
def test_posenc_refuses_before_any_launch(what, over):
    a = dict(POSENC, **over)
    rc, msg = _call("tg_sam_posenc", [a[k] for k in ("out_dtype", "coords", "n", "gauss", "F", "labels", "table", "out")] + [None])
    assert rc == TG_ERR_ARG and b"tg_sam_posenc:" in msg, f"{what}: {rc} {msg!r}"


HEAD = dict(dtype=0, x=FAKE, images=1, g=16, w1=FAKE, w2=FAKE, vec=FAKE, hyper_in=FAKE, M=4, eps=1e-6, out=FAKE)
HEAD_REFUSALS = [(f"g {g}", dict(g=g), TG_ERR_UNSUPPORTED) for g in (4, 12, 20, 63, 72, 128)] + [
    ("M 5", dict(M=5), TG_ERR_UNSUPPORTED), ("M 0", dict(M=0), TG_ERR_ARG), ("images 0", dict(images=0), TG_ERR_ARG), ("g 0", dict(g=0), TG_ERR_ARG),
    ("bad dtype", dict(dtype=2), TG_ERR_ARG), ("eps 0", dict(eps=0.0), TG_ERR_ARG), ("misaligned x", dict(x=FAKE + 8), TG_ERR_ARG),
    ("misaligned out", dict(out=FAKE + 4), TG_ERR_ARG)] + [(f"null {f}", {f: None}, TG_ERR_ARG) for f in ("x", "w1", "w2", "vec", "hyper_in", "out")]


@pytest.mark.parametrize("what,over,code", HEAD_REFUSALS, ids=[r[0] for r in HEAD_REFUSALS])
def test_mask_head_refuses_before_any_launch(what, over, code):
    a = dict(HEAD, **over)
    rc, msg = _call("tg_sam_mask_head", [a[k] for k in ("dtype", "x", "images", "g", "w1", "w2", "vec", "hyper_in", "M", "eps", "out")] + [None])
    assert rc == code and b"tg_sam_mask_head:" in msg, f"{what}: {rc} {msg!r}"


POST = dict(logits=FAKE, planes=3, L=256, S=1024, hr=682, wr=1024, h0=333, w0=500, threshold=0.0, ht=41, wt=62, mask=FAKE, areas=FAKE)
POST_REFUSALS = [(f"{k} 0", {k: 0}) for k in ("planes", "L", "S", "hr", "wr", "h0", "w0", "ht", "wt")] + [
    ("hr > S", dict(hr=1025)), ("wr > S", dict(wr=2000)), ("ht < 0", dict(ht=-3)), ("planes 70000", dict(planes=70000)), ("side > 32768", dict(wt=40000))] + [
    (f"null {f}", {f: None}) for f in ("logits", "mask", "areas")]


@pytest.mark.parametrize("what,over", POST_REFUSALS, ids=[r[0] for r in POST_REFUSALS])
def test_mask_post_refuses_before_any_launch(what, over):
    a = dict(POST, **over)
    rc, msg = _call("tg_sam_mask_post", [a[k] for k in ("logits", "planes", "L", "S", "hr", "wr", "h0", "w0", "threshold", "ht", "wt", "mask", "areas")] + [None])
    assert rc == TG_ERR_ARG and b"tg_sam_mask_post:" in msg, f"{what}: {rc} {msg!r}"


def test_ops_wrappers_refuse_cpu_tensors():
    from theatergen_amd import ops
    with pytest.raises(RuntimeError, match="GPU"):
        ops.sam_posenc(torch.zeros(3, 2), torch.zeros(2, 128))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.sam_mask_head(torch.zeros(64, 256, dtype=torch.bfloat16), 1, 8, torch.zeros(65536, dtype=torch.bfloat16), torch.zeros(8192, dtype=torch.bfloat16),
                          torch.zeros(224), torch.zeros(1, 4, 32, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.sam_mask_post(torch.zeros(1, 3, 32, 32), 128, (128, 128), (64, 64), (8, 8))


# ---- weight packing ------------------------------------------------------------------------------------------------------------------
def test_convtranspose_packing_equals_conv_transpose2d_in_fp64():
    from theatergen_amd.weights_pack import convtranspose2x2_matrices, pack_sam_upscale, sam_upscale_k_order
    gen = torch.Generator().manual_seed(0)
    c1w, c2w = torch.randn(256, 64, 2, 2, generator=gen).double(), torch.randn(64, 32, 2, 2, generator=gen).double()
    c1b, lnw, lnb, c2b = (torch.randn(n, generator=gen).double() for n in (64, 64, 64, 32))
    x = torch.randn(2, 256, 3, 5, generator=gen).double()
    for w, b in ((c1w, c1b), (c2w, c2b)):
        xin = x[:, :w.shape[0]]
        ref = F.conv_transpose2d(xin, w, b, stride=2)
        m = convtranspose2x2_matrices(w)                                                        # [4, Cout, Cin]
        got = torch.einsum("kon,bnij->bkoij", m, xin) + b[None, None, :, None, None]            # [B, (a, b), Cout, i, j]
        got = got.reshape(2, 2, 2, w.shape[1], 3, 5).permute(0, 3, 4, 1, 5, 2).reshape(ref.shape)   # pixel (2 i + a, 2 j + b)
        assert torch.allclose(got, ref, rtol=1e-12, atol=1e-12)
    w1, w2, vec = pack_sam_upscale(c1w, c1b, lnw, lnb, c2w, c2b)
    assert vec.dtype == torch.float32 and torch.equal(vec, torch.cat([c1b, lnw, lnb, c2b]).float())
    m1, m2 = convtranspose2x2_matrices(c1w), convtranspose2x2_matrices(c2w)
    f1 = w1.reshape(4, 2, 16, 2, 32, 8)                                                         # [ab, tile, ks, hi, l31, j], as the kernel indexes it
    f2 = w2.reshape(4, 4, 2, 32, 8)
    kap = sam_upscale_k_order()
    assert sorted(kap.reshape(-1).tolist()) == list(range(64))
    for ab, t, ks, hi, l, j in [(0, 0, 0, 0, 0, 0), (3, 1, 15, 1, 31, 7), (2, 1, 6, 0, 17, 3), (1, 0, 9, 1, 4, 5)]:
        assert f1[ab, t, ks, hi, l, j] == m1[ab, 32 * t + l, 16 * ks + 8 * hi + j]
        assert f2[ab, ks % 4, hi, l, j] == m2[ab, l, kap[ks % 4, hi, j]]
    # the kernel's second GEMM sums over (ks, hi, j) with the first GEMM's accumulator order as K: register 8 (ks & 1) + j of tile ks >> 1 of half hi
    for ks in range(4):
        for hi in range(2):
            for j in range(8):
                r = 8 * (ks & 1) + j
                assert int(kap[ks, hi, j]) == 32 * (ks >> 1) + 8 * (r >> 2) + 4 * hi + (r & 3)


# ---- post-processing reference -------------------------------------------------------------------------------------------------------
TARGETS = lambda h0, w0: [(h0 // 8, w0 // 8), (int(h0 / 3.3), int(w0 / 2.7)), (h0 + h0 // 2 + 1, 2 * w0 + 3)]


def test_post_reference_equals_transformers_post_process_masks():
    tr = pytest.importorskip("transformers")
    if not hasattr(tr, "SamImageProcessorPil"):
        pytest.skip("this transformers has no SamImageProcessorPil")
    from tests import sam_post_reference as R
    proc = tr.SamImageProcessorPil()
    gen = torch.Generator().manual_seed(1)
    lg = torch.randn(1, 3, 256, 256, generator=gen)
    for orig, resh in (((333, 500), (682, 1024)), ((512, 512), (1024, 1024))):
        theirs = proc.post_process_masks(lg[None].clone(), torch.tensor([orig]), torch.tensor([resh]))[0]
        vals = R.post_values(lg, 1024, resh, orig)
        sure = vals.abs() > 1e-5 * float(lg.abs().max())
        assert float(sure.double().mean()) > 1 - 1e-3
        assert int(((theirs.bool() != (vals > 0)) & sure).sum()) == 0
        for target in TARGETS(*orig)[:2]:
            ours = R.resize_bool(theirs, target)
            ref = F.interpolate(theirs.type(torch.float), target, mode="bilinear").type(torch.bool)
            assert torch.equal(ours, ref)


@pytest.mark.parametrize("orig", [(64, 64), (48, 64), (333, 500)])
def test_or_rule_equals_the_float_interpolate(orig):
    from tests import sam_post_reference as R
    gen = torch.Generator().manual_seed(orig[0])
    for density in (0.5, 0.05):
        m = torch.rand((2, 3) + orig, generator=gen) < density
        for target in TARGETS(*orig) + [orig]:
            assert torch.equal(R.or_taps(m, target), R.resize_bool(m, target)), (orig, target)
    big = torch.rand(1, 512, 512, generator=gen) < 0.3                                      # the 64 x 64 target of a 512^2 mask: pixels (8 i + 3..4, 8 j + 3..4)
    blocks = big.reshape(1, 64, 8, 64, 8)[:, :, 3:5, :, 3:5].any(dim=4).any(dim=2)
    assert torch.equal(R.resize_bool(big, (64, 64)), blocks) and torch.equal(R.or_taps(big, (64, 64)), blocks)


# ---- the device route with stubs -----------------------------------------------------------------------------------------------------
def _stub_route(monkeypatch):
    from tests import sam_post_reference as R
    from theatergen_amd import ops
    from theatergen_amd.sam_decoder import SamModel, sam_decoder_config
    calls = dict(processor=0, encoder=0, decoder=0, post=0)
    g = 8

    class Counting(SamModel):
        def __call__(self, image_embeddings=None, input_boxes=None, input_points=None, **kw):
            calls["decoder"] += 1
            B, nb = (input_boxes if input_boxes is not None else input_points).shape[:2]
            gen = torch.Generator().manual_seed(int(image_embeddings.sum()))
            return SimpleNamespace(pred_masks=torch.randn(B, nb, 3, 4 * g, 4 * g, generator=gen), iou_scores=torch.rand(B, nb, 3, generator=gen).bfloat16())

    def processor(images, return_tensors="pt", **kw):
        calls["processor"] += 1
        assert not kw, "the device route rescales the prompts itself"
        images = images if isinstance(images, list) else [images]
        return {"pixel_values": torch.stack([torch.full((3, 128, 128), float(im[0, 0, 0])) for im in images]),
                "original_sizes": torch.tensor([im.shape[:2] for im in images]), "reshaped_input_sizes": torch.tensor([(96, 128) for _ in images])}

    def encoder(pv):
        calls["encoder"] += 1
        return pv[:, :1, :g, :g].clone()

    def post(logits, padded, resh, orig, target, threshold=0.0, out=None):
        calls["post"] += 1
        mask = R.or_taps(R.post_values(logits, padded, resh, orig) > threshold, target).to(torch.uint8)
        return mask, mask.sum((-1, -2)).to(torch.int32)
    monkeypatch.setattr(ops, "sam_mask_post", post)
    model = Counting(None, sam_decoder_config(g), with_vision=False)
    return {"sam_model": model, "sam_processor": processor, "sam_encoder": encoder}, calls


def _image(tag):
    im = np.zeros((48, 64, 3), np.uint8)
    im[0, 0, 0] = tag
    return im


def test_refine_attn_on_the_device_route_runs_each_stage_once(monkeypatch):
    from theatergen_amd import sam as S
    md, calls = _stub_route(monkeypatch)
    m, c, m512, c512 = S.sam_refine_attn([[4, 6, 40, 30]], 0, _image(3), None, md, 48, 64, None, None, False, None, None, None, None, 0.85, 0.2, False)
    assert calls == dict(processor=1, encoder=1, decoder=1, post=2)
    assert m.shape == (6, 8) and m512.shape == (48, 64) and m.dtype == np.bool_ and isinstance(c, np.float32) and c == c512
    # the selection is select_mask's, on the areas the post-processing returns
    masks, conf = S.sam(md, _image(3), input_boxes=[[[4, 6, 40, 30]]], target_mask_shape=(48, 64))
    want, want_c = S.select_mask(masks[0][0], conf, discourage_mask_below_confidence=0.85, discourage_mask_below_coarse_iou=0.2)
    assert np.array_equal(want, m512) and want_c == c512
    calls.update(processor=0, encoder=0, decoder=0, post=0)
    out = S.sam_refine_characters([_image(3), _image(9)], [[[4, 6, 40, 30]], [[1, 2, 30, 40]]], md, 48, 64, 0.85, 0.2)
    assert calls == dict(processor=1, encoder=1, decoder=1, post=4) and [len(o) for o in out] == [2, 2, 2, 2]
    with pytest.raises(NotImplementedError, match="use_box_input"):
        S.sam_refine_attn([[4, 6, 40, 30]], 0, _image(3), None, md, 48, 64, None, None, True, None, None, None, None, 0.85, 0.2, False)
    md["sam_model"] = object()
    with pytest.raises(NotImplementedError, match="device route"):
        S.sam_refine_characters([_image(3)], [[[4, 6, 40, 30]]], md, 48, 64, 0.85, 0.2)


def test_prompts_are_rescaled_as_the_processor_does(monkeypatch):
    from theatergen_amd import sam as S
    md, _ = _stub_route(monkeypatch)
    seen = {}
    inner = type(md["sam_model"]).__call__

    def spy(self, **kw):
        seen.update(kw)
        return inner(self, **kw)
    monkeypatch.setattr(type(md["sam_model"]), "__call__", spy)
    S.sam(md, _image(1), input_boxes=[[[4, 6, 40, 30]]], target_mask_shape=(6, 8))
    assert np.array_equal(seen["input_boxes"], np.array([[[8.0, 12.0, 80.0, 60.0]]]))               # 48 x 64 -> 96 x 128: both axes x 2
    S.sam(md, _image(1), input_points=[[[[10, 20], [3, 4]]]], target_mask_shape=(6, 8))
    assert np.array_equal(seen["input_points"], np.array([[[[20.0, 40.0], [6.0, 8.0]]]])) and np.array_equal(seen["input_labels"], np.ones((1, 1, 2), np.int32))


def test_constructor_and_state_dict_refusals():
    from theatergen_amd.sam_decoder import SamMaskDecoder, SamModel, SamPromptEncoder, sam_decoder_config
    for bad in (dict(hidden_size=128), dict(num_attention_heads=4), dict(attention_downsample_rate=1), dict(mlp_dim=1024), dict(num_hidden_layers=3),
                dict(num_multimask_outputs=4), dict(iou_head_depth=2), dict(image_embedding_size=12), dict(image_embedding_size=72), dict(image_embedding_size=0)):
        cfg = sam_decoder_config()
        for k, v in bad.items():
            setattr(cfg, k, v)
        for cls in (SamPromptEncoder, SamMaskDecoder, lambda c: SamModel(None, c, with_vision=False)):
            with pytest.raises(NotImplementedError, match="supported"):
                cls(cfg)
    m = SamModel(None, sam_decoder_config(8), with_vision=False)
    sd = m.state_dict()
    assert "mask_decoder.transformer.layers.1.cross_attn_image_to_token.out_proj.weight" in sd and "prompt_encoder.mask_embed.conv3.bias" in sd
    assert "mask_decoder.output_hypernetworks_mlps.3.layers.0.weight" in sd and "shared_image_embedding.positional_embedding" in sd
    loaded = SamModel.from_state_dict(None, sd, device="cpu", dtype=torch.float16, decoder_config=sam_decoder_config(8))
    assert loaded.dtype == torch.float16 and loaded.shared_image_embedding.positional_embedding.dtype == torch.float32
    less = {k: v for k, v in sd.items() if k != "mask_decoder.iou_token.weight"}
    with pytest.raises(RuntimeError, match="missing"):
        SamModel.from_state_dict(None, less, device="cpu", decoder_config=sam_decoder_config(8))
    with pytest.raises(RuntimeError, match="unexpected"):
        SamModel.from_state_dict(None, dict(sd, **{"vision_encoder.pos_embed": torch.zeros(1)}), device="cpu", decoder_config=sam_decoder_config(8))
    with pytest.raises(RuntimeError, match="GPU"):
        m(image_embeddings=torch.zeros(1, 256, 8, 8), input_boxes=[[[1, 2, 3, 4]]])
