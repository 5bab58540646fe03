"""GPU: SAM's prompt encoder, mask decoder and mask post-processing on the device (csrc/tg_sam_head.hip, theatergen_amd/sam_decoder.py, the device route of
theatergen_amd/sam.py).

  * ``ops.sam_posenc`` against an fp64 restatement, within the fp32 rounding of its argument carried through the sine's derivative;
  * ``ops.sam_mask_head`` against fp64 conv_transpose2d / layer_norm / gelu / matmul on the same rounded operands: within the per-op tolerance AND no worse
    than twice the unfused route through the existing kernels; pixel placement with a one-hot token;
  * ``ops.sam_mask_post`` against tests/sam_post_reference.py (fp64) away from the threshold, against the reference's float resize exactly, areas exactly;
  * the decoder end to end against transformers' float64 goldens: within 3 x the rounding floor the generator measured and below its autocast route;
  * the call surface with a stub processor and a stub encoder.
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]


def op_tol(dtype):
    return 1.5e-2 if dtype == torch.bfloat16 else 4e-3


def rel_l2(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return float((got - ref).norm() / ref.norm())


def _record(rec):
    """TG_SAM_ERR_JSON=path: the measured errors go to that file too (scripts/sam_decoder_timing.py turns them into the findings table)"""
    path = os.environ.get("TG_SAM_ERR_JSON")
    if path:
        import json
        recs = json.load(open(path)) if os.path.exists(path) else []
        with open(path, "w") as f:
            json.dump(recs + [rec], f, indent=1)


# ---- positional encoding -------------------------------------------------------------------------------------------------------------------
def _coords(n, gen):
    c = torch.rand(n, 2, generator=gen) * 1.6 - 0.3                       # below 0 and above 1 included
    edge = torch.tensor([[0.0, 1.0], [1.0, 0.0], [-0.25, 1.5], [0.5, 0.5]])
    c[:min(n, 4)] = edge[:min(n, 4)]
    return c.float().contiguous()


def _posenc64(c, gm):
    t = (2 * c.double() - 1) @ gm.double()
    return torch.cat([torch.sin(2 * np.pi * t), torch.cos(2 * np.pi * t)], -1)


def _posenc_bound(c, gm):
    xp = (2 * c.double() - 1).abs()
    b = 2 * np.pi * 2.0 ** -21 * (xp[:, :1] * gm[0].double().abs()[None] + xp[:, 1:] * gm[1].double().abs()[None]) + 2.0 ** -20
    return torch.cat([b, b], -1)


@pytest.mark.parametrize("n", [1, 7, 64, 4096])
def test_posenc_fp32_within_the_rounding_of_its_argument(n):
    from theatergen_amd import ops
    gen = torch.Generator().manual_seed(n)
    gm = (32 * torch.randn(2, 128, generator=gen)).float().contiguous()
    if n in (64, 4096):                                                   # the dense grid of get_image_wide_positional_embeddings
        g = int(n ** 0.5)
        v = (torch.arange(g, dtype=torch.float32) + 0.5) / g
        c = torch.stack([v[None, :].expand(g, g), v[:, None].expand(g, g)], -1).reshape(n, 2).contiguous()
    else:
        c = _coords(n, gen)
    ref, bound = _posenc64(c, gm), _posenc_bound(c, gm)
    got = ops.sam_posenc(c.to(DEV), gm.to(DEV)).cpu()
    assert got.dtype == torch.float32 and got.shape == (n, 256)
    err = (got.double() - ref).abs()
    print(f"posenc n={n}: max err {float(err.max()):.3e}, max err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    for dt, eps in ((torch.bfloat16, 2.0 ** -7), (torch.float16, 2.0 ** -10)):          # eps = the spacing at 1: ulp(v) = eps 2^floor(log2 |v|)
        lo = ops.sam_posenc(c.to(DEV), gm.to(DEV), dtype=dt).cpu()
        assert lo.dtype == dt
        mag = ref.abs() + bound
        half_ulp = torch.maximum(2.0 ** torch.floor(torch.log2(mag)) * eps / 2, torch.tensor(2.0 ** -25 if dt == torch.float16 else 0.0).double())
        assert bool(((lo.double() - ref).abs() <= bound + half_ulp).all()), dt


def test_posenc_labels_select_the_added_row_exactly():
    from theatergen_amd import ops
    gen = torch.Generator().manual_seed(5)
    gm = (32 * torch.randn(2, 128, generator=gen)).float()
    c = _coords(37, gen)
    labels = torch.tensor([(-1, 0, 1, 2, 3)[i % 5] for i in range(37)], dtype=torch.int32)
    table = torch.randn(5, 256, generator=gen).float()
    plain = ops.sam_posenc(c.to(DEV), gm.to(DEV)).cpu()
    got = ops.sam_posenc(c.to(DEV), gm.to(DEV), labels.to(DEV), table.to(DEV)).cpu()
    want = torch.where(labels[:, None] < 0, table[4][None].expand(37, -1), plain + table[labels.clamp(min=0).long()])
    assert torch.equal(got, want)


# ---- mask head -----------------------------------------------------------------------------------------------------------------------------
def _head_operands(P, g, M, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s, k=1.0: (k * torch.randn(*s, generator=gen)).to(dtype)
    return dict(x=r(P * g * g, 256), c1w=r(256, 64, 2, 2, k=0.05), c1b=r(64, k=0.1), lnw=(1 + 0.1 * torch.randn(64, generator=gen)).to(dtype), lnb=r(64, k=0.1),
                c2w=r(64, 32, 2, 2, k=0.1), c2b=r(32, k=0.1), hyper=r(P, M, 32))


def _head64(o, P, g):
    d = {k: v.double() for k, v in o.items()}
    x = d["x"].reshape(P, g, g, 256).permute(0, 3, 1, 2)
    u = F.conv_transpose2d(x, d["c1w"], d["c1b"], stride=2)
    u = F.gelu(F.layer_norm(u.permute(0, 2, 3, 1), (64,), d["lnw"], d["lnb"], 1e-6).permute(0, 3, 1, 2))
    u = F.gelu(F.conv_transpose2d(u, d["c2w"], d["c2b"], stride=2))
    return torch.einsum("pmc,pchw->pmhw", d["hyper"], u)


def _head_fused(o, P, g):
    from theatergen_amd import ops
    from theatergen_amd.weights_pack import pack_sam_upscale
    w1, w2, vec = pack_sam_upscale(o["c1w"], o["c1b"], o["lnw"], o["lnb"], o["c2w"], o["c2b"])
    return ops.sam_mask_head(o["x"].to(DEV), P, g, w1.to(DEV), w2.to(DEV), vec.to(DEV), o["hyper"].to(DEV).contiguous())


def _head_unfused(o, P, g):
    """the same chain through the existing kernels: GEMM, pixel shuffle by indexing, LayerNorm, GELU, GEMM, GELU, GEMM (rounds to the dtype after each)"""
    from theatergen_amd import ops
    from theatergen_amd.weights_pack import convtranspose2x2_matrices
    d = {k: v.to(DEV) for k, v in o.items()}
    T, M = P * g * g, o["hyper"].shape[1]
    m1 = convtranspose2x2_matrices(d["c1w"]).reshape(256, 256).contiguous()
    y = ops.linear(d["x"], m1, d["c1b"].repeat(4).contiguous())                                    # [T, (a, b, 64)]
    y = y.reshape(P, g, g, 2, 2, 64).permute(0, 1, 3, 2, 4, 5).reshape(T * 4, 64).contiguous()     # [P, 2g, 2g, 64]
    y = ops.act(ops.layernorm(y, d["lnw"], d["lnb"], 1e-6), ops.ACT_GELU)
    m2 = convtranspose2x2_matrices(d["c2w"]).reshape(128, 64).contiguous()
    z = ops.act(ops.linear(y, m2, d["c2b"].repeat(4).contiguous()), ops.ACT_GELU)                  # [T * 4, (a', b', 32)]
    z = z.reshape(P, 2 * g, 2 * g, 2, 2, 32).permute(0, 1, 3, 2, 4, 5).reshape(P, 16 * g * g, 32).contiguous()
    hp = F.pad(d["hyper"], (0, 0, 0, 8 - M)).contiguous()
    out = torch.stack([ops.linear(z[p], hp[p])[:, :M] for p in range(P)])                          # [P, pixels, M]
    return out.permute(0, 2, 1).reshape(P, M, 4 * g, 4 * g)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P,g", [(1, 8), (3, 16), (1, 64)])
def test_mask_head_against_fp64_and_the_unfused_route(P, g, dtype):
    o = _head_operands(P, g, 4, dtype, seed=100 * g + P)
    ref = _head64(o, P, g)
    got = _head_fused(o, P, g)
    assert got.dtype == torch.float32 and got.shape == (P, 4, 4 * g, 4 * g)
    e_fused, e_unfused = rel_l2(got, ref), rel_l2(_head_unfused(o, P, g), ref)
    print(f"mask_head P={P} g={g} {dtype}: rel-L2 fused {e_fused:.3e}, unfused {e_unfused:.3e}, op_tol / 2 {op_tol(dtype) / 2:.1e}")
    assert e_fused <= op_tol(dtype) / 2
    assert e_fused <= 2 * e_unfused


def test_mask_head_one_hot_token_lands_on_its_4x4_block():
    P, g, dtype = 2, 8, torch.bfloat16
    o = _head_operands(P, g, 3, dtype, seed=9)
    x = o["x"]
    o["x"] = torch.zeros_like(x)
    zero = _head_fused(o, P, g).cpu()
    p, i, j = 1, 5, 2
    o["x"][p * g * g + i * g + j] = x[0]
    one = _head_fused(o, P, g).cpu()
    changed = (one != zero)
    want = torch.zeros_like(changed)
    want[p, :, 4 * i:4 * i + 4, 4 * j:4 * j + 4] = True
    assert bool((changed & ~want).sum() == 0), "a pixel outside the token's block moved"
    assert int(changed[p, :, 4 * i:4 * i + 4, 4 * j:4 * j + 4].sum()) >= 3 * 16 - 2
    assert rel_l2(one, _head64(o, P, g)) <= op_tol(dtype) / 2


# ---- mask post-processing ------------------------------------------------------------------------------------------------------------------
POST_CASES = [(32, 128, (128, 128), (64, 64)), (32, 128, (96, 128), (48, 64)), (256, 1024, (682, 1024), (333, 500))]


def _logits(kind, L, seed):
    gen = torch.Generator().manual_seed(seed)
    if kind == "noise":
        return torch.randn(1, 3, L, L, generator=gen).float().contiguous()
    y, x = torch.meshgrid(torch.arange(L, dtype=torch.float64), torch.arange(L, dtype=torch.float64), indexing="ij")
    ph = torch.rand(3, 4, generator=gen).double() * 6.28
    out = torch.stack([torch.sin(2 * np.pi * (1 + m) * y / L + ph[m, 0]) * torch.cos(2 * np.pi * 1.5 * x / L + ph[m, 1]) + 0.3 * torch.sin(2 * np.pi * 3 * (x + y) / L + ph[m, 2])
                       for m in range(3)])
    return (4 * out)[None].float().contiguous()


@pytest.mark.parametrize("kind", ["noise", "smooth"])
@pytest.mark.parametrize("L,S,resh,orig", POST_CASES, ids=["64x64", "48x64-crop", "333x500"])
def test_mask_post_equals_fp64_away_from_the_threshold_and_the_float_resize_exactly(L, S, resh, orig, kind):
    from tests import sam_post_reference as R
    from theatergen_amd import ops
    lg = _logits(kind, L, seed=L + orig[0])
    vals = R.post_values(lg, S, resh, orig)
    mask, areas = ops.sam_mask_post(lg.to(DEV), S, resh, orig, orig)
    mask, areas = mask.cpu(), areas.cpu()
    assert mask.dtype == torch.uint8 and mask.shape == (1, 3) + tuple(orig) and areas.dtype == torch.int32 and areas.shape == (1, 3)
    assert set(mask.unique().tolist()) <= {0, 1}
    sure = vals.abs() > 1e-5 * float(lg.abs().max())
    excluded = 1.0 - float(sure.double().mean())
    wrong = int(((mask.bool() != (vals > 0)) & sure).sum())
    print(f"mask_post {kind} {orig}: excluded share {excluded:.2e}, wrong among the rest {wrong}")
    assert excluded <= 1e-3
    assert wrong == 0
    assert torch.equal(areas.long(), mask.long().sum((-1, -2)))
    h0, w0 = orig
    for target in [(h0 // 8, w0 // 8), (int(h0 / 3.3), int(w0 / 2.7)), (h0 + h0 // 2 + 1, 2 * w0 + 3)]:
        m_t, a_t = ops.sam_mask_post(lg.to(DEV), S, resh, orig, target)
        m_t, a_t = m_t.cpu(), a_t.cpu()
        assert torch.equal(m_t.bool(), R.resize_bool(mask, target)), f"target {target}"
        assert torch.equal(a_t.long(), m_t.long().sum((-1, -2))), f"areas at target {target}"


# ---- the decoder end to end ----------------------------------------------------------------------------------------------------------------
def _golden_model(tag, dtype):
    import make_sam_decoder_golden as G
    from theatergen_amd.sam_decoder import SamModel, sam_decoder_config
    c = G.CASES[tag]
    gold = np.load(os.path.join(HERE, "golden", f"sam_decoder_{tag}.npz"))
    w = G.make_weights(c["g"], c["seed"])
    assert np.allclose(G.weight_checksums(w), gold["weight_checksums"], rtol=1e-12, atol=0), "make_weights drifted from the stored goldens"
    model = SamModel.from_state_dict(None, {k: torch.from_numpy(v) for k, v in w.items()}, device=DEV, dtype=dtype, decoder_config=sam_decoder_config(c["g"]))
    emb = torch.from_numpy(G.make_embeddings(c["g"], c["seed"], gold["boxes"].shape[0])).to(DEV, dtype)
    return G, model, emb, gold


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tag", ["g16", "g64"])
def test_decoder_within_three_times_the_rounding_floor_and_below_autocast(tag, dtype):
    G, model, emb, gold = _golden_model(tag, dtype)
    out = model(image_embeddings=emb, input_boxes=gold["boxes"])
    pm, iou = out.pred_masks.float().cpu().numpy(), out.iou_scores.float().cpu().numpy()
    assert out.pred_masks.dtype == torch.float32 and pm.shape == gold["pred_masks"].shape and iou.shape == gold["iou_scores"].shape
    name = str(dtype).split(".")[-1]
    err = G.errors(pm, iou, gold["pred_masks"].astype(np.float64), gold["iou_scores"].astype(np.float64))
    floor, autocast = gold["floor_" + name], gold["autocast_" + name]
    print(f"decoder {tag} {name}: [pred_masks rel-L2, iou rel-L2, sign flips] measured {err}, floor {floor}, autocast {autocast}")
    _record(dict(case=tag, dtype=name, measured=err.tolist(), floor=floor.tolist(), autocast=autocast.tolist()))
    assert (err <= 3 * floor).all(), f"measured {err} against 3 x floor {3 * floor}"
    assert (err < autocast).all(), f"measured {err} against the autocast route {autocast}"
    single = model(image_embeddings=emb, input_boxes=gold["boxes"], multimask_output=False)
    assert single.pred_masks.shape[2] == 1 and single.iou_scores.shape[2] == 1


def test_refused_arguments():
    G, model, emb, gold = _golden_model("g16", torch.bfloat16)
    for name in ("input_masks", "attention_similarity", "target_embedding"):
        with pytest.raises(NotImplementedError, match=name):
            model(image_embeddings=emb, input_boxes=gold["boxes"], **{name: torch.zeros(1)})


# ---- the call surface ----------------------------------------------------------------------------------------------------------------------
class _StubProcessor:
    """images: uint8 arrays [h, w, 3] whose pixel (0, 0, 0) is the image's tag.  pixel_values [B, 3, S, S] carry the tag; the sizes are the processor's."""

    def __init__(self, S):
        self.S, self.calls = S, 0
        self.image_processor = SimpleNamespace(post_process_masks=self._post)
        self.post_calls = 0

    def __call__(self, images, input_points=None, input_boxes=None, return_tensors="pt"):
        self.calls += 1
        images = images if isinstance(images, list) else [images]
        orig = [im.shape[:2] for im in images]
        resh = [(int(h * self.S / max(h, w) + 0.5), int(w * self.S / max(h, w) + 0.5)) for h, w in orig]
        pv = torch.stack([torch.full((3, self.S, self.S), float(im[0, 0, 0])) for im in images])
        out = {"pixel_values": pv, "original_sizes": torch.tensor(orig), "reshaped_input_sizes": torch.tensor(resh)}
        if input_boxes is not None:
            out["input_boxes"] = torch.tensor(input_boxes, dtype=torch.float64)
        return out

    def _post(self, masks, original_sizes, reshaped_input_sizes):
        self.post_calls += 1
        return [torch.zeros((m.shape[0], m.shape[1]) + tuple(int(v) for v in o), dtype=torch.bool) for m, o in zip(masks, original_sizes)]


def _surface_dict(dtype=torch.bfloat16):
    import make_sam_decoder_golden as G
    from theatergen_amd.sam_decoder import SamModel, sam_decoder_config
    g = 8
    w = G.make_weights(g, 808)
    model = SamModel.from_state_dict(None, {k: torch.from_numpy(v) for k, v in w.items()}, device=DEV, dtype=dtype, decoder_config=sam_decoder_config(g))
    table = torch.randn(8, 256, g, g, generator=torch.Generator().manual_seed(3)).to(DEV, dtype)
    calls = {"encoder": 0}

    def encoder(pixel_values):
        calls["encoder"] += 1
        return table[pixel_values[:, 0, 0, 0].long()].contiguous()
    encoder.device = torch.device(DEV)
    return {"sam_model": model, "sam_processor": _StubProcessor(16 * g), "sam_encoder": encoder}, calls


def _image(tag, h=48, w=64):
    im = np.zeros((h, w, 3), np.uint8)
    im[0, 0, 0] = tag
    return im


def test_sam_device_route_returns_the_documented_structure():
    from theatergen_amd import sam as S
    md, calls = _surface_dict()
    masks, conf = S.sam(md, _image(1), input_boxes=[[[4, 6, 40, 30], [10, 2, 60, 44]]], target_mask_shape=(6, 8))
    assert isinstance(masks, list) and len(masks) == 1 and isinstance(masks[0], np.ndarray) and masks[0].dtype == np.bool_ and masks[0].shape == (2, 3, 6, 8)
    assert isinstance(conf, np.ndarray) and conf.dtype == np.float32 and conf.shape == (3,)
    masks_t, _ = S.sam(md, _image(1), input_boxes=[[[4, 6, 40, 30], [10, 2, 60, 44]]], target_mask_shape=(48, 64), return_numpy=False)
    assert isinstance(masks_t[0], torch.Tensor) and masks_t[0].dtype == torch.bool and masks_t[0].shape == (2, 3, 48, 64) and not masks_t[0].is_cuda
    assert md["sam_processor"].calls == 2 and calls["encoder"] == 2 and md["sam_processor"].post_calls == 0
    pm, _ = S.sam_point_input(md, _image(2), input_points=[[[[20, 20], [30, 10]]]], target_mask_shape=(48, 64))
    assert pm[0].shape == (1, 3, 48, 64)


def test_refine_characters_equals_single_calls_bit_for_bit():
    from theatergen_amd import sam as S
    md, calls = _surface_dict()
    images, boxes = [_image(1), _image(5)], [[[4, 6, 40, 30]], [[12.5, 3, 50, 47]]]
    both = S.sam_refine_characters(images, boxes, md, 48, 64, 0.85, 0.2)
    assert md["sam_processor"].calls == 1 and calls["encoder"] == 1
    for i in range(2):
        one = S.sam_refine_attn(boxes[i], 0, images[i], None, md, 48, 64, None, None, False, None, None, None, None, 0.85, 0.2, False)
        assert one[0].shape == (6, 8) and one[2].shape == (48, 64) and one[0].dtype == np.bool_
        for k in range(4):
            assert np.array_equal(np.asarray(both[k][i]), np.asarray(one[k])), f"character {i}, output {k}"
    assert md["sam_processor"].calls == 3 and calls["encoder"] == 3


def test_a_transformers_style_model_still_takes_the_old_path():
    from theatergen_amd import sam as S
    md, calls = _surface_dict()
    seen = {}

    def foreign(image_embeddings=None, **kw):
        seen.update(kw, emb=image_embeddings)
        B = image_embeddings.shape[0]
        return SimpleNamespace(pred_masks=torch.zeros(B, 1, 3, 32, 32, device=DEV), iou_scores=torch.full((B, 1, 3), 0.5, device=DEV))
    md["sam_model"] = foreign
    masks, conf = S.sam(md, _image(1), input_boxes=[[[4, 6, 40, 30]]], target_mask_shape=(6, 8))
    assert "input_boxes" in seen and md["sam_processor"].post_calls == 1 and calls["encoder"] == 1
    assert masks[0].shape == (1, 3, 6, 8) and conf.shape == (3,)
