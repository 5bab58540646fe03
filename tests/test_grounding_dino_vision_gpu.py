"""GPU: ``tg_attention_swin`` against the fp64 restatement of its contract (tests/swin_window_reference.py), its refusals, and
``GroundingDinoVisionFront`` against the transformers golden (tests/golden/make_grounding_dino_vision_golden.py) and inside an attached model.

Bounds: ``op_tol`` (a launch against fp64 from the stored operands) and ``golden_tol`` (a model against transformers fp32) of tests/test_sam_gpu.py.
"""
import functools

import numpy as np
import pytest
import torch

from tests import parity_metrics as pm
from tests import swin_window_reference as R
from tests.golden import make_grounding_dino_vision_golden as G

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
IDS = [f"{H}x{W}_s{s}_b{b}_h{h}" for H, W, s, b, h in R.CASES]
GUARD = 4096


def op_tol(dtype):
    return 1.5e-2 if dtype == torch.bfloat16 else 4e-3


def golden_tol(dtype):
    return 3e-2 if dtype == torch.bfloat16 else 6e-3


@functools.lru_cache(maxsize=None)
def _case(case, dname):
    """stored operands (host tensors in the storage dtype) and the fp64 reference from them: computed once per (case, dtype)"""
    H, W, shift, B, heads = case
    dt = DTYPES[dname]
    rnd = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(dt).double().numpy()
    qkv, pads, table = R.make_case(H, W, shift, B, heads, seed=H * 100 + W, round_to=rnd)
    ref = R.run_case(qkv, pads, table, H, W, shift)
    to = lambda a: torch.from_numpy(a).to(dt)
    return to(qkv), to(pads), to(table), torch.from_numpy(ref)


def _launch(qkv, pads, table, H, W, shift, heads, fill=7.0):
    """qkv [B, n, 3C] on the device -> (out [B, n, C], the guard band behind it)"""
    from theatergen_amd import ops
    B, n, C3 = qkv.shape
    C = C3 // 3
    flat = qkv.reshape(B * n, C3)
    buf = torch.full((B * n * C + GUARD,), fill, dtype=qkv.dtype, device=qkv.device)
    ops.attention_swin(flat, C3, n * C3, flat[:, C:], C3, n * C3, flat[:, 2 * C:], C3, n * C3, pads[0], pads[1], pads[2], table, B, heads, H, W, shift,
                       32 ** -0.5, buf, C, n * C)
    torch.cuda.synchronize()
    return buf[:B * n * C].reshape(B, n, C), buf[B * n * C:]


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_attention_swin_against_fp64_contract(case, dname):
    H, W, shift, B, heads = case
    dt = DTYPES[dname]
    qkv, pads, table, ref = _case(case, dname)
    dq, dp, dtb = qkv.cuda(), pads.cuda(), table.cuda()
    out, guard = _launch(dq, dp, dtb, H, W, shift, heads, fill=float("nan"))
    m = pm.metrics(out.float().cpu(), ref)
    tol = op_tol(dt)
    print(f"attention_swin {IDS[R.CASES.index(case)]} {dname}: rel-L2 {m['rel_l2']:.3e} max {m['max_rel']:.3e} (tolerance {tol / 2:.1e} / {tol:.1e})")
    assert bool(torch.isfinite(out).all()), "an output element was not written (NaN fill survives)"
    assert bool(torch.isnan(guard).all()), "the guard band after out was written"
    pm.check(out.float().cpu(), ref, f"attention_swin {case} {dname}", tol / 2, tol)
    again, _ = _launch(dq, dp, dtb, H, W, shift, heads, fill=float("nan"))
    assert torch.equal(out.view(torch.int16), again.view(torch.int16)), "two launches differ"
    if B > 1:
        one, _ = _launch(dq[1:2].contiguous(), dp, dtb, H, W, shift, heads, fill=float("nan"))
        assert torch.equal(one[0].view(torch.int16), out[1].view(torch.int16)), "batch item 1 depends on the batch"


def test_attention_swin_refusals_leave_out_untouched():
    from theatergen_amd import ops
    dt = torch.bfloat16
    H = W = 7

    def call(heads=1, hd=32, win=7, H=H, W=W, shift=0, off=0):
        C = heads * hd
        flat = torch.zeros((64 * 3 * C + 8,), dtype=dt, device="cuda")
        qkv = flat[off:off + 49 * 3 * C].reshape(49, 3 * C)
        pad = torch.zeros(C, dtype=dt, device="cuda")
        tab = torch.zeros(((2 * win - 1) ** 2, heads), dtype=dt, device="cuda")
        out = torch.full((49, C), 7.0, dtype=dt, device="cuda")
        with pytest.raises(RuntimeError) as e:
            ops.attention_swin(qkv, 3 * C, 49 * 3 * C, qkv[:, C:], 3 * C, 49 * 3 * C, qkv[:, 2 * C:], 3 * C, 49 * 3 * C, pad, pad, pad, tab, 1, heads, H, W,
                               shift, hd ** -0.5, out, C, 49 * C, head_dim=hd, window=win)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()), "a refused call wrote to out"
        return str(e.value)
    assert "error -3" in call(hd=64)
    assert "error -3" in call(win=12)
    assert "error -1" in call(H=6)
    assert "error -1" in call(shift=2)
    assert "error -1" in call(off=4)                      # q 8 bytes off a 16-byte boundary


# ---- the front against the golden ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _front(dname):
    from types import SimpleNamespace
    from theatergen_amd.grounding_dino import GroundingDinoVisionFront
    cfg = SimpleNamespace(backbone_config=dict(embed_dim=G.EMBED, depths=list(G.DEPTHS), num_heads=list(G.HEADS), window_size=7,
                                               out_indices=list(G.OUT_INDICES)), num_feature_levels=4, d_model=G.D_MODEL,
                          positional_embedding_temperature=20, position_embedding_type="sine")
    w = {k: torch.from_numpy(v) for k, v in G.make_weights().items()}
    return GroundingDinoVisionFront.from_state_dict(cfg, w, "cuda", DTYPES[dname])


@functools.lru_cache(maxsize=None)
def _front_run(dname):
    """one run of the front on the golden image per dtype, shared by the checks below"""
    front = _front(dname)
    pv = torch.from_numpy(G.golden_image()).cuda()
    mask = torch.from_numpy(G.golden_mask()).cuda()
    taps = []
    with torch.no_grad():
        front.backbone(pv, hidden_taps=taps)
    feats, pos = front(pv, mask)
    proj = front.project(feats)
    z = np.load(G.PATH)
    rows = [int(r) for r in z["rows"]]
    got = {"hidden0": taps[0][2][0, rows], "hidden1": taps[1][2][0, rows]}
    got.update({f"feature{i}": feats[i][0][0] for i in range(3)})
    got.update({f"proj{i}": proj[i][0] for i in range(4)})
    return front, mask, feats, pos, proj, {k: v.float().cpu() for k, v in got.items()}, z


QUANTITIES = ["hidden0", "hidden1", "feature0", "feature1", "feature2", "proj0", "proj1", "proj2", "proj3"]


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("name", QUANTITIES)
def test_front_against_transformers_golden(name, dname):
    """Stage-1 hidden states after block 0 / block 1, the raw feature maps and the projected levels at ``golden_tol``.
    Measured (rel-L2, bf16 / f16): hidden0 4.3e-3 / 4.5e-4, hidden1 4.8e-3 / 5.4e-4, feature0..2 7.0e-3 .. 1.0e-2 / 7.5e-4 .. 1.1e-3,
    proj0..3 8.4e-3 .. 1.2e-2 / 8.8e-4 .. 1.2e-3; transformers' own bf16 / fp16 CPU run of this model: 7.1e-3 .. 1.3e-2 / 7.7e-4 .. 1.3e-3."""
    dt = DTYPES[dname]
    got, z = _front_run(dname)[5], _front_run(dname)[6]
    tol = golden_tol(dt)
    m = pm.metrics(got[name], torch.from_numpy(z[name]))
    print(f"grounding dino front {dname} {name}: rel-L2 {m['rel_l2']:.3e} max {m['max_rel']:.3e} (tolerance {tol / 2:.1e} / {tol:.1e})")
    pm.check(got[name], torch.from_numpy(z[name]), f"grounding dino front {dname} {name}", tol / 2, tol)


@pytest.mark.parametrize("dname", list(DTYPES))
def test_front_masks_and_position_embeddings(dname):
    """masks equal; position embeddings within 1e-5 max abs (fp32 sin / cos of arguments <= 2 pi, ten times the rounding of the argument)"""
    dt = DTYPES[dname]
    front, mask, feats, pos, proj, _, z = _front_run(dname)
    # the three backbone levels from forward, the extra level as GroundingDinoModel.forward builds it
    m3 = front.level_mask(mask, proj[3].shape[-2:])
    masks = [m for _, m in feats] + [m3]
    pos = list(pos) + [front.position_embedding(proj[3], m3)]
    for i in range(4):
        assert np.array_equal(masks[i][0].cpu().numpy(), z[f"mask{i}"]), f"mask {i}"
    # the stored embeddings are fp32; ours are rounded to the model dtype last, so compare before that rounding
    for i in range(4):
        p32 = front.position_embedding(torch.empty(0, dtype=torch.float32), masks[i])
        err = float((p32[0].cpu() - torch.from_numpy(z[f"pos{i}"])).abs().max())
        print(f"grounding dino front {dname} pos{i}: max abs {err:.2e}")
        assert err <= 1e-5, (i, err)
        assert torch.equal(pos[i], p32.to(dt))


@pytest.mark.parametrize("dname", list(DTYPES))
def test_project_level_takes_a_tensor_that_is_not_the_last_forwards(dname):
    """``project_level`` on a fresh NCHW tensor of a feature map's shape, allocated after the forward's feature maps are dropped (the allocator may hand
    out the very same block), is the projection of THAT tensor; so is a feature map that was modified in place."""
    dt = DTYPES[dname]
    front = _front(dname)
    pv = torch.from_numpy(G.golden_image()).cuda()
    mask = torch.from_numpy(G.golden_mask()).cuda()
    feats, _ = front(pv, mask)
    shape, kept = tuple(feats[1][0].shape), feats[2][0]
    own = front.project_level(2, kept).clone()
    del feats
    gen = torch.Generator(device="cuda").manual_seed(3)
    fresh = torch.randn(shape, device="cuda", generator=gen).to(dt)
    ref_fresh = front.project_level(1, fresh.clone().contiguous())           # the uncached route by construction: a copy nobody handed out
    got_fresh = front.project_level(1, fresh)
    assert torch.equal(got_fresh, ref_fresh)
    again = front.project_level(2, kept)                                     # still the last forward's map, unmodified: same bits by either route
    assert torch.equal(again, own)
    kept.copy_(torch.randn(tuple(kept.shape), device="cuda", generator=gen).to(dt))
    want = front.project_level(2, kept.clone())
    assert torch.equal(front.project_level(2, kept), want), "a feature map modified in place was projected from its old tokens"
    assert not torch.equal(want, own)
    feats2, _ = front(pv, mask)                                              # and a new forward after the old maps are gone
    del kept
    other = torch.randn(tuple(feats2[0][0].shape), device="cuda", generator=gen).to(dt)
    first = front.project_level(0, feats2[0][0])
    assert not torch.equal(front.project_level(0, other), first)


def test_attention_swin_wrapper_checks_buffers():
    """the wrapper knows the tensors the C entry point cannot: dtype, device, extent, overlapping batch items"""
    from theatergen_amd import ops
    dt = torch.bfloat16
    n, C = 49, 32
    qkv = torch.zeros((2 * n, 3 * C), dtype=dt, device="cuda")
    pad, tab = torch.zeros(C, dtype=dt, device="cuda"), torch.zeros((169, 1), dtype=dt, device="cuda")

    def call(out, batch=2, out_bs=n * C, k=None):
        k = qkv[:, C:] if k is None else k
        ops.attention_swin(qkv, 3 * C, n * 3 * C, k, 3 * C, n * 3 * C, qkv[:, 2 * C:], 3 * C, n * 3 * C, pad, pad, pad, tab, batch, 1, 7, 7, 0, 32 ** -0.5,
                           out, C, out_bs)
    good = torch.full((2 * n, C), 7.0, dtype=dt, device="cuda")
    call(good)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(good).all()) and not bool((good == 7.0).any())
    for kw in (dict(out=torch.full((2 * n, C), 7.0, dtype=torch.float16, device="cuda")),            # another dtype
               dict(out=torch.full((2 * n - 1, C), 7.0, dtype=dt, device="cuda")),                   # one row short
               dict(out=torch.full((2 * n, C), 7.0, dtype=dt, device="cuda"), out_bs=0),            # both items on the same rows
               dict(out=torch.full((2 * n, C), 7.0, dtype=dt, device="cuda"), out_bs=-n * C),
               dict(out=torch.full((2 * n, C), 7.0, dtype=dt, device="cuda"), k=torch.zeros((n, 3 * C), dtype=dt, device="cuda"))):     # k one item short
        with pytest.raises(RuntimeError, match="attention_swin"):
            call(**kw)
        torch.cuda.synchronize()
        assert bool((kw["out"] == 7.0).all())


def test_front_refuses_a_stage_below_the_window():
    front = _front("bf16")
    with pytest.raises(ValueError, match="smaller than the window"):
        front.backbone(torch.zeros(1, 3, 112, 224, device="cuda"))            # 28 x 56 tokens: stage 4 would be 4 x 7


@pytest.mark.parametrize("dname", list(DTYPES))
def test_attached_model_matches_transformers(dname):
    """A tiny fp32 ``GroundingDinoForObjectDetection`` on the device with and without ``attach`` (front in ``dname``), same ``input_ids``.
    transformers initialises the last layer of every ``bbox_embed`` to zero, which would make the boxes the selected queries' reference points whatever
    the decoder sees; here those layers get seeded non-zero weights, so ``pred_boxes`` carries the decoder's output behind the front."""
    pytest.importorskip("transformers")
    from transformers import GroundingDinoForObjectDetection
    from theatergen_amd.grounding_dino import GroundingDinoVisionFront
    dt = DTYPES[dname]
    torch.manual_seed(0)
    model = GroundingDinoForObjectDetection(G.config(decoder_layers=2)).eval()
    w = G.make_weights()
    missing, unexpected = model.load_state_dict({"model." + k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
    assert not unexpected
    gen = torch.Generator().manual_seed(7)
    n_box = 0
    with torch.no_grad():
        for name, prm in model.named_parameters():
            if "bbox_embed" in name and ".layers.2." in name:                # the zero-initialised output layer of a box head
                prm.copy_(0.2 * torch.randn(prm.shape, generator=gen))
                n_box += 1
    assert n_box >= 2
    model = model.to(device="cuda")                       # fp32: transformers' deformable attention (grid_sample) does not run in half precision
    pv = torch.from_numpy(G.golden_image()).to(device="cuda")
    mask = torch.from_numpy(G.golden_mask()).cuda()
    ids = torch.tensor([[1, 17, 23, 5, 2]], device="cuda")
    kw = dict(pixel_values=pv, pixel_mask=mask, input_ids=ids, attention_mask=torch.ones_like(ids), token_type_ids=torch.zeros_like(ids))
    with torch.no_grad():
        ref = model(**kw)
        ref_logits, ref_boxes = ref.logits.float().cpu(), ref.pred_boxes.float().cpu()
        front = GroundingDinoVisionFront.from_state_dict(model.config, model.state_dict(), "cuda", dt)
        front.attach(model)
        got = model(**kw)
    tol = golden_tol(dt)
    for name, g, r in (("logits", got.logits.float().cpu(), ref_logits), ("pred_boxes", got.pred_boxes.float().cpu(), ref_boxes)):
        fin = torch.isfinite(r)
        assert torch.equal(fin, torch.isfinite(g)), f"{name}: the -inf pattern of the text mask differs"
        m = pm.metrics(torch.where(fin, g, torch.zeros_like(g)), torch.where(fin, r, torch.zeros_like(r)))
        print(f"attached model {dname} {name}: rel-L2 {m['rel_l2']:.3e} (tolerance {tol:.1e})")
        assert m["rel_l2"] <= tol, (name, m)
    assert float((ref_boxes - ref_boxes[:, :1]).abs().max()) > 1e-3, "the reference boxes do not vary: the comparison would be vacuous"
