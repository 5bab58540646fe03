"""GPU: ``tg_dino_contrastive`` and ``tg_dino_box_update`` against the fp64 restatements of their contracts and the bounds derived in
tests/dino_head_reference.py; ``GroundingDinoDecoderHead`` against the transformers golden (tests/golden/make_grounding_dino_decoder_golden.py); the
attached model, ``GroundingDinoDetector`` and ``detect`` against the same tiny model in fp32.

Outputs are sentinel-filled before every launch and operand padding is NaN.  The decoder's bound per quantity is TWICE the stored error of the rounded
emulation, as for the encoder.  Queries are matched by proposal index before any comparison.  Where the golden has ``embedding_init_target`` the content
query belongs to the RANK of a proposal and scores a rounding apart swap ranks, so the states are compared with the golden's rank order passed in
(``topk_proposals``); the head's own selection is checked as a set, with its initial boxes, in a run of its own.
"""
import copy
import functools

import numpy as np
import pytest
import torch

from tests import dino_head_reference as DR
from tests import parity_metrics as pm
from tests.golden import make_grounding_dino_decoder_golden as G
from tests.golden import make_grounding_dino_encoder_golden as GE

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
MANT = {"bf16": 7, "f16": 10}
SENTINEL = 12345.0


# ---- tg_dino_contrastive -----------------------------------------------------------------------------------------------------------------------------
def _padded(a, pitch, dt):
    """[.., rows, d] host array -> device view [.., rows, d] of a NaN-filled buffer with row pitch ``pitch``"""
    buf = torch.full(a.shape[:-1] + (pitch,), float("nan"), dtype=dt, device="cuda")
    buf[..., :a.shape[-1]] = torch.from_numpy(a).to(dt)
    return buf[..., :a.shape[-1]]


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("i", range(len(DR.CONTRASTIVE_CASES)), ids=DR.CONTRASTIVE_IDS)
def test_contrastive_against_fp64_contract(i, dname):
    """Measured: the largest error is 0.001 - 0.005 of the bound in every case."""
    from theatergen_amd import ops
    case, dt = DR.CONTRASTIVE_CASES[i], DTYPES[dname]
    n, Lt, T, d, qp, tp, B, _ = case
    q, text, mask = DR.make_contrastive_case(case, dt, 300 + i)
    want, want_max, bound = DR.contrastive_reference(q, text, mask, T)
    qd, td, md = _padded(q, qp, dt), _padded(text, tp, dt), torch.from_numpy(mask).cuda()
    logits = torch.full((B, n, T), SENTINEL, device="cuda")
    row_max = torch.full((B, n), SENTINEL, device="cuda")
    ops.dino_contrastive(qd, td, md, T, logits=logits, row_max=row_max)
    only_max = ops.dino_contrastive(qd, td, md.bool(), T, logits=False, row_max=True)[1]
    only_logits = ops.dino_contrastive(qd, td, md, T, logits=True, row_max=False)[0]
    again = ops.dino_contrastive(qd, td, md, T)[0]
    item0 = ops.dino_contrastive(qd[:1], td[:1], md[:1], T, logits=True, row_max=True)
    torch.cuda.synchronize()
    got, got_max = logits.double().cpu().numpy(), row_max.double().cpu().numpy()
    assert np.array_equal(np.isneginf(got), np.isneginf(want)) and not np.isnan(got).any()           # the -inf pattern, exactly; no sentinel, no NaN
    fin = np.isfinite(want)
    excess = (np.abs(got[fin] - want[fin]) / bound[fin]).max() if fin.any() else 0.0
    print(f"dino_contrastive {dname} {DR.CONTRASTIVE_IDS[i]}: largest error / bound {excess:.3f}")
    assert excess <= 1.0
    assert torch.equal(row_max, logits.max(-1).values)                                               # bit-equal to the row maximum of the same call
    assert np.array_equal(np.isneginf(got_max), np.isneginf(want_max))
    assert torch.equal(only_max, row_max) and torch.equal(only_logits, logits) and torch.equal(again, logits)
    assert torch.equal(item0[0], logits[:1]) and torch.equal(item0[1], row_max[:1])                  # an item does not depend on the batch


# ---- tg_dino_box_update ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("i", range(len(DR.BOX_CASES)), ids=DR.BOX_IDS)
def test_box_update_against_fp64_contract(i, dname):
    """Measured, largest error / bound: ref 0.001 - 0.014, ref_levels 0.002 - 0.019, pos_in 0.69 - 0.99 (the one storage rounding reaches its half ulp)."""
    from theatergen_amd import ops
    case, dt = DR.BOX_CASES[i], DTYPES[dname]
    rows, B, L, d, hp, mode = case
    h, w3, b3, prior, vr = DR.make_box_case(case, dt, 400 + i)
    is_box = mode == "box"
    want = DR.box_update_reference(h, w3, b3, prior, is_box, vr, rows // B, MANT[dname])
    hd, w3d = _padded(h, hp, dt), torch.from_numpy(w3).to(dt).cuda()
    b3d, pd, vrd = torch.from_numpy(b3).cuda(), torch.from_numpy(prior).cuda(), torch.from_numpy(vr).cuda()
    ref = torch.full((rows, 4), SENTINEL, device="cuda")
    lev = torch.full((rows, L, 4), SENTINEL, device="cuda")
    pos_buf = torch.full((rows, 2 * d + 8), SENTINEL, dtype=dt, device="cuda")
    ops.dino_box_update(hd, w3d, b3d, pd, is_box, rows // B, vrd, ref=ref, ref_levels=lev, pos_in=pos_buf[:, :2 * d])
    alone = ops.dino_box_update(hd, w3d, b3d, pd, is_box)                                            # each optional output may be absent
    lev_only = ops.dino_box_update(hd, w3d, b3d, pd, is_box, rows // B, vrd, ref_levels=True)
    pos_only = ops.dino_box_update(hd, w3d, b3d, pd, is_box, rows // B, vrd, pos_in=True)
    torch.cuda.synchronize()
    assert alone[1] is None and alone[2] is None and lev_only[2] is None and pos_only[1] is None
    assert torch.equal(alone[0], ref) and torch.equal(lev_only[0], ref) and torch.equal(lev_only[1], lev)
    assert torch.equal(pos_only[0], ref) and torch.equal(pos_only[2], pos_buf[:, :2 * d])
    assert bool((pos_buf[:, 2 * d:] == torch.tensor(SENTINEL, dtype=dt)).all())                                      # nothing past 2 d of a row is written
    for name, t in (("ref", ref), ("ref_levels", lev), ("pos_in", pos_buf[:, :2 * d])):
        g = t.double().cpu().numpy()
        val, bound = want[name]
        assert not np.isnan(g).any()
        excess = (np.abs(g - val) / np.maximum(bound, 1e-300))[bound > 0].max()
        print(f"dino_box_update {dname} {DR.BOX_IDS[i]} {name}: largest error / bound {excess:.3f}")
        assert excess <= 1.0, name
        assert np.array_equal(g[bound == 0], val[bound == 0])                                        # prior = +inf: exactly 1 (and its level boxes exact)
    if not is_box:
        assert bool((ref[torch.isposinf(pd)] == 1.0).all())


# ---- the decoder head against the golden ---------------------------------------------------------------------------------------------------------------
def _head(which, dname):
    from theatergen_amd.grounding_dino_decoder import GroundingDinoDecoderHead
    w = {k: torch.from_numpy(v) for k, v in G.make_weights(which).items()}
    return GroundingDinoDecoderHead.from_state_dict(G.config(which), w, "cuda", DTYPES[dname])


def _head_args(which, dname):
    kw = G.inputs(which)
    return (kw["memory"].to(DTYPES[dname]).cuda(), kw["valid"].cuda(), kw["text"].to(DTYPES[dname]).cuda(), kw["token_mask"].cuda(), list(G.SHAPES),
            kw["valid_ratios"].cuda())


def _sorted(out, which):
    """the head's outputs with every item's queries sorted by proposal index, as the golden stores them"""
    order = torch.argsort(out.topk_proposals, dim=1)
    take = lambda t, dim: torch.stack([t[b].index_select(dim - 1, order[b]) for b in range(t.shape[0])]).float().cpu()      # noqa: E731
    got = {"topk_sorted": take(out.topk_proposals, 1), "logits": take(out.logits, 1), "pred_boxes": take(out.pred_boxes, 1),
           "ref0": take(out.init_reference_points, 1)}
    for i in range(out.intermediate_hidden_states.shape[1]):
        got[f"hidden{i}"] = take(out.intermediate_hidden_states[:, i], 1)
        got[f"refs{i}"] = take(out.intermediate_reference_points[:, i], 1)
    return got


@functools.lru_cache(maxsize=None)
def _head_run(which, dname):
    """per config and dtype: the head's own selection (free run) and, for the config whose content queries go by rank, a run with the golden's rank order;
    each forward twice (the replay must be bit-equal)"""
    z = np.load(G.PATH)
    head, args = _head(which, dname), _head_args(which, dname)
    free = head(*args)
    free2 = head(*args)
    pin = torch.from_numpy(z[f"{which}_topk"]).cuda() if G.CONFIGS[which]["embedding_init_target"] else None
    pinned = head(*args, topk_proposals=pin) if pin is not None else free
    torch.cuda.synchronize()
    for name in ("logits", "pred_boxes", "topk_proposals", "intermediate_hidden_states", "intermediate_reference_points"):
        assert torch.equal(getattr(free, name), getattr(free2, name)), name                         # a second forward replays bit-equal
    return _sorted(free, which), _sorted(pinned, which), z, head.op_calls


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("which", list(G.CONFIGS))
def test_head_selects_the_golden_set(which, dname):
    """the head's own top-k: the SET of proposals equals the golden's, and their initial boxes (matched by proposal) are inside the bound"""
    free, _, z, _ = _head_run(which, dname)
    assert np.array_equal(free["topk_sorted"].numpy(), z[f"{which}_topk_sorted"])
    if which == "main":
        emu = z[f"emu_{dname}_main_ref0"]
        pm.check(free["ref0"], torch.from_numpy(z["main_ref0"]), f"decoder head {dname} ref0", 2 * float(emu[0]), 2 * float(emu[1]))


def _check(got, want, emu, label):
    want = torch.from_numpy(want)
    fin = torch.isfinite(want)
    assert torch.equal(torch.isneginf(got), torch.isneginf(want)) and not torch.isnan(got).any(), label
    m = pm.metrics(got[fin], want[fin])
    print(f"{label}: rel-L2 {m['rel_l2']:.3e} max {m['max_rel']:.3e} (emulation {emu[0]:.3e} / {emu[1]:.3e}, bound twice that)")
    pm.check(got[fin], want[fin], label, 2 * float(emu[0]), 2 * float(emu[1]))


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("name", list(G.quantities("main")))
def test_head_against_transformers_golden(name, dname):
    """Initial boxes, per layer the normed states and the boxes after it, final logits and boxes, with the golden's rank order.  Measured rel-L2, device
    (emulation): bf16 states 5.9e-3 (5.9e-3) / 8.2e-3 (8.1e-3), logits 8.8e-3 (8.7e-3), pred_boxes 4.9e-4 (4.6e-4), initial boxes 1.3e-4 (1.3e-4); f16 states
    4.8e-4 (4.8e-4) / 6.5e-4 (6.5e-4), logits 6.3e-4 (6.4e-4), pred_boxes 2.9e-5 (2.5e-5); maxima 0.75 - 1.4 x the emulation's
    (profiles/grounding_dino_decoder_findings.md)."""
    _, pinned, z, _ = _head_run("main", dname)
    _check(pinned[name], z[f"main_{name}"], z[f"emu_{dname}_main_{name}"], f"decoder head {dname} {name}")


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("name", list(G.quantities("gathered")))
def test_head_with_gathered_targets_against_golden(name, dname):
    free, _, z, _ = _head_run("gathered", dname)
    _check(free[name], z[f"gathered_{name}"], z[f"emu_{dname}_gathered_{name}"], f"decoder head (gathered targets) {dname} {name}")


@pytest.mark.parametrize("dname", list(DTYPES))
def test_free_run_is_the_run_pinned_to_its_own_order(dname):
    """What a caller gets from a free run on a model whose query embeddings differ (the main config): exactly the forward of ITS OWN rank order — pinning
    the head to the order it chose itself replays the free run bit for bit, so ``topk_proposals`` changes nothing but where the order comes from.  Against
    the fp32 golden such a run differs by the content queries of the proposals whose ranks a rounding swapped: their number and the resulting distance of
    the boxes (matched by proposal) are printed, not asserted — the distance is that of another, equally valid, assignment of content queries."""
    z = np.load(G.PATH)
    head, args = _head("main", dname), _head_args("main", dname)
    free = head(*args)
    own = head(*args, topk_proposals=free.topk_proposals.clone())
    torch.cuda.synchronize()
    for name in ("logits", "pred_boxes", "intermediate_hidden_states", "intermediate_reference_points", "init_reference_points"):
        assert torch.equal(getattr(free, name), getattr(own, name)), name
    swapped = int((free.topk_proposals.cpu() != torch.from_numpy(z["main_topk"])).sum())
    m = pm.metrics(_sorted(free, "main")["pred_boxes"], torch.from_numpy(z["main_pred_boxes"]))
    print(f"free run {dname}: {swapped} of {free.topk_proposals.numel()} ranks differ from the fp32 order; pred_boxes by proposal rel-L2 {m['rel_l2']:.3e} "
          f"max {m['max_rel']:.3e}")


def test_head_refuses_output_attentions_and_tallies_calls():
    head, args = _head("main", "bf16"), _head_args("main", "bf16")
    with pytest.raises(NotImplementedError, match="output_attentions"):
        head(*args, output_attentions=True)
    assert head.op_calls == 0
    head.taps = []
    head(*args)
    assert head.op_calls > 0 and [t[0] for t in head.taps] == ["select", "layer", "layer"]


# ---- the whole model -----------------------------------------------------------------------------------------------------------------------------------
# A tiny GroundingDinoForObjectDetection (the encoder fixture's backbone and image: 992 tokens) in fp32 on the device is the reference.  Behind a bf16 /
# fp16 front and encoder the proposal scores move by more than the gaps between them, so neither the selected set nor the rank order of a selection would
# be the fp32 model's.  The model therefore takes EVERY token (num_queries = 992) and its query_position_embeddings rows are all equal: the decoder is then
# permutation-equivariant and queries are matched by proposal index.  (The selection itself and the rank -> content query assignment are what the golden
# tests above check.)  Bound per output and metric (rel-L2, max-rel), from stored figures only:
#     gain x (bound of what enters the head) + 2 x the decoder fixture's emulation error of the output
# where the gain is the fixture's ``main_input_gain_{output}`` — the output's error per unit of error of the encoder's outputs, from an fp32 rerun with
# perturbed memory and text (1.15 / 1.25 for logits, 0.034 / 0.053 for boxes: a sigmoid coordinate passes little of it on) — and what enters the head is
# bounded by the front's ``golden_tol`` for its projected levels (tol / 2 rel-L2, tol max; imported) plus the encoder fixture's bound for its last layer.
# ``detect``'s pixel tolerance is the boxes' max bound times the image side.
def _tiny_config():
    c = G.config("main")
    c.num_queries = G.NV
    c.encoder_layers = GE.LAYERS
    return c


def _by_proposal(scores, *tensors):
    order = torch.argsort(torch.topk(scores, scores.shape[1], dim=1)[1], dim=1)
    return [torch.stack([t[b].index_select(0, order[b]) for b in range(t.shape[0])]).float().cpu() for t in tensors]


@functools.lru_cache(maxsize=None)
def _model_runs(dname):
    from transformers import GroundingDinoForObjectDetection
    from theatergen_amd.detector import GroundingDinoDetector
    from theatergen_amd.grounding_dino import GroundingDinoVisionFront
    from theatergen_amd.grounding_dino_decoder import GroundingDinoDecoderHead
    from theatergen_amd.grounding_dino_encoder import GroundingDinoFusionEncoder
    torch.manual_seed(0)
    model = GroundingDinoForObjectDetection(_tiny_config()).eval().float()
    w = {"model." + k: v for k, v in GE.make_weights().items()}
    w.update(G.make_weights("main", shapes=G.taken_shapes(model)))
    w["model.query_position_embeddings.weight"] = np.repeat(w["model.query_position_embeddings.weight"][:1], G.NV, 0)
    sd = {k: torch.from_numpy(v) for k, v in w.items()}
    sd.update({"model.decoder." + k: v for k, v in sd.items() if k.startswith("bbox_embed.")})
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and not any(k in sd for k in missing)
    model = model.to("cuda")
    gen = torch.Generator().manual_seed(9)
    pv = torch.randn((G.BATCH, 3) + GE.IMAGE_HW, generator=gen)
    mask = torch.ones((G.BATCH,) + GE.IMAGE_HW, dtype=torch.long)
    mask[1, GE.MASK_HW[0]:, :] = 0
    mask[1, :, GE.MASK_HW[1]:] = 0
    ids = torch.tensor(G.INPUT_IDS)
    cpu_kw = dict(pixel_values=pv, pixel_mask=mask, input_ids=ids, attention_mask=(ids != 0).long(), token_type_ids=torch.zeros_like(ids))
    kw = {k: v.cuda() for k, v in cpu_kw.items()}
    dt = DTYPES[dname]
    with torch.no_grad():
        ref = model(**kw)
        ref_out = _by_proposal(ref.enc_outputs_class.max(-1)[0], ref.logits, ref.pred_boxes)
        detector = GroundingDinoDetector.from_hf(model, dt)                                          # before attach: it reads the model's own weights
        d1 = detector(**cpu_kw)
        d2 = detector(**cpu_kw)
        with pytest.raises(NotImplementedError, match="output_attentions"):
            detector(**cpu_kw, output_attentions=True)
        fp32 = copy.deepcopy(model)                                                                 # the reference survives the attach below
        sd = model.state_dict()
        parts = (GroundingDinoVisionFront.from_state_dict(model.config, sd, "cuda", dt), GroundingDinoFusionEncoder.from_state_dict(model.config, sd, "cuda", dt),
                 GroundingDinoDecoderHead.from_state_dict(model.config, sd, "cuda", dt))
        for p in parts:
            p.attach(model)
        att = model(**kw)
        assert att.logits.dtype == torch.float32 and att.last_hidden_state.dtype == torch.float32
        att_out = _by_proposal(att.enc_outputs_class.max(-1)[0], att.logits, att.pred_boxes)
        torch.cuda.synchronize()
    assert torch.equal(d1.logits, d2.logits) and torch.equal(d1.pred_boxes, d2.pred_boxes)          # a second forward replays bit-equal
    assert (detector.cache_hits, detector.cache_misses) == (1, 1)                                   # ... from the caption cache
    order = torch.argsort(d1.topk_proposals, dim=1)
    det_out = [torch.stack([t[b].index_select(0, order[b]) for b in range(G.BATCH)]).float().cpu() for t in (d1.logits, d1.pred_boxes)]
    return ref_out, att_out, det_out, (fp32, detector)


def _model_bound(dname, name):
    from tests.test_grounding_dino_vision_gpu import golden_tol
    ze, zd = np.load(GE.PATH), np.load(G.PATH)
    front, e, d, g = golden_tol(DTYPES[dname]), ze[f"emu_{dname}_layer1_vision"], zd[f"emu_{dname}_main_{name}"], zd[f"main_input_gain_{name}"]
    enters = (front / 2 + 2 * float(e[0]), front + 2 * float(e[1]))
    return float(g[0]) * enters[0] + 2 * float(d[0]), float(g[1]) * enters[1] + 2 * float(d[1])


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("route", ["attached", "detector"])
def test_whole_model_matches_transformers_fp32(route, dname):
    """Measured rel-L2 / max (bound): bf16 logits 1.8e-2 / 2.6e-2 attached, 2.2e-2 / 3.4e-2 detector (5.5e-2 / 9.8e-2), boxes 4e-4 / 2.5e-3 (2.0e-3 / 5.3e-3);
    f16 logits 2.1e-3 / 5.6e-3 attached, 2.2e-3 / 4.6e-3 detector (6.4e-3 / 1.2e-2), boxes 4e-5 / 4e-4 (2.0e-4 / 5.0e-4)."""
    ref_out, att_out, det_out, _ = _model_runs(dname)
    got = att_out if route == "attached" else det_out
    for name, g, r in (("logits", got[0], ref_out[0]), ("pred_boxes", got[1], ref_out[1])):
        fin = torch.isfinite(r)
        assert torch.equal(torch.isneginf(g), torch.isneginf(r)) and not torch.isnan(g).any()
        b = _model_bound(dname, name)
        m = pm.metrics(g[fin], r[fin])
        print(f"{route} model {dname} {name}: rel-L2 {m['rel_l2']:.3e} max {m['max_rel']:.3e} (bound {b[0]:.3e} / {b[1]:.3e})")
        pm.check(g[fin], r[fin], f"{route} grounding dino {dname} {name}", *b)


class _Processor:
    """stands for the GroundingDINO processor: the fixture's ids for any word, the image scaled to [-1, 1], CPU tensors"""

    def __call__(self, images, text, return_tensors="pt", padding=False):
        images = images if isinstance(images, list) else [images]
        n = len(images)
        ids = torch.tensor(G.INPUT_IDS[:1]).repeat(n, 1)
        pv = torch.stack([torch.from_numpy(np.asarray(im, np.float32) / 127.5 - 1.0).permute(2, 0, 1) for im in images])
        return {"pixel_values": pv, "pixel_mask": torch.ones((n,) + tuple(pv.shape[-2:]), dtype=torch.long), "input_ids": ids,
                "attention_mask": (ids != 0).long(), "token_type_ids": torch.zeros_like(ids)}


@pytest.mark.parametrize("dname", list(DTYPES))
def test_detect_through_the_detector(dname):
    """``detect`` with the detector in the model's place returns the box ``select_box`` picks from the fp32 model's outputs, to within the box bound times
    the image side; ``detect_many`` returns the same list"""
    from theatergen_amd.detector import detect, detect_many, select_box
    _, _, _, (fp32, detector) = _model_runs(dname)
    rs = np.random.RandomState(5)
    H, W = GE.IMAGE_HW
    images = [rs.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(2)]
    proc = _Processor()
    gd = {"model": detector, "processor": proc}
    got = [detect(gd, "cat", im) for im in images]
    many = detect_many(gd, ["cat", "cat"], images)
    tol = _model_bound(dname, "pred_boxes")[1] * max(H, W)
    for im, (box, ok), (box_m, ok_m) in zip(images, got, many):
        kw = {k: v.cuda() for k, v in proc(im, "cat").items()}
        with torch.no_grad():
            out = fp32(**kw)
        want, want_ok = select_box(out.logits[0], out.pred_boxes[0], H, W)
        print(f"detect {dname}: {box} vs fp32 {want} (tolerance {tol:.3f} px)")
        assert ok == want_ok == ok_m and np.abs(box - want).max() <= tol and np.abs(box_m - box).max() <= tol
