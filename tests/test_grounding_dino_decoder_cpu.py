"""CPU: the fp64 restatements of ``tg_dino_contrastive`` and ``tg_dino_box_update`` are pinned to the ``transformers`` expressions; the decoder fixture
reproduces; names, config refusals, symbols, bindings, the refusals that need no device; ``detect`` / ``detect_many`` and the caption cache on stubs."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import dino_head_reference as DR
from tests.golden import make_grounding_dino_decoder_golden as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("i", range(len(DR.CONTRASTIVE_CASES)), ids=DR.CONTRASTIVE_IDS)
def test_contrastive_reference_is_transformers(i):
    from transformers.models.grounding_dino.modeling_grounding_dino import GroundingDinoContrastiveEmbedding
    case = DR.CONTRASTIVE_CASES[i]
    q, text, mask = DR.make_contrastive_case(case, torch.bfloat16, 300 + i)
    got, row_max, bound = DR.contrastive_reference(q, text, mask, case[2])
    want = GroundingDinoContrastiveEmbedding(SimpleNamespace(max_text_len=case[2]))(
        torch.from_numpy(q).double(), torch.from_numpy(text).double(), torch.from_numpy(mask).bool()).numpy()
    assert np.array_equal(np.isneginf(got), np.isneginf(want))
    fin = np.isfinite(want)
    assert want.dtype == np.float32                       # the module pads into a float32 tensor whatever it was given: its fp64 products rounded once
    np.testing.assert_allclose(got[fin], want[fin], rtol=2.0 ** -23, atol=0)
    assert np.array_equal(row_max, got.max(-1)) and (bound[fin] > 0).all() and (bound[~fin] == 0).all()
    if case[7] == "none1":
        assert np.isneginf(got[1]).all() and np.isneginf(row_max[1]).all()


def test_contrastive_cases_cover_the_listed_sizes():
    c = DR.CONTRASTIVE_CASES
    assert {x[0] for x in c} == {1, 63, 64, 65, 130} and {x[1] for x in c} == {1, 8, 9, 33, 256} and {x[3] for x in c} == {128, 256}
    assert any(x[1] == x[2] for x in c) and any(x[2] > x[1] for x in c) and any(x[2] % 4 for x in c) and any(x[2] % 4 == 0 for x in c)
    assert any(x[4] > x[3] for x in c) and any(x[5] > x[3] for x in c) and any(x[6] == 2 and x[7] == "pad" for x in c) and any(x[7] == "none1" for x in c)
    b = DR.BOX_CASES
    assert {x[0] for x in b} == {1, 7, 64, 901} and {x[2] for x in b} == {1, 4} and {x[5] for x in b} == {"box", "logit"} and any(x[4] > x[3] for x in b)


@pytest.mark.parametrize("i", range(len(DR.BOX_CASES)), ids=DR.BOX_IDS)
def test_box_update_reference_is_transformers(i):
    from transformers.models.grounding_dino.modeling_grounding_dino import encode_sinusoidal_position_embedding
    case = DR.BOX_CASES[i]
    rows, B, L, d, _, mode = case
    h, w3, b3, prior, vr = DR.make_box_case(case, torch.float16, 400 + i)
    is_box = mode == "box"
    if is_box:
        flat = prior.reshape(-1)
        assert {0.0, 1.0, 0.5}.issubset(set(flat.tolist())) if flat.size >= 5 else True
    else:
        assert np.isposinf(prior).any()
    got = DR.box_update_reference(h, w3, b3, prior, is_box, vr, rows // B, 10, eps_dtype=np.float64)
    H, W3, B3, P, VR = (torch.from_numpy(np.asarray(t)).double() for t in (h, w3, b3, prior, vr))
    tmp = H @ W3.T + B3
    ref = (tmp + (torch.special.logit(P, eps=1e-5) if is_box else P)).sigmoid()              # GroundingDinoDecoder.forward / GroundingDinoModel.forward
    lev = ref.view(B, rows // B, 1, 4) * torch.cat([VR, VR], -1)[:, None]
    pos = encode_sinusoidal_position_embedding(lev[:, :, 0, :], num_pos_feats=d // 2).reshape(rows, 2 * d)
    np.testing.assert_allclose(got["ref"][0], ref.numpy(), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(got["ref_levels"][0], lev.reshape(rows, L, 4).numpy(), rtol=1e-12, atol=1e-15)
    # transformers forms dim_t = 10000^(..) in FLOAT32 and divides the fp64 argument by it: the restatement's exact dim_t differs by fp32's rounding of dim_t
    np.testing.assert_allclose(got["pos_in"][0], pos.numpy(), rtol=0, atol=2 * np.pi * 2.0 ** -22)
    if not is_box:
        assert (got["ref"][0][np.isposinf(prior)] == 1.0).all() and (got["ref"][1][np.isposinf(prior)] == 0.0).all()
    # the float32 clamp constants the kernel uses differ from the fp64 ones by less than the logit's own bound
    g32 = DR.box_update_reference(h, w3, b3, prior, is_box, vr, rows // B, 10)
    assert (np.abs(g32["ref"][0] - got["ref"][0]) <= 1e-7).all()
    for name in ("ref", "ref_levels", "pos_in"):
        assert np.isfinite(g32[name][1]).all() and (g32[name][1] >= 0).all()


def test_expected_names_are_transformers_names():
    from theatergen_amd.grounding_dino_decoder import expected_names
    for which in G.CONFIGS:
        model = G.hf_model(which)
        assert expected_names(model.config) == set(G.taken_shapes(model)), which
    assert "model.query_position_embeddings.weight" not in expected_names(G.config("gathered"))


def test_fixture_generator_reproduces_the_stored_checksums_and_the_score_gap():
    """The issue asks to redraw the SEED until the fp32 gap between the ``num_queries``-th and the next proposal score exceeds 8 x the bf16 emulation's
    largest score error.  The generator deviates: it keeps the seed and redraws single memory ROWS (the first proposal below the cut, from a second stream of
    the seed) until the gap opens — neighbouring scores are ~0.3 apart at that rank and the error is ~0.15, so a gap of ~1.3 does not come from redrawing
    everything (the generator's docstring).  The fixture's input is therefore tailored to the selection; the condition itself is the issue's and is
    checked here on the stored figures and on a rerun."""
    z = np.load(G.PATH)
    assert int(z["seed"]) == G.SEED and os.path.getsize(G.PATH) < 200 * 1024
    for which, c in G.CONFIGS.items():
        np.testing.assert_allclose(G.weight_checksums(G.make_weights(which)), z[f"{which}_weight_checksums"], rtol=0, atol=1e-9)
        Q = c["num_queries"]
        gap, err = z[f"{which}_score_gap"]
        assert gap > G.GAP_FACTOR * err > 0, which
        gaps, e, _ = G.score_gap(G.load_model(which)[0], G.inputs(which), Q)                     # the stored figures are what a rerun gives
        assert min(gaps) == pytest.approx(gap, rel=1e-4) and e == pytest.approx(err, rel=1e-3) and min(gaps) > G.GAP_FACTOR * e
        assert z[f"{which}_topk"].shape == (G.BATCH, Q) and np.array_equal(np.sort(z[f"{which}_topk"], 1), z[f"{which}_topk_sorted"])
        assert z[f"{which}_logits"].shape == (G.BATCH, Q, G.MAX_TEXT_LEN) and z[f"{which}_pred_boxes"].shape == (G.BATCH, Q, 4)
        assert np.isneginf(z[f"{which}_logits"][:, :, G.TEXT_LEN:]).all()
        for name in G.quantities(which):
            for dt, hi in (("bf16", 0.05), ("f16", 0.01)):
                e2 = z[f"emu_{dt}_{which}_{name}"]
                assert e2.shape == (2,) and 0 < e2[0] < hi and 0 < e2[1] < 2 * hi, (which, name, dt, e2)
    for name, lo, hi in (("logits", 0.5, 2.0), ("pred_boxes", 0.01, 0.2)):                             # the error of the encoder's outputs, as the heads pass it on
        g = z[f"main_input_gain_{name}"]
        assert g.shape == (2,) and lo < g[0] < hi and lo < g[1] < hi, (name, g)
    assert z["main_hidden1"].shape == (G.BATCH, 20, G.D_MODEL) and z["main_refs0"].shape == (G.BATCH, 20, 4)


def test_config_refusals_name_the_field():
    from theatergen_amd.grounding_dino_decoder import check_config
    good = dict(d_model=256, decoder_attention_heads=8, decoder_ffn_dim=2048, decoder_layers=6, num_feature_levels=4, decoder_n_points=4,
                activation_function="relu", two_stage=True, query_dim=4, max_text_len=256, num_queries=900, two_stage_bbox_embed_share=False)
    check_config(SimpleNamespace(**good))
    for which in G.CONFIGS:
        check_config(G.config(which))
    for change, word in ((dict(d_model=512), "d_model"), (dict(decoder_attention_heads=4), "decoder_attention_heads"),
                         (dict(decoder_n_points=8), "decoder_n_points"), (dict(num_feature_levels=5), "num_feature_levels"),
                         (dict(activation_function="gelu"), "activation_function"), (dict(two_stage=False), "two_stage"), (dict(query_dim=2), "query_dim"),
                         (dict(max_text_len=512), "max_text_len"), (dict(two_stage_bbox_embed_share=True), "two_stage_bbox_embed_share")):
        with pytest.raises(NotImplementedError, match=word):
            check_config(SimpleNamespace(**dict(good, **change)))


def test_state_dict_mismatch_is_an_error():
    from theatergen_amd.grounding_dino_decoder import GroundingDinoDecoderHead
    w = {k: torch.from_numpy(v) for k, v in G.make_weights().items()}
    w.pop("bbox_embed.1.layers.2.bias")
    with pytest.raises(RuntimeError, match="missing"):
        GroundingDinoDecoderHead(G.config(), w, "cpu", torch.bfloat16)
    w = {k: torch.from_numpy(v) for k, v in G.make_weights().items()}
    w["model.decoder.layers.0.extra.weight"] = torch.zeros(1)
    with pytest.raises(RuntimeError, match="unexpected"):
        GroundingDinoDecoderHead(G.config(), w, "cpu", torch.bfloat16)
    with pytest.raises(RuntimeError, match="dtype"):
        GroundingDinoDecoderHead(G.config(), {k: torch.from_numpy(v) for k, v in G.make_weights().items()}, "cpu", torch.float32)


def _declared(header, name):
    m = re.search(r"^int " + name + r"\s*\(([^;]*)\);", header, flags=re.M | re.S)
    assert m, f"{name} is not declared"
    kinds = {"int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float}
    return [C.c_void_p if "*" in p else kinds[p.split()[0]] for p in (q.strip() for q in m.group(1).replace("\n", " ").split(","))]


def test_abi_entries_header_binding_and_symbols_agree():
    from theatergen_amd import _lib
    header = open(os.path.join(ROOT, "include", "theatergen_hip.h")).read()
    assert re.search(r"#define TG_ABI_VERSION 308\b", header) and _lib.ABI_VERSION == 308
    h = _lib.lib()
    for name in ("tg_dino_contrastive", "tg_dino_box_update"):
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int32 and args == _declared(header, name), name
        assert getattr(h, name) is not None

    # host validation, fake pointers (never read): every refusal the header lists, each naming the entry point
    def ctr(dtype=0, batch=1, n=5, d=128, Lt=9, T=16, q=64, q_ld=128, q_bs=0, text=64, t_ld=128, t_bs=0, mask=64, logits=64, row_max=64):
        return h.tg_dino_contrastive(dtype, batch, n, d, Lt, T, q, q_ld, q_bs, text, t_ld, t_bs, mask, logits, row_max, None)
    for kw, code in ((dict(d=64), -3), (dict(d=192), -3), (dict(Lt=0), -3), (dict(Lt=17), -3), (dict(T=257, Lt=257), -3), (dict(dtype=2), -1),
                     (dict(batch=0), -1), (dict(n=0), -1), (dict(q=0), -1), (dict(text=0), -1), (dict(mask=0), -1), (dict(logits=0, row_max=0), -1),
                     (dict(q_ld=132), -1), (dict(q_ld=120), -1), (dict(t_ld=120), -1), (dict(batch=2, q_bs=4), -1), (dict(batch=2, t_bs=-8), -1),
                     (dict(q=72), -1), (dict(text=8), -1), (dict(logits=66), -1), (dict(row_max=65), -1)):
        assert ctr(**kw) == code, kw
        assert b"tg_dino_contrastive" in h.tg_last_error()

    def box(dtype=0, rows=6, rpb=3, d=128, hp=64, h_ld=128, w3=64, b3=64, prior=64, flag=1, vr=64, L=4, ref=64, lev=64, pos=64, pos_ld=256):
        return h.tg_dino_box_update(dtype, rows, rpb, d, hp, h_ld, w3, b3, prior, flag, vr, L, ref, lev, pos, pos_ld, None)
    for kw, code in ((dict(d=64), -3), (dict(L=0), -3), (dict(L=5), -3), (dict(dtype=2), -1), (dict(rows=0), -1), (dict(rows=2 ** 31), -1),
                     (dict(rpb=0), -1), (dict(rpb=4), -1), (dict(flag=2), -1), (dict(hp=0), -1), (dict(w3=0), -1), (dict(b3=0), -1), (dict(prior=0), -1),
                     (dict(ref=0), -1), (dict(vr=0), -1), (dict(vr=0, lev=0), -1), (dict(h_ld=120), -1), (dict(pos_ld=255), -1), (dict(prior=72), -1),
                     (dict(b3=66), -1), (dict(ref=66), -1), (dict(hp=65), -1), (dict(pos=65), -1)):
        assert box(**kw) == code, kw
        assert b"tg_dino_box_update" in h.tg_last_error()


def test_wrapper_refusals_without_a_device():
    from theatergen_amd import ops
    bf = torch.bfloat16
    q, t, m = torch.zeros(1, 5, 128, dtype=bf), torch.zeros(1, 9, 128, dtype=bf), torch.ones(1, 9, dtype=torch.bool)
    for args, kw, word in (((q.float(), t, m, 16), {}, "dtype"), ((q[0], t, m, 16), {}, "q must be"), ((q, t.half(), m, 16), {}, "does not match"),
                           ((torch.zeros(1, 5, 64, dtype=bf), torch.zeros(1, 9, 64, dtype=bf), m, 16), {}, "d = 64"), ((q, t, m, 8), {}, "max_text_len"),
                           ((q, t, m, 300), {}, "max_text_len"), ((q, t, m[:, :8], 16), {}, "token_mask"), ((q, t, m.float(), 16), {}, "token_mask"),
                           ((torch.zeros(1, 5, 132, dtype=bf)[:, :, :128], t, m, 16), {}, "pitches"),
                           ((q, t, m, 16), dict(logits=False, row_max=False), "neither"), ((q, t, m, 16), dict(logits=torch.zeros(1, 5, 15)), "logits must be"),
                           ((q, t, m, 16), dict(row_max=torch.zeros(1, 5, dtype=torch.float64)), "row_max must be"), ((q, t, m, 16), {}, "GPU")):
        with pytest.raises(RuntimeError, match=word):
            ops.dino_contrastive(*args, **kw)
    h, w3, b3, pr, vr = torch.zeros(6, 128, dtype=bf), torch.zeros(4, 128, dtype=bf), torch.zeros(4), torch.zeros(6, 4), torch.ones(2, 4, 2)
    for args, kw, word in (((h.float(), w3, b3, pr, True), {}, "dtype"), ((h[0], w3, b3, pr, True), {}, "h must be"),
                           ((torch.zeros(6, 64, dtype=bf), w3, b3, pr, True), {}, "d = 64"), ((h, w3.half(), b3, pr, True), {}, "w3 must be"),
                           ((h, w3[:3], b3, pr, True), {}, "w3 must be"), ((h, w3, b3.double(), pr, True), {}, "b3 must be"),
                           ((h, w3, b3, pr[:5], True), {}, "prior must be"), ((h, w3, b3, pr, True), dict(rows_per_batch=4), "multiple"),
                           ((h, w3, b3, pr, True), dict(ref_levels=True), "need valid_ratios"),
                           ((h, w3, b3, pr, True), dict(rows_per_batch=3, valid_ratios=torch.ones(2, 5, 2), pos_in=True), "1 <= L <= 4"),
                           ((h, w3, b3, pr, True), dict(rows_per_batch=3, valid_ratios=torch.ones(3, 4, 2), pos_in=True), "valid_ratios must be"),
                           ((h, w3, b3, pr, True), dict(rows_per_batch=3, valid_ratios=vr, pos_in=torch.zeros(6, 256)), "pos_in must be"),
                           ((h, w3, b3, pr, True), dict(rows_per_batch=3, valid_ratios=vr, ref_levels=torch.zeros(6, 3, 4)), "ref_levels must be"),
                           ((h, w3, b3, pr, True), dict(ref=torch.zeros(6, 3)), "ref must be"),
                           ((h, w3, b3, pr, True), dict(rows_per_batch=3, valid_ratios=vr, ref_levels=True, pos_in=True), "GPU")):
        with pytest.raises(RuntimeError, match=word):
            ops.dino_box_update(*args, **kw)


# ---- detect / detect_many / the caption cache, on stubs -----------------------------------------------------------------------------------------
class _StubProcessor:
    """a caption -> ids by word hash, padded to the longest; images -> a [B, 3, 8, 8] tensor of each image's mean"""
    calls = 0

    def __call__(self, images, text, return_tensors="pt", padding=False):
        type(self).calls += 1
        images = images if isinstance(images, list) else [images]
        text = text if isinstance(text, list) else [text]
        ids = [[101] + [1000 + sum(map(ord, w)) % 500 for w in t.replace(".", " . ").split()] + [102] for t in text]
        n = max(map(len, ids))
        return {"input_ids": torch.tensor([i + [0] * (n - len(i)) for i in ids]), "attention_mask": torch.tensor([[1] * len(i) + [0] * (n - len(i)) for i in ids]),
                "pixel_values": torch.stack([torch.full((3, 8, 8), float(np.asarray(im).mean())) for im in images])}


class _StubModel:
    """per item: logits and boxes that depend on the item's ids (without the padding) and pixels only"""
    calls = 0

    def __call__(self, pixel_values, input_ids, attention_mask=None, **kw):
        type(self).calls += 1
        B = input_ids.shape[0]
        logits, boxes = torch.full((B, 6, 16), -5.0), torch.zeros(B, 6, 4)
        for b in range(B):
            key = int((input_ids[b] * attention_mask[b]).sum()) + int(pixel_values[b, 0, 0, 0] * 10)
            g = torch.Generator().manual_seed(key)
            if float(pixel_values[b, 0, 0, 0]) > 0:                 # a black image: nothing over the threshold
                logits[b] = torch.randn(6, 16, generator=g) * 2
            boxes[b] = torch.rand(6, 4, generator=g) * 0.5 + 0.25
        return SimpleNamespace(logits=logits, pred_boxes=boxes)


def test_detect_many_is_detect_one_by_one():
    from theatergen_amd.detector import detect, detect_many
    gd = {"model": _StubModel(), "processor": _StubProcessor()}
    words = ["cat", "a red wizard", "dog", ["owl", "hat"], "x"]
    images = [np.full((40 + 3 * i, 60 - 2 * i, 3), 10 * i, np.uint8) for i in range(len(words))]
    one = [detect(gd, w, im) for w, im in zip(words, images)]
    p0, m0 = _StubProcessor.calls, _StubModel.calls
    many = detect_many(gd, words, images)
    assert _StubProcessor.calls == p0 + 1 and _StubModel.calls == m0 + 1                     # one processor call, one forward
    assert len(many) == len(one) and {ok for _, ok in one} == {True, False}
    for (b1, ok1), (b2, ok2) in zip(one, many):
        assert ok1 == ok2 and np.array_equal(b1, b2) and b2.dtype == np.float32
    assert detect_many(gd, [], []) == []
    with pytest.raises(ValueError, match="words"):
        detect_many(gd, ["a"], [])


def test_caption_cache_hits_only_for_cpu_ids():
    from theatergen_amd.detector import GroundingDinoDetector
    det = GroundingDinoDetector.__new__(GroundingDinoDetector)
    from collections import OrderedDict
    det._captions, det.cache_size, det.cache_hits, det.cache_misses = OrderedDict(), 2, 0, 0
    runs = []
    det._encode_text = lambda ids, am, tt: runs.append(tuple(ids.shape)) or ("states", len(runs))
    ids, am = torch.tensor([[101, 7, 102, 0]]), torch.tensor([[1, 1, 1, 0]])
    a = det.text_states(ids, am)
    assert det.text_states(ids.clone(), am.clone()) is a and len(runs) == 1 and (det.cache_hits, det.cache_misses) == (1, 1)
    assert det.text_states(ids, torch.tensor([[1, 1, 1, 1]])) is not a and len(runs) == 2     # the mask is part of the key
    assert det.text_states(ids.view(2, 2), am.view(2, 2)) is not a and len(runs) == 3         # and so is the shape; this evicts the oldest of 2 entries
    det.text_states(ids, am)
    assert len(runs) == 4 and len(det._captions) == 2
    n = len(runs)
    meta = ids.to("meta")                                                                     # stands for device ids: never read, never cached
    det.text_states(meta, am.to("meta"))
    det.text_states(meta, am.to("meta"))
    assert len(runs) == n + 2 and det.cache_hits == 1
    det.cache_size = 0
    det.text_states(ids, am)
    det.text_states(ids, am)
    assert len(runs) == n + 4
