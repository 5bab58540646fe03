"""Regenerate tests/golden/grounding_dino_decoder.npz from ``transformers``' GroundingDINO (fp32, CPU): the two-stage query selection of
``GroundingDinoModel.forward``, ``GroundingDinoDecoder`` and the last level of ``GroundingDinoForObjectDetection``'s heads — the part
``theatergen_amd.grounding_dino_decoder.GroundingDinoDecoderHead`` runs.  ``hf_run`` restates the lines of ``GroundingDinoModel.forward`` between the
encoder and the decoder with the model's OWN modules (``generate_encoder_output_proposals``, ``encoder_output_class_embed``,
``encoder_output_bbox_embed``, ``decoder``, ``class_embed``, ``bbox_embed``), because the run starts from encoder outputs, not from an image.

Config ``"main"``: ``d_model 128, decoder_attention_heads 4, decoder_ffn_dim 256, decoder_layers 2, num_queries 20`` (not a multiple of 8),
``max_text_len 16``, ``decoder_bbox_embed_share False`` (every layer its own box head), the encoder fixture's four levels (992 tokens) with item 1's padded
mask, its 9 text tokens with padding, batch 2.  Config ``"gathered"``: ``embedding_init_target False`` (the target is the gathered object queries),
``decoder_layers 1, num_queries 12``, final outputs only.  (``GroundingDinoModel.forward`` itself cannot run that config in ``transformers`` 5.x: it reads
``query_position_embeddings``, which the constructor did not make.  The restated lines take the branch the config names.)

The weights are NOT stored: ``make_weights`` draws them from numpy's legacy ``RandomState`` in sorted-name order — parameter = base + s * randn, rounded
to fp16-representable values, base 1 for LayerNorm weights, s 0.3 for ``sampling_offsets.weight`` / ``attention_weights.weight``, s 1 for
``sampling_offsets.bias``, s 0.5 for ``query_position_embeddings.weight``, s 0.05 for everything else — the last layers of the box heads included, which
``transformers`` initialises to zero (with that no box would move).  The file keeps (sum, sum of squares) per parameter.  The encoder outputs are drawn
the same way: memory and text states ~ N(0, 1).

Stored, float32, with the queries of every item SORTED BY PROPOSAL INDEX (``topk_sorted``; ``topk`` keeps the score order): the initial reference boxes,
per layer the normed hidden states and the reference boxes after the layer, the final ``logits`` and ``pred_boxes``; for ``"gathered"`` the final outputs.
Per quantity and storage dtype the error (rel-L2, max-rel; logits over their finite entries) of a ROUNDED EMULATION of the same forward: weights, inputs
and every Linear / LayerNorm output rounded to the storage dtype, except the 4-wide outputs of the box heads: coordinates stay fp32.  The GPU test's bound
for a quantity is twice that error.  ``main_input_gain_{logits,pred_boxes}``: the error of the two outputs per unit of relative rms error of the encoder's
outputs (``input_gain``), for the tests in which a bf16 / fp16 front and encoder stand before the head.

THE SCORE GAP.  With ``embedding_init_target`` the content query of a selected proposal is ``query_position_embeddings[rank]``: only the SET of selected
proposals can be made stable under rounding, their order cannot (20 scores of ~35 with a bf16 error of ~0.15), so the GPU test pins the order where it
compares decoder states.  For the set, the fp32 gap between the ``num_queries``-th and the next proposal score must exceed 8 x the largest score error of
the bf16 emulation, for every item.  Scores of 992 N(0, 1)-like tokens are ~0.3 apart at rank 20 and the error is ~0.15: no redrawn seed gets there
(400 were tried), so ``inputs`` redraws ROWS instead: while an item's gap is too small, the memory row of its (``num_queries`` + 1)-th proposal is drawn
again from a second stream of the seed, until the condition holds (``make`` asserts it, the CPU test checks it on the stored figures and on a rerun).

    python tests/golden/make_grounding_dino_decoder_golden.py
"""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
try:
    from tests.golden import make_grounding_dino_encoder_golden as E
except ImportError:                                       # run as a script: the repository root is not on the path yet
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from tests.golden import make_grounding_dino_encoder_golden as E

PATH = os.path.join(HERE, "grounding_dino_decoder.npz")
SEED = 3000
D_MODEL, HEADS, MAX_TEXT_LEN = 128, 4, 16
CONFIGS = {"main": dict(decoder_layers=2, num_queries=20, embedding_init_target=True),
           "gathered": dict(decoder_layers=1, num_queries=12, embedding_init_target=False)}
SHAPES, BATCH, TEXT_LEN, INPUT_IDS = E.SHAPES, E.BATCH, E.TEXT_LEN, E.INPUT_IDS
NV = sum(h * w for h, w in SHAPES)
GAP_FACTOR = 8.0
TAKEN = ("model.decoder.", "model.enc_output.", "model.enc_output_norm.", "model.encoder_output_bbox_embed.", "model.query_position_embeddings.",
         "bbox_embed.")


def config(which="main"):
    from transformers import GroundingDinoConfig
    return GroundingDinoConfig(
        backbone_config=dict(model_type="swin", embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8], window_size=7, out_indices=[2, 3, 4]),
        d_model=D_MODEL, num_feature_levels=len(SHAPES), encoder_layers=1, encoder_attention_heads=HEADS, decoder_attention_heads=HEADS,
        encoder_ffn_dim=1024, decoder_ffn_dim=256, encoder_n_points=4, decoder_n_points=4, max_text_len=MAX_TEXT_LEN, disable_custom_kernels=True,
        decoder_bbox_embed_share=False,
        text_config=dict(model_type="bert", hidden_size=32, num_hidden_layers=1, num_attention_heads=2, intermediate_size=64, vocab_size=2000,
                         max_position_embeddings=64), **CONFIGS[which])


def hf_model(which="main"):
    import torch
    from transformers import GroundingDinoForObjectDetection
    torch.manual_seed(0)
    return GroundingDinoForObjectDetection(config(which)).eval().float()


def taken_shapes(model):
    return {k: tuple(v.shape) for k, v in model.state_dict().items() if k.startswith(TAKEN) and not k.startswith("model.decoder.bbox_embed.")}


def make_weights(which="main", seed=SEED, shapes=None):
    """{name in GroundingDinoForObjectDetection's state dict: float32 array of fp16-representable values}, drawn in sorted-name order"""
    if shapes is None:
        shapes = taken_shapes(hf_model(which))
    rs = np.random.RandomState(seed + (0 if which == "main" else 7))
    out = {}
    for name, shape in sorted(shapes.items()):
        base, s = 0.0, 0.05
        if "norm" in name and name.endswith(".weight"):
            base = 1.0
        elif name.endswith("sampling_offsets.weight") or name.endswith("attention_weights.weight"):
            s = 0.3
        elif name.endswith("sampling_offsets.bias"):
            s = 1.0
        elif name.endswith("query_position_embeddings.weight"):
            s = 0.5
        out[name] = (base + s * rs.standard_normal(shape)).astype(np.float16).astype(np.float32)
    return out


def weight_checksums(w):
    return np.array([[v.astype(np.float64).sum(), (v.astype(np.float64) ** 2).sum()] for _, v in sorted(w.items())])


@functools.lru_cache(maxsize=None)
def inputs(which="main", seed=SEED):
    """the encoder's outputs and the masks, as torch tensors (fp32 / bool, CPU): memory [B, Nv, d], text [B, Lt, d], valid [B, Nv] (True = a real token,
    ``mask_flatten``), token_mask [B, Lt] (True = a real token), valid_ratios [B, L, 2]"""
    import torch
    rs = np.random.RandomState(seed + 1)
    f16 = lambda a: torch.from_numpy(a.astype(np.float16).astype(np.float32))                       # noqa: E731
    memory = f16(rs.standard_normal((BATCH, NV, D_MODEL)))
    text = f16(rs.standard_normal((BATCH, TEXT_LEN, D_MODEL)))
    masks = E.level_masks()
    ratios = []
    for m in masks:                                                                                 # GroundingDinoModel.get_valid_ratio
        _, H, W = m.shape
        ratios.append(torch.stack([m[:, 0, :].sum(1).float() / W, m[:, :, 0].sum(1).float() / H], -1))
    kw = dict(memory=memory, text=text, valid=torch.cat([m.flatten(1) for m in masks], 1), token_mask=torch.tensor(INPUT_IDS) != 0,
              valid_ratios=torch.stack(ratios, 1).float())
    # the score gap (module docstring): redraw the row of the first proposal below the cut until every item's gap is wide enough
    model, Q, rs2 = load_model(which, seed)[0], CONFIGS[which]["num_queries"], np.random.RandomState(seed + 2)
    for _ in range(400):
        gaps, e, nxt = score_gap(model, kw, Q)
        small = [b for b in range(BATCH) if not gaps[b] > GAP_FACTOR * e]
        if not small:
            return kw
        for b in small:
            memory[b, nxt[b]] = f16(rs2.standard_normal(D_MODEL))
    raise RuntimeError("the score gap did not open")


def load_model(which="main", seed=SEED):
    import torch
    model = hf_model(which)
    w = make_weights(which, seed, taken_shapes(model))
    sd = {k: torch.from_numpy(v) for k, v in w.items()}
    sd.update({"model.decoder." + k: v for k, v in sd.items() if k.startswith("bbox_embed.")})     # the decoder's spelling of the same heads
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and not [k for k in missing if k.startswith(TAKEN)], (missing, unexpected)
    return model, w


def hf_run(model, kw, round_dtype=None, select_only=False, pin=None, check_set=True):
    """the restated forward -> dict of tensors in SCORE order.  ``round_dtype``: the rounded emulation (the arithmetic stays fp32).  ``pin``: a [B, Q] index
    tensor that replaces the run's own order of the selected proposals AFTER its set was found equal (the rank decides the content query)."""
    import copy

    import torch
    rnd = (lambda x: x.to(round_dtype).float()) if round_dtype is not None else (lambda x: x)
    hooks = []
    memory, text = kw["memory"], kw["text"]
    if round_dtype is not None:
        model = copy.deepcopy(model)
        model.model.decoder.bbox_embed = model.bbox_embed
        with torch.no_grad():
            for p in model.parameters():
                p.copy_(rnd(p))
        for m in model.modules():
            if isinstance(m, torch.nn.LayerNorm) or (isinstance(m, torch.nn.Linear) and m.out_features != 4):
                hooks.append(m.register_forward_hook(lambda _m, _i, o: rnd(o)))
        memory, text = rnd(memory), rnd(text)
    core, cfg = model.model, model.config
    valid, token_mask, vr = kw["valid"], kw["token_mask"], kw["valid_ratios"]
    Q = cfg.num_queries
    with torch.no_grad():
        oq, props = core.generate_encoder_output_proposals(memory, ~valid, list(SHAPES))
        scores = core.encoder_output_class_embed(oq, text, token_mask).max(-1)[0]
        out = dict(scores=scores)
        if not select_only:
            coord_logits = core.encoder_output_bbox_embed(oq) + props
            topk = torch.topk(scores, Q, dim=1)[1]
            if pin is not None:
                assert not check_set or torch.equal(torch.sort(topk, 1)[0], torch.sort(pin, 1)[0]), "the run selects another set"
                topk = pin
            ref0 = torch.gather(coord_logits, 1, topk.unsqueeze(-1).repeat(1, 1, 4)).sigmoid()
            if cfg.embedding_init_target:
                target = core.query_position_embeddings.weight.unsqueeze(0).repeat(BATCH, 1, 1)
            else:
                target = torch.gather(oq, 1, topk.unsqueeze(-1).repeat(1, 1, D_MODEL))
            spatial = torch.tensor(SHAPES, dtype=torch.long)
            dec = core.decoder(inputs_embeds=target, vision_encoder_hidden_states=memory, vision_encoder_attention_mask=valid,
                               text_encoder_hidden_states=text, text_encoder_attention_mask=~token_mask, reference_points=ref0,
                               spatial_shapes=spatial, spatial_shapes_list=list(SHAPES),
                               level_start_index=torch.cat((spatial.new_zeros((1,)), spatial.prod(1).cumsum(0)[:-1])), valid_ratios=vr,
                               return_dict=True)
            hs, refs = dec.intermediate_hidden_states, dec.intermediate_reference_points
            before = ref0 if cfg.decoder_layers == 1 else refs[:, -2]
            logits = model.class_embed[-1](hs[:, -1], text, token_mask)
            boxes = (model.bbox_embed[-1](hs[:, -1]) + torch.special.logit(before, eps=1e-5)).sigmoid()
            out.update(topk=topk, ref0=ref0, hidden=hs, refs=refs, logits=logits, pred_boxes=boxes)
    for h in hooks:
        h.remove()
    return out


def score_gap(model, kw, Q):
    """(per item the fp32 gap between the Q-th and the next proposal score, the largest bf16-emulation score error, per item the index of that next
    proposal)"""
    import torch
    ref = hf_run(model, kw, select_only=True)["scores"]
    emu = hf_run(model, kw, torch.bfloat16, select_only=True)["scores"]
    top, idx = torch.topk(ref, Q + 1, dim=1)
    return (top[:, Q - 1] - top[:, Q]).tolist(), float((emu - ref).abs().max()), idx[:, Q].tolist()


INPUT_NOISE, INPUT_DRAWS = 1e-2, 3


def input_gain(model, kw, run):
    """How an error of the ENCODER'S OUTPUTS reaches the heads: {"logits" | "pred_boxes": [rel-L2 of the output per unit of rel-L2 of the input error,
    max-rel of the output per unit of max-rel of the input error]}, both metrics as ``err`` defines them, the input error pooled over the memory and the
    text states.  The fp32 forward is rerun with both perturbed by Gaussian noise of relative rms ``INPUT_NOISE`` (the size of the encoder fixture's bf16
    error), the selection held at the unperturbed run's (what moves is what the decoder and the heads pass on, not the top-k); the largest ratio over
    ``INPUT_DRAWS`` draws is kept.  The whole-model tests multiply it by the bound, in the same metric, of what enters the head."""
    import torch
    ref = sort_by_proposal(run)
    gen = torch.Generator().manual_seed(SEED + 3)
    gain = {"logits": [0.0, 0.0], "pred_boxes": [0.0, 0.0]}
    for _ in range(INPUT_DRAWS):
        noisy = dict(kw)
        for k in ("memory", "text"):
            noisy[k] = kw[k] + INPUT_NOISE * kw[k].pow(2).mean().sqrt() * torch.randn(kw[k].shape, generator=gen)
        pool = lambda d: np.concatenate([d[k].numpy().ravel() for k in ("memory", "text")])            # noqa: E731
        e_in = err(pool(noisy), pool(kw))
        got = sort_by_proposal(hf_run(model, noisy, pin=run["topk"], check_set=False))
        for name in gain:
            e = err(got[name].numpy(), ref[name].numpy())
            gain[name] = [max(g, v / i) for g, v, i in zip(gain[name], e, e_in)]
    return gain


def sort_by_proposal(run):
    """the per-query tensors of ``hf_run`` with every item's queries sorted by proposal index"""
    import torch
    topk = run["topk"]
    order = torch.argsort(topk, dim=1)
    take = lambda t, dim: torch.stack([t[b].index_select(dim - 1, order[b]) for b in range(BATCH)])      # noqa: E731
    return dict(topk_sorted=take(topk, 1), ref0=take(run["ref0"], 1), hidden=take(run["hidden"], 2), refs=take(run["refs"], 2),
                logits=take(run["logits"], 1), pred_boxes=take(run["pred_boxes"], 1))


def err(a, b):
    """[rel-L2, max-rel] over the entries finite in ``b``; the -inf pattern must agree"""
    fin = np.isfinite(np.asarray(b))
    assert np.array_equal(fin, np.isfinite(np.asarray(a)))
    a, b = np.asarray(a, np.float64)[fin], np.asarray(b, np.float64)[fin]
    return [float(np.linalg.norm(a - b) / np.linalg.norm(b)), float(np.abs(a - b).max() / np.abs(b).max())]


def quantities(which):
    """{name: accessor on a ``sort_by_proposal`` dict}"""
    q = {"logits": lambda r: r["logits"], "pred_boxes": lambda r: r["pred_boxes"]}
    if which == "main":
        q["ref0"] = lambda r: r["ref0"]
        for i in range(CONFIGS["main"]["decoder_layers"]):
            q[f"hidden{i}"] = lambda r, i=i: r["hidden"][:, i]
            q[f"refs{i}"] = lambda r, i=i: r["refs"][:, i]
    return q


def make(path=PATH):
    import torch
    out = dict(seed=np.array(SEED))
    for which in CONFIGS:
        kw = inputs(which)
        model, w = load_model(which)
        out[f"{which}_weight_checksums"] = weight_checksums(w)
        gaps, e, _ = score_gap(model, kw, CONFIGS[which]["num_queries"])
        gap = min(gaps)
        assert gap > GAP_FACTOR * e
        out[f"{which}_score_gap"] = np.array([gap, e])
        run = hf_run(model, kw)
        ref = sort_by_proposal(run)
        out[f"{which}_topk"] = run["topk"].numpy()
        out[f"{which}_topk_sorted"] = ref["topk_sorted"].numpy()
        for name, get in quantities(which).items():
            out[f"{which}_{name}"] = get(ref).numpy()
        if which == "main":
            for name, g in input_gain(model, kw, run).items():
                out[f"main_input_gain_{name}"] = np.array(g)
                print("main input gain", name, g)
        for dname, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
            emu_run = hf_run(model, kw, dt, pin=run["topk"] if CONFIGS[which]["embedding_init_target"] else None)
            assert np.array_equal(np.sort(emu_run["topk"].numpy(), 1), np.sort(run["topk"].numpy(), 1)), "the emulation selects another set"
            emu = sort_by_proposal(emu_run)
            for name, get in quantities(which).items():
                out[f"emu_{dname}_{which}_{name}"] = np.array(err(get(emu).numpy(), get(ref).numpy()))
                print(which, dname, name, out[f"emu_{dname}_{which}_{name}"])
        print(which, "score gap", gap, "bf16 score error", e)
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    import torch
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    make()
