"""CPU: the fp64 restatement of ``tg_attention_swin`` is pinned against transformers' own SwinLayer path, the kernel cases exercise every clause of
the contract, ``detect`` on a stub, the ABI entry, the fixture's generator."""
import os
import re

import numpy as np
import pytest
import torch

from tests import swin_window_reference as R
from tests.golden import make_grounding_dino_vision_golden as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OP_TOL_WORST = 1.5e-2            # op_tol of tests/test_sam_gpu.py for bf16, the wider of the two
IDS = [f"{H}x{W}_s{s}_b{b}_h{h}" for H, W, s, b, h in R.CASES]


def _rel_l2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_restatement_equals_transformers_swin_layer(case):
    """``swin_window_reference`` on fp32 inputs against SwinLayer's own maybe_pad / cyclic_shift / window_partition / get_attn_mask / SwinAttention /
    window_reverse with the same weights (o_proj = identity).  max abs <= 1e-5 of the output's max: fp32 against fp64 on O(1) values, 49-term sums."""
    swin = pytest.importorskip("transformers.models.swin.modeling_swin")
    from transformers import SwinConfig
    H, W, shift, B, heads = case
    C = heads * 32
    torch.manual_seed(H * 100 + W)
    cfg = SwinConfig(embed_dim=C, depths=[1], num_heads=[heads], window_size=7, attn_implementation="eager")
    layer = swin.SwinLayer(cfg, C, (H, W), heads, 0.0, shift_size=shift).eval().float()
    att = layer.attention
    with torch.no_grad():
        for lin in (att.q_proj, att.k_proj, att.v_proj):
            lin.weight.copy_(torch.randn(C, C) * C ** -0.5 * 1.5)
            lin.bias.copy_(torch.randn(C))
        att.o_proj.weight.copy_(torch.eye(C))
        att.o_proj.bias.zero_()
        att.relative_position_bias.relative_position_bias_table.copy_(torch.randn(169, heads))
        x = torch.randn(B, H, W, C)
        # SwinLayer.forward between layernorm_before and the residual add (always_partition: the backbone's path)
        hp, pad = layer.maybe_pad(x, H, W)
        Hp, Wp = hp.shape[1], hp.shape[2]
        win = swin.window_partition(layer.cyclic_shift(hp), 7).view(-1, 49, C)
        mask = layer.get_attn_mask(Hp, Wp, dtype=hp.dtype, device=hp.device)
        o, _ = att(win, mask)
        o = layer.cyclic_shift(swin.window_reverse(o.view(-1, 7, 7, C), 7, Hp, Wp), reverse=True)[:, :H, :W].reshape(B, H * W, C)
        xd = x.double().reshape(B, H * W, C)
        q, k, v = (xd @ lin.weight.double().T + lin.bias.double() for lin in (att.q_proj, att.k_proj, att.v_proj))
    pads = [lin.bias.detach().double().numpy() for lin in (att.q_proj, att.k_proj, att.v_proj)]
    table = att.relative_position_bias.relative_position_bias_table.detach().double().numpy()
    ref = R.swin_window_reference(q.numpy(), k.numpy(), v.numpy(), pads[0], pads[1], pads[2], table, H, W, shift, 32 ** -0.5)
    err = np.abs(o.double().numpy() - ref).max() / np.abs(ref).max()
    print(f"restatement vs SwinLayer {case}: max abs / max {err:.2e}")
    assert err <= 1e-5


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_every_clause_of_the_contract_moves_the_result(case):
    """A condition on the inputs of the GPU cases: dropping the bias, the shift mask, the padded keys or the roll moves the fp64 reference by more than
    10 * op_tol / 2 rel-L2 wherever the case has that feature — a kernel that forgot one cannot pass at op_tol."""
    H, W, shift, B, heads = case
    qkv, pads, table = R.make_case(H, W, shift, B, heads, seed=H * 100 + W)
    ref = R.run_case(qkv, pads, table, H, W, shift)
    has = {"bias": True, "mask": shift > 0, "roll": shift > 0, "padkeys": H % 7 != 0 or W % 7 != 0}
    for what, present in has.items():
        if not present:
            continue
        moved = _rel_l2(R.run_case(qkv, pads, table, H, W, shift, drop=(what,)), ref)
        print(f"{case}: without {what} the reference moves by {moved:.3f}")
        assert moved > 10 * OP_TOL_WORST / 2, (what, moved)


def test_region_formula_is_transformers_mask():
    swin = pytest.importorskip("transformers.models.swin.modeling_swin")
    from transformers import SwinConfig
    layer = swin.SwinLayer(SwinConfig(embed_dim=32, depths=[1], num_heads=[1], window_size=7), 32, (14, 21), 1, 0.0, shift_size=3)
    m = layer.get_attn_mask(14, 21, torch.float32, torch.device("cpu")).numpy()
    reg = np.array([[R.region(r, c, 14, 21, 3) for c in range(21)] for r in range(14)])
    regw = reg.reshape(2, 7, 3, 7).transpose(0, 2, 1, 3).reshape(-1, 49)
    want = np.where(regw[:, None, :] != regw[:, :, None], -100.0, 0.0)
    assert np.array_equal(m, want)


class _StubModel:
    def __init__(self, logits, boxes):
        self.logits, self.boxes, self.calls = logits, boxes, []

    def __call__(self, **kw):
        from types import SimpleNamespace
        self.calls.append(kw)
        return SimpleNamespace(logits=self.logits[None], pred_boxes=self.boxes[None])


def _logit(p):
    return float(np.log(p / (1 - p)))


def test_detect_on_a_stub():
    from theatergen_amd.detector import caption_of, detect, select_box
    seen = {}

    def processor(images=None, text=None, return_tensors=None):
        seen["text"] = text
        return {"pixel_values": torch.zeros(1, 3, 8, 8), "input_ids": torch.zeros(1, 4, dtype=torch.long)}
    image = np.zeros((300, 400, 3), np.uint8)
    boxes = torch.tensor([[0.5, 0.5, 0.2, 0.4], [0.25, 0.5, 0.5, 0.5], [0.9, 0.9, 0.1, 0.1]])
    logits = torch.full((3, 5), -10.0)
    logits[0, 1], logits[1, 3], logits[2, 0] = _logit(0.6), _logit(0.8), _logit(0.2)
    model = _StubModel(logits, boxes)
    xyxy, ok = detect({"model": model, "processor": processor}, "A Red Fox", image)
    assert ok and seen["text"] == "a red fox" and caption_of(["Cat", "DOG"]) == "cat. dog"
    np.testing.assert_allclose(xyxy, [0.0, 75.0, 200.0, 225.0], atol=1e-3)            # query 1: cx .25 cy .5 w .5 h .5 on 400 x 300
    assert set(model.calls[0]) == {"pixel_values", "input_ids"}
    # the threshold edge: a confidence that does not EXCEED 0.3 is no box
    edge = torch.full((2, 3), -10.0)
    edge[0, 0] = _logit(0.2999)
    assert not select_box(edge, boxes[:2], 300, 400)[1]
    edge[1, 2] = _logit(0.3001)
    xy, ok = select_box(edge, boxes[:2], 300, 400)
    assert ok and np.allclose(xy, [0.0, 75.0, 200.0, 225.0], atol=1e-3)
    xy, ok = detect({"model": _StubModel(torch.full((3, 5), -10.0), boxes), "processor": processor}, "fox", image)
    assert not ok and xy.shape == (4,)


def test_abi_entry_header_binding_and_symbol_agree():
    import ctypes as C
    from theatergen_amd import _lib
    header = open(os.path.join(ROOT, "include", "theatergen_hip.h")).read()
    m = re.search(r"^int tg_attention_swin\s*\(([^;]*)\);", header, flags=re.M | re.S)
    assert m, "tg_attention_swin is not declared"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    res, args = _lib.SIGNATURES["tg_attention_swin"]
    kinds = {"int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float}
    want = [C.c_void_p if "*" in p else kinds[p.split()[0]] for p in params]
    assert res is C.c_int32 and args == want
    assert re.search(r"#define TG_ABI_VERSION 308\b", header) and _lib.ABI_VERSION == 308
    h = _lib.lib()
    assert h.tg_attention_swin is not None
    # host validation, fake pointers (never read): each refusal names the entry point

    def call(dtype=0, batch=1, heads=1, hd=32, win=7, H=7, W=7, shift=0, scale=1.0, q=64, ld=96, out=64):
        return h.tg_attention_swin(dtype, batch, heads, hd, win, H, W, shift, scale, q, ld, 0, 64, ld, 0, 64, ld, 0, 64, 64, 64, 64, out, 32, 0, None)
    for kw, code in ((dict(hd=64), -3), (dict(win=12), -3), (dict(H=6), -1), (dict(W=6), -1), (dict(shift=2), -1), (dict(q=72), -1), (dict(ld=100), -1),
                     (dict(scale=0.0), -1), (dict(dtype=2), -1), (dict(out=0), -1)):
        assert call(**kw) == code, kw
        assert b"tg_attention_swin" in h.tg_last_error()


def test_fixture_generator_reproduces_the_stored_checksums():
    z = np.load(G.PATH)
    w = G.make_weights()
    assert set(w) == set(G.param_shapes())
    np.testing.assert_allclose(G.weight_checksums(w), z["weight_checksums"], rtol=0, atol=1e-9)
    from theatergen_amd.grounding_dino import expected_names
    from types import SimpleNamespace
    cfg = SimpleNamespace(backbone_config=dict(embed_dim=G.EMBED, depths=list(G.DEPTHS), num_heads=list(G.HEADS), window_size=7,
                                               out_indices=list(G.OUT_INDICES)), num_feature_levels=4, d_model=G.D_MODEL)
    assert expected_names(cfg) == set(w)
    assert z["hidden0"].shape == (len(G.ROWS), 50, 32) and z["feature2"].shape == (256, 8, 7) and z["proj3"].shape == (64, 4, 4)
