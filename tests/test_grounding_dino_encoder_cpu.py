"""CPU: the fp64 restatements of ``tg_msdeform_attn`` and of masked wide-head attention are pinned to the ``transformers`` modules; the kernel cases
exercise what they claim; names, symbols, bindings and the refusals that need no device."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

from tests import bi_attention_reference as BR
from tests import msdeform_reference as MR
from tests.golden import make_grounding_dino_encoder_golden as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@functools.lru_cache(maxsize=None)
def _case(i):
    return MR.make_case(MR.CASES[i], seed=100 + i)


@functools.lru_cache(maxsize=None)
def _ref(i, drop=()):
    value, offsets, logits, ref, mask = _case(i)
    stats = {}
    return MR.msdeform_reference(value, MR.CASES[i][0], offsets, logits, ref, mask, drop=drop, stats=stats), stats


def _transformers_msdeform(value, shapes, offsets, logits, ref, mask):
    """MultiScaleDeformableAttention + the location arithmetic of GroundingDinoMultiscaleDeformableAttention.forward, fp32"""
    from transformers.models.grounding_dino.modeling_grounding_dino import MultiScaleDeformableAttention
    value, offsets, logits, ref = (torch.from_numpy(np.asarray(t)).float() for t in (value, offsets, logits, ref))
    B, Nv, Cc = value.shape
    heads = Cc // 32
    _, Nq, _, L, P, _ = offsets.shape
    if mask is not None:
        value = value.masked_fill(torch.from_numpy(mask).bool()[..., None], 0.0)
    value = value.view(B, Nv, heads, 32)
    w = torch.softmax(logits, -1).view(B, Nq, heads, L, P)
    spatial = torch.tensor(shapes, dtype=torch.long)
    if ref.shape[-1] == 2:
        norm = torch.stack([spatial[..., 1], spatial[..., 0]], -1)
        loc = ref[:, :, None, :, None, :] + offsets / norm[None, None, None, :, None, :]
    else:
        loc = ref[:, :, None, :, None, :2] + offsets / P * ref[:, :, None, :, None, 2:] * 0.5
    return MultiScaleDeformableAttention()(value, spatial, list(shapes), None, loc, w, 64).numpy()


@pytest.mark.parametrize("i", range(len(MR.CASES)), ids=MR.IDS)
def test_msdeform_reference_is_transformers(i):
    """R = 2 (cases 0, 1, 3) and R = 4 (case 2), with and without the value mask: <= 1e-6 rel-L2 against the fp32 modules"""
    value, offsets, logits, ref, mask = _case(i)
    want = _transformers_msdeform(value, MR.CASES[i][0], offsets, logits, ref, mask)
    e = _rel(_ref(i)[0], want)
    print(f"msdeform reference vs transformers, {MR.IDS[i]}: rel-L2 {e:.2e}")
    assert e <= 1e-6


@pytest.mark.parametrize("i", range(len(MR.CASES)), ids=MR.IDS)
def test_msdeform_cases_exercise_every_clause(i):
    shapes, heads, B, Nq, R, has_mask = MR.CASES[i]
    base, stats = _ref(i)
    print(f"{MR.IDS[i]}: {stats['outside']:.1%} of taps outside their map, {stats['masked']:.1%} of the rest on a masked token")
    assert stats["outside"] >= 0.05
    drops = ["padding", "softmax", "shift"]
    if has_mask:
        assert stats["masked"] >= 0.05
        drops.append("mask")
    if len(shapes) > 1:
        drops.append("start")
    for drop in drops:
        e = _rel(_ref(i, (drop,))[0], base)
        print(f"  without {drop}: moves by {e:.3f}")
        assert e >= 0.05, (drop, e)


def test_small_level_taps_are_always_partly_outside():
    """case 2's last level is 2 x 1: whatever the position, at least one of a sample's four neighbours lies outside it"""
    assert MR.CASES[1][0][-1] == (2, 1)


def test_golden_mask_fractions():
    m = MR.golden_value_mask(G.SHAPES, 2)
    valid = torch.cat([lm.flatten(1) for lm in G.level_masks()], 1).numpy()
    assert np.array_equal(m.astype(bool), ~valid), "msdeform_reference.golden_value_mask is out of step with the golden's masks"
    frac = m.mean(1)
    print("padding fractions of the golden items:", frac)
    assert frac[0] == 0 and 0.5 < frac[1] < 0.7


def test_bi_attention_reference_is_transformers():
    """GroundingDinoBiMultiHeadAttention with both masks, fp32, against the restatement between its projections (projections done here in fp64)"""
    from transformers.models.grounding_dino.modeling_grounding_dino import GroundingDinoBiMultiHeadAttention
    torch.manual_seed(3)
    cfg = G.config()
    m = GroundingDinoBiMultiHeadAttention(cfg).eval().float()
    for p in m.parameters():
        torch.nn.init.normal_(p, std=0.08)
    B, Nv, Lt = 2, 45, 9
    v, t = torch.randn(B, Nv, cfg.d_model), torch.randn(B, Lt, cfg.d_model)
    vmask = torch.zeros(B, Nv, dtype=torch.bool)
    vmask[1, 20:] = True
    tmask = torch.zeros(B, Lt, dtype=torch.bool)
    tmask[0, 7:], tmask[1, 4:] = True, True
    with torch.no_grad():
        (ov, _), (ot, _) = m(v, t, vision_attention_mask=vmask, text_attention_mask=tmask)
    npw = lambda p: p.detach().double().numpy()                                                                # noqa: E731
    lin = lambda l, x: x.double().numpy() @ npw(l.weight).T + npw(l.bias)                                      # noqa: E731
    rv, rt = BR.bi_attention_reference(lin(m.vision_proj, v), lin(m.text_proj, t), lin(m.values_vision_proj, v), lin(m.values_text_proj, t), m.head_dim,
                                       vision_mask=vmask.numpy(), text_mask=tmask.numpy())
    assert m.head_dim == 256 and m.num_heads == 2
    ev = _rel(rv @ npw(m.out_vision_proj.weight).T + npw(m.out_vision_proj.bias), ov.numpy())
    et = _rel(rt @ npw(m.out_text_proj.weight).T + npw(m.out_text_proj.bias), ot.numpy())
    print(f"bi-attention reference vs transformers: vision {ev:.2e} text {et:.2e}")
    assert ev <= 1e-6 and et <= 1e-6
    # and the single-direction restatement is the same arithmetic
    one = BR.masked_attention_reference(lin(m.vision_proj, v), lin(m.text_proj, t), lin(m.values_text_proj, t), 256 ** -0.5, tmask.numpy())
    assert np.array_equal(one, rv)


def test_expected_names_are_transformers_names():
    from theatergen_amd.grounding_dino_encoder import expected_names
    enc = G.hf_encoder()
    assert expected_names(enc.config) == {"encoder." + k for k in enc.state_dict()}


def test_fixture_generator_reproduces_the_stored_checksums():
    z = np.load(G.PATH)
    w = G.make_weights()
    np.testing.assert_allclose(G.weight_checksums(w), z["weight_checksums"], rtol=0, atol=1e-9)
    assert np.array_equal(z["rows"], G.rows()) and 120 <= len(z["rows"]) <= 200
    assert z["layer1_vision"].shape == (2, len(z["rows"]), G.D_MODEL) and z["layer1_text"].shape == (2, G.TEXT_LEN, G.D_MODEL)
    assert os.path.getsize(G.PATH) < 800 * 1024
    for name in ("bf16", "f16"):
        for q in G.QUANTITIES:
            for side in ("vision", "text"):
                e = z[f"emu_{name}_{q}_{side}"]
                assert e.shape == (2,) and 0 < e[0] < 0.05 and 0 < e[1] < 0.1


def test_config_refusals_name_the_field():
    from types import SimpleNamespace
    from theatergen_amd.grounding_dino_encoder import check_config
    good = dict(d_model=256, encoder_attention_heads=8, encoder_ffn_dim=2048, encoder_layers=6, num_feature_levels=4, encoder_n_points=4,
                activation_function="relu")
    check_config(SimpleNamespace(**good))
    check_config(G.config())
    for change, word in ((dict(d_model=512), "d_model"), (dict(encoder_n_points=8), "encoder_n_points"), (dict(num_feature_levels=5), "num_feature_levels"),
                         (dict(encoder_ffn_dim=1024), "encoder_ffn_dim"), (dict(activation_function="gelu"), "activation_function")):
        with pytest.raises(NotImplementedError, match=word):
            check_config(SimpleNamespace(**dict(good, **change)))


def test_state_dict_mismatch_is_an_error():
    from theatergen_amd.grounding_dino_encoder import GroundingDinoFusionEncoder
    w = {k: torch.from_numpy(v) for k, v in G.make_weights().items()}
    w.pop("encoder.layers.0.fusion_layer.vision_param")
    with pytest.raises(RuntimeError, match="missing"):
        GroundingDinoFusionEncoder(G.config(), w, "cpu", torch.bfloat16)
    w = {k: torch.from_numpy(v) for k, v in G.make_weights().items()}
    w["encoder.layers.0.extra.weight"] = torch.zeros(1)
    with pytest.raises(RuntimeError, match="unexpected"):
        GroundingDinoFusionEncoder(G.config(), w, "cpu", torch.bfloat16)


def _declared(header, name):
    m = re.search(r"^int " + name + r"\s*\(([^;]*)\);", header, flags=re.M | re.S)
    assert m, f"{name} is not declared"
    kinds = {"int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float}
    from theatergen_amd import _lib
    ptr = lambda p: C.POINTER(_lib.AttnDesc) if "tg_attn_desc" in p else C.c_void_p                             # noqa: E731
    return [ptr(p) if "*" in p else kinds[p.split()[0]] for p in (q.strip() for q in m.group(1).replace("\n", " ").split(","))]


def test_abi_entries_header_binding_and_symbols_agree():
    from theatergen_amd import _lib
    header = open(os.path.join(ROOT, "include", "theatergen_hip.h")).read()
    assert re.search(r"#define TG_ABI_VERSION 308\b", header) and _lib.ABI_VERSION == 308
    h = _lib.lib()
    for name in ("tg_msdeform_attn", "tg_attention_wide_kmask"):
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int32 and args == _declared(header, name), name
        assert getattr(h, name) is not None

    # host validation, fake pointers (never read): each refusal names the entry point
    shapes = (C.c_int32 * 8)(7, 5, 4, 3, 2, 2, 1, 1)

    def call(dtype=0, batch=1, heads=1, hd=32, L=1, P=4, nq=5, R=2, sh=shapes, value=64, v_ld=32, off=64, off_ld=8, log=64, log_ld=4, ref=64, out=64,
             out_ld=32, out_bs=0):
        return h.tg_msdeform_attn(dtype, batch, heads, hd, L, P, nq, R, sh, value, v_ld, 0, off, off_ld, log, log_ld, ref, None, out, out_ld, out_bs, None)
    bad_shape = (C.c_int32 * 2)(0, 5)
    for kw, code in ((dict(hd=64), -3), (dict(P=8), -3), (dict(L=5), -3), (dict(L=0), -3), (dict(R=3), -3), (dict(dtype=2), -1), (dict(nq=0), -1),
                     (dict(value=72), -1), (dict(log=68), -1), (dict(v_ld=36), -1), (dict(off_ld=4), -1), (dict(log_ld=2), -1), (dict(out=0), -1),
                     (dict(sh=bad_shape), -1), (dict(batch=2, out_bs=32), -1), (dict(heads=2), -1)):
        assert call(**kw) == code, kw
        assert b"tg_msdeform_attn" in h.tg_last_error()

    d = _lib.AttnDesc()
    d.dtype, d.batch, d.heads, d.head_dim, d.n_q, d.len0, d.scale = 0, 1, 1, 256, 4, 40, 1.0
    d.q, d.k0, d.vt0, d.out = 64, 64, 64, 64
    d.q_ld = d.k0_ld = d.out_ld = 256
    d.vt0_ld = 40
    for kw, code in ((dict(mask=0), -1), (dict(mask=68), -1), (dict(splits=0), -1), (dict(splits=2), -1), (dict(hd=128), -3), (dict(len0=36), -1)):
        d.head_dim, d.len0 = kw.get("hd", 256), kw.get("len0", 40)
        assert h.tg_attention_wide_kmask(C.byref(d), kw.get("mask", 64), 40, kw.get("splits", 1), None, 0, None) == code, kw
        assert b"tg_attention_wide_kmask" in h.tg_last_error()


def test_wrapper_refusals_without_a_device():
    from theatergen_amd import ops
    x = torch.zeros(8, 256, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.msdeform_attn(x, 32, 0, [(2, 2)], x, 8, x, 4, torch.zeros(1, 1, 1, 2), 1, 1, 1, x, 32, 0)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.attention_wide(x, 256, 0, x, 256, 0, x, 8, 0, 8, 1, 1, 256, 8, 1.0, x, 256, 0, key_mask=torch.zeros(1, 8, dtype=torch.uint8))
