"""GPU: ``tg_msdeform_attn`` and ``attention_wide(key_mask=)`` against the fp64 restatements of their contracts (tests/msdeform_reference.py,
tests/bi_attention_reference.py), their refusals, and ``GroundingDinoFusionEncoder`` against the transformers golden
(tests/golden/make_grounding_dino_encoder_golden.py) and inside an attached model.

Bounds: ``op_tol`` for ``msdeform_attn`` (a launch against fp64 from the stored operands: fp32 arithmetic and one rounding, as ``tg_attention_swin``);
the format bound of tests/test_attn_wide_gpu.py for the masked wide attention (its second bound there, against the materialised route, has no masked
counterpart); for the encoder, per quantity, TWICE the error of the rounded emulation stored in the golden (weights, inputs and every Linear / LayerNorm
output rounded to the storage dtype inside transformers' encoder): the device rounds at other points (P, folded epilogues) and sums in another order, an
independent rounding set of similar size adds about sqrt(2), and a wrong tap, mask or weight moves these quantities by >= 0.05 (CPU sensitivity test).
"""
import functools

import numpy as np
import pytest
import torch

from tests import bi_attention_reference as BR
from tests import msdeform_reference as MR
from tests import parity_metrics as pm
from tests.golden import make_grounding_dino_encoder_golden as G

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
GUARD = 4096


def op_tol(dtype):
    return 1.5e-2 if dtype == torch.bfloat16 else 4e-3


def fmt_bound(dtype):
    return 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11


# ---- msdeform_attn ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ms_case(i, dname):
    """stored operands (host tensors in the storage dtype; ref fp32) and the fp64 reference from them: computed once per (case, dtype)"""
    dt = DTYPES[dname]
    rnd = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(dt).double().numpy()           # noqa: E731
    value, offsets, logits, ref, mask = MR.make_case(MR.CASES[i], seed=100 + i, round_to=rnd)
    want = MR.msdeform_reference(value, MR.CASES[i][0], offsets, logits, ref, mask)
    to = lambda a: torch.from_numpy(a).to(dt)                                                      # noqa: E731
    return (to(value), to(offsets), to(logits), torch.from_numpy(ref).float(), None if mask is None else torch.from_numpy(mask),
            torch.from_numpy(want))


def _ms_launch(shapes, value, offsets, logits, ref, mask, fill=float("nan")):
    """device operands -> (out [B, Nq, C], the guard band behind it).  Offsets and logits are two column slices of one buffer, as the encoder's GEMM
    writes them."""
    from theatergen_amd import ops
    B, Nv, C = value.shape
    heads = C // 32
    Nq, L = offsets.shape[1], len(shapes)
    n_off, n_log = heads * L * 8, heads * L * 4
    ld = (n_off + n_log + 7) // 8 * 8                        # the row pitch keeps the 16-byte offset loads aligned (heads * L odd: 4 spare columns)
    ol = torch.full((B * Nq, ld), float("nan"), dtype=value.dtype, device=value.device)
    ol[:, :n_off], ol[:, n_off:n_off + n_log] = offsets.reshape(B * Nq, n_off), logits.reshape(B * Nq, n_log)
    buf = torch.full((B * Nq * C + GUARD,), fill, dtype=value.dtype, device=value.device)
    ops.msdeform_attn(value, C, Nv * C, shapes, ol, ld, ol[:, n_off:], ld, ref, B, heads, Nq, buf, C, Nq * C, value_mask=mask)
    torch.cuda.synchronize()
    return buf[:B * Nq * C].reshape(B, Nq, C), buf[B * Nq * C:]


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("i", range(len(MR.CASES)), ids=MR.IDS)
def test_msdeform_attn_against_fp64_contract(i, dname):
    """Measured rel-L2 / max on the four cases: bf16 1.66e-3 .. 1.69e-3 / 1.64e-3 .. 3.34e-3, f16 2.04e-4 .. 2.09e-4 / 2.38e-4 .. 3.58e-4."""
    shapes = MR.CASES[i][0]
    dt = DTYPES[dname]
    value, offsets, logits, ref, mask, want = _ms_case(i, dname)
    dev = [None if t is None else t.cuda() for t in (value, offsets, logits, ref, mask)]
    out, guard = _ms_launch(shapes, *dev)
    m = pm.metrics(out.float().cpu(), want)
    tol = op_tol(dt)
    print(f"msdeform_attn {MR.IDS[i]} {dname}: rel-L2 {m['rel_l2']:.3e} max {m['max_rel']:.3e} (tolerance {tol / 2:.1e} / {tol:.1e})")
    assert bool(torch.isfinite(out).all()), "an output element was not written (NaN fill survives)"
    assert bool(torch.isnan(guard).all()), "the guard band after out was written"
    pm.check(out.float().cpu(), want, f"msdeform_attn {MR.IDS[i]} {dname}", tol / 2, tol)
    again, _ = _ms_launch(shapes, *dev)
    assert torch.equal(out.view(torch.int16), again.view(torch.int16)), "two launches differ"
    if value.shape[0] > 1:
        one, _ = _ms_launch(shapes, *[None if t is None else t[1:2].contiguous() for t in dev])
        assert torch.equal(one[0].view(torch.int16), out[1].view(torch.int16)), "batch item 1 depends on the batch"


def test_msdeform_attn_refusals_leave_out_untouched():
    from theatergen_amd import ops
    dt = torch.bfloat16

    def call(heads=1, hd=32, P=4, shapes=((4, 3),), R=2, off=0, nq=6, out_rows=None, mask_dtype=None, ref_dtype=torch.float32):
        C, L = heads * hd, len(shapes)
        nv = sum(h * w for h, w in shapes)
        flat = torch.zeros((nv * C + 16,), dtype=dt, device="cuda")
        value = flat[off:off + nv * C].reshape(1, nv, C)
        ol = torch.zeros((nq, (heads * L * P * 3 + 7) // 8 * 8 + 8), dtype=dt, device="cuda")      # a row pitch that keeps the load widths
        ref = torch.zeros((1, nq, L, R), dtype=ref_dtype, device="cuda")
        out = torch.full((nq if out_rows is None else out_rows, C), 7.0, dtype=dt, device="cuda")
        mask = None if mask_dtype is None else torch.zeros((1, nv), dtype=mask_dtype, device="cuda")
        with pytest.raises(RuntimeError) as e:
            ops.msdeform_attn(value, C, nv * C, shapes, ol, ol.stride(0), ol[:, heads * L * P * 2:], ol.stride(0), ref, 1, heads, nq, out, C, nq * C,
                              value_mask=mask, head_dim=hd, n_points=P)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()), "a refused call wrote to out"
        return str(e.value)
    assert "error -3" in call(hd=64)
    assert "error -3" in call(P=8)
    assert "error -3" in call(shapes=((2, 2),) * 5)
    assert "error -3" in call(R=3)
    assert "error -1" in call(off=4)                       # value 8 bytes off a 16-byte boundary
    assert "msdeform_attn" in call(out_rows=5)             # the wrapper: out one row short
    assert "msdeform_attn" in call(mask_dtype=torch.bool)  # the wrapper: the mask is uint8
    assert "msdeform_attn" in call(ref_dtype=torch.float16)


# ---- attention_wide(key_mask=) -------------------------------------------------------------------------------------------------------------------------
def _wide(q, k, v, mask, splits, fill=float("nan")):
    """q [B, n_q, C], k / v [B, len, C] on the device (len a multiple of 8), mask uint8 [B, len] or None -> out [B, n_q, C]"""
    from theatergen_amd import ops
    B, n_q, C = q.shape
    n = k.shape[1]
    vt = v.transpose(1, 2).contiguous()
    out = torch.full((B, n_q, C), fill, dtype=q.dtype, device=q.device)
    ops.attention_wide(q, C, n_q * C, k, C, n * C, vt, n, C * n, n, B, C // 256, 256, n_q, 256 ** -0.5, out, C, n_q * C, key_splits=splits, key_mask=mask)
    torch.cuda.synchronize()
    return out


def _wide_inputs(dt, B, heads, n_q, n, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, r, heads * 256, generator=g).to(dt) for r in (n_q, n, n)]


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("case", ["random_mask", "full_tile", "full_split"])
def test_attention_wide_key_mask_against_fp64(case, dname):
    """n_q 5 / len 40 with a random mask; n_q 130 / len 96 with keys 32 - 63 (one whole 32-key tile) masked, unsplit and with key_splits = 3 (one whole
    split: its partial is (m, l, o) = (-inf, 0, 0))."""
    dt = DTYPES[dname]
    B, heads = 2, 2
    if case == "random_mask":
        n_q, n, splits = 5, 40, None
        mask = (torch.rand(B, n, generator=torch.Generator().manual_seed(5)) < 0.4).to(torch.uint8)
        mask[:, 3] = 0
    else:
        n_q, n, splits = 130, 96, (3 if case == "full_split" else None)
        mask = torch.zeros(B, n, dtype=torch.uint8)
        mask[:, 32:64] = 1
        mask[1, 70:] = 1
    q, k, v = _wide_inputs(dt, B, heads, n_q, n, seed=11)
    want = torch.from_numpy(BR.masked_attention_reference(q.double().numpy(), k.double().numpy(), v.double().numpy(), 256 ** -0.5, mask.numpy()))
    out = _wide(q.cuda(), k.cuda(), v.cuda(), mask.cuda(), splits)
    assert bool(torch.isfinite(out).all()), "NaN / unwritten output"
    m = pm.metrics(out.float().cpu(), want)
    print(f"attention_wide key_mask {case} {dname}: rel-L2 {m['rel_l2']:.3e} max {m['max_rel']:.3e} (bound {fmt_bound(dt):.3e})")
    assert m["rel_l2"] <= fmt_bound(dt), m
    again = _wide(q.cuda(), k.cuda(), v.cuda(), mask.cuda(), splits)
    assert torch.equal(out.view(torch.int16), again.view(torch.int16)), "two launches differ"
    one = _wide(q[1:2].cuda(), k[1:2].cuda(), v[1:2].cuda(), mask[1:2].cuda(), splits)
    assert torch.equal(one[0].view(torch.int16), out[1].view(torch.int16)), "batch item 1 depends on the batch"


@pytest.mark.parametrize("splits", [None, 3])
def test_attention_wide_zero_mask_is_the_unmasked_call(splits):
    dt = torch.bfloat16
    q, k, v = [t.cuda() for t in _wide_inputs(dt, 2, 2, 130, 96, seed=12)]
    plain = _wide(q, k, v, None, splits)
    masked = _wide(q, k, v, torch.zeros(2, 96, dtype=torch.uint8, device="cuda"), splits)
    assert torch.equal(plain.view(torch.int16), masked.view(torch.int16))


def test_attention_wide_all_masked_row_is_zero_and_refusals():
    from theatergen_amd import ops
    dt = torch.bfloat16
    q, k, v = [t.cuda() for t in _wide_inputs(dt, 1, 1, 5, 40, seed=13)]
    out = _wide(q, k, v, torch.ones(1, 40, dtype=torch.uint8, device="cuda"), None)
    assert bool((out == 0).all()), "a row with every key masked is documented to be zeros"
    out = _wide(q, k, v, torch.ones(1, 40, dtype=torch.uint8, device="cuda"), 2)
    assert bool((out == 0).all())
    sentinel = torch.full((1, 5, 256), 7.0, dtype=dt, device="cuda")
    vt = v.transpose(1, 2).contiguous()
    for bad in (torch.zeros(1, 40, dtype=torch.bool, device="cuda"), torch.zeros(1, 48, dtype=torch.uint8, device="cuda"),
                torch.zeros(1, 40, dtype=torch.uint8)):
        with pytest.raises(RuntimeError, match="key_mask"):
            ops.attention_wide(q, 256, 5 * 256, k, 256, 40 * 256, vt, 40, 256 * 40, 40, 1, 1, 256, 5, 256 ** -0.5, sentinel, 256, 5 * 256, key_mask=bad)
    torch.cuda.synchronize()
    assert bool((sentinel == 7.0).all())


# ---- the encoder against the golden ----------------------------------------------------------------------------------------------------------------------
def _dev(kw):
    return {k: v.cuda() if isinstance(v, torch.Tensor) else v for k, v in kw.items()}


@functools.lru_cache(maxsize=None)
def _encoder_run(dname):
    """one forward of the device encoder on the golden inputs per dtype, shared by the checks below"""
    from theatergen_amd.grounding_dino_encoder import GroundingDinoFusionEncoder
    w = {k: torch.from_numpy(v) for k, v in G.make_weights().items()}
    enc = GroundingDinoFusionEncoder.from_state_dict(G.config(), w, "cuda", DTYPES[dname])
    enc.taps = []
    out = enc(**_dev(G.inputs()), output_hidden_states=True, return_dict=True)
    torch.cuda.synchronize()
    taps, enc.taps = enc.taps, None
    fus = [t for t in taps if t[0] == "fusion" and t[1] == 0][0]
    got = {"fusion0": (fus[2], fus[3]), "layer0": (out.vision_hidden_states[1], out.text_hidden_states[1]),
           "layer1": (out.last_hidden_state_vision, out.last_hidden_state_text)}
    assert len(out.vision_hidden_states) == G.LAYERS + 1 and out.attentions is None
    return {k: (v.float().cpu(), t.float().cpu()) for k, (v, t) in got.items()}, np.load(G.PATH)


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("side", ["vision", "text"])
@pytest.mark.parametrize("name", G.QUANTITIES)
def test_encoder_against_transformers_golden(name, side, dname):
    """After layer-0 fusion, after layer 0 and after layer 1; vision at the stored rows, text everywhere.  Bound = 2 x the stored error of the rounded
    emulation (rel-L2 and max-rel).  Measured rel-L2, device (emulation), after layer-0 fusion / layer 0 / layer 1: bf16 vision 3.4e-3 (3.0e-3) /
    6.5e-3 (5.9e-3) / 9.7e-3 (8.7e-3), bf16 text 3.4e-3 (2.9e-3) / 5.1e-3 (4.8e-3) / 6.8e-3 (6.5e-3); f16 vision 3.0e-4 (2.1e-4) / 5.6e-4 (4.6e-4) /
    8.9e-4 (7.0e-4), f16 text 2.8e-4 (2.0e-4) / 4.1e-4 (3.6e-4) / 6.1e-4 (5.1e-4); maxima 0.9 - 1.7 x the emulation's
    (profiles/grounding_dino_encoder_findings.md)."""
    got, z = _encoder_run(dname)
    g = got[name][0][:, [int(r) for r in z["rows"]]] if side == "vision" else got[name][1]
    want = torch.from_numpy(z[f"{name}_{side}"])
    emu = z[f"emu_{dname}_{name}_{side}"]
    m = pm.metrics(g, want)
    print(f"grounding dino encoder {dname} {name} {side}: rel-L2 {m['rel_l2']:.3e} max {m['max_rel']:.3e} "
          f"(emulation {emu[0]:.3e} / {emu[1]:.3e}, bound twice that)")
    pm.check(g, want, f"grounding dino encoder {dname} {name} {side}", 2 * float(emu[0]), 2 * float(emu[1]))


def test_encoder_refuses_output_attentions():
    from theatergen_amd.grounding_dino_encoder import GroundingDinoFusionEncoder
    w = {k: torch.from_numpy(v) for k, v in G.make_weights().items()}
    enc = GroundingDinoFusionEncoder.from_state_dict(G.config(), w, "cuda", torch.bfloat16)
    with pytest.raises(NotImplementedError, match="output_attentions"):
        enc(**_dev(G.inputs()), output_attentions=True)


@pytest.mark.parametrize("dname", list(DTYPES))
def test_attached_model_matches_transformers(dname):
    """A tiny fp32 ``GroundingDinoModel`` on the device with and without ``attach`` (encoder in ``dname``): the encoder's last hidden states at the bounds
    of the golden's last layer.  Logits are not asserted: the two-stage top-k behind the encoder is discontinuous.
    Measured rel-L2 / max (bound): bf16 vision 1.00e-2 / 1.38e-2 (1.74e-2 / 3.40e-2), bf16 text 6.9e-3 / 1.07e-2 (1.31e-2 / 2.38e-2), f16 vision
    9.7e-4 / 1.77e-3 (1.41e-3 / 2.12e-3), f16 text 6.7e-4 / 9.5e-4 (1.03e-3 / 1.39e-3)
    (profiles/grounding_dino_encoder_findings.md)."""
    from transformers import GroundingDinoModel
    from theatergen_amd.grounding_dino_encoder import GroundingDinoFusionEncoder
    torch.manual_seed(0)
    model = GroundingDinoModel(G.config()).eval().float()
    w = G.make_weights()
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
    assert not unexpected and not any(k in w for k in missing)
    model = model.to("cuda")
    gen = torch.Generator().manual_seed(9)
    pv = torch.randn((G.BATCH, 3) + G.IMAGE_HW, generator=gen).cuda()
    mask = torch.ones((G.BATCH,) + G.IMAGE_HW, dtype=torch.long)
    mask[1, G.MASK_HW[0]:, :] = 0
    mask[1, :, G.MASK_HW[1]:] = 0
    ids = torch.tensor(G.INPUT_IDS).cuda()
    kw = dict(pixel_values=pv, pixel_mask=mask.cuda(), input_ids=ids, attention_mask=(ids != 0).long(), token_type_ids=torch.zeros_like(ids))
    z = np.load(G.PATH)
    with torch.no_grad():
        ref = model(**kw)
        rv, rt = ref.encoder_last_hidden_state_vision.float().cpu(), ref.encoder_last_hidden_state_text.float().cpu()
        GroundingDinoFusionEncoder.from_state_dict(model.config, model.state_dict(), "cuda", DTYPES[dname]).attach(model)
        got = model(**kw)
    assert got.encoder_last_hidden_state_vision.dtype == torch.float32
    for side, g, r in (("vision", got.encoder_last_hidden_state_vision.float().cpu(), rv), ("text", got.encoder_last_hidden_state_text.float().cpu(), rt)):
        emu = z[f"emu_{dname}_layer1_{side}"]
        m = pm.metrics(g, r)
        print(f"attached model {dname} {side}: rel-L2 {m['rel_l2']:.3e} max {m['max_rel']:.3e} (bound {2 * emu[0]:.3e} / {2 * emu[1]:.3e})")
        pm.check(g, r, f"attached grounding dino encoder {dname} {side}", 2 * float(emu[0]), 2 * float(emu[1]))
