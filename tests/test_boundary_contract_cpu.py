"""CPU: tests/boundary_contract.py proved without a kernel.

  * every fp64 restatement equals torch's own fp64 ``conv2d`` / ``softmax`` / ``gelu`` / ``silu`` / ``permute`` to 1e-12 on every case;
  * ``plan`` gives the kernel and the LDS bytes of a by-hand table for every case: the four LDS-gate brackets (conv_in 64 512 / 65 664 B, conv_out
    64 512 / 65 664 B) and the 163 840 bytes of the matrix-core conv_out at cin 320, cout 8;
  * every fp32 model of a kernel's algorithm passes every case through the judge the GPU test uses (so the operands stay inside the bounds
    without the kernel), in both storage types;
  * every injected fault fails at least one case (the table is printed);
  * the argument checks of the entries, through the loaded library, decided on the host before any launch.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import boundary_contract as bc

DTYPES = [torch.bfloat16, torch.float16]
ALL_CASES = bc.all_cases()


@functools.lru_cache(maxsize=None)
def _case(cid, dtype):
    entry, kw = ALL_CASES[cid]
    a = bc.make_case(entry, dtype, **kw)
    return a, bc.reference(a)


def _rel(got, want):
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-300)


# ---- the restatement against torch's fp64 operators ------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c for c in ALL_CASES if c.split(" ")[0] in ("conv_in", "conv_out")])
def test_conv_restatement_is_torch_conv2d(cid):
    a, (ref, _) = _case(cid, torch.bfloat16)
    ext = bc._ext(a)
    cin, cout = a["cin"], a["cout"]
    W = ext["weight"].reshape(cout, 3, 3, cin).permute(0, 3, 1, 2)
    if a["entry"] == "conv_in":
        want = F.conv2d(ext["sample"], W, ext["bias"], padding=1).permute(0, 2, 3, 1).reshape(-1, cout)
    else:
        x = ext["x"]
        if a.get("coef") is not None:
            f = x * ext["coef"][:, 0][:, None, None, :] + ext["coef"][:, 1][:, None, None, :]
            x = (F.silu(f) if a["a_silu"] else f).to(a["dtype"]).double()
        want = F.conv2d(x.permute(0, 3, 1, 2), W, ext["bias"], padding=1)
    assert _rel(ref["out"], want) <= 1e-12


@pytest.mark.parametrize("cid", [c for c in ALL_CASES if c.split(" ")[0] in ("transpose", "softmax", "probs", "geglu", "act", "add", "timestep")])
def test_glue_restatements_are_torch_operators(cid):
    a, (ref, _) = _case(cid, torch.float16)
    e, ext = a["entry"], bc._ext(a)
    if e == "transpose":
        want = ext["src"].permute(0, 2, 1)
        assert torch.equal(ref["dst"], want)
        return
    if e == "softmax_rows":
        got, want = ref["out"], torch.softmax(bc._f32(a["scale"]) * ext["x"], -1)
    elif e == "attn_probs":
        nb, H = a["batch"] - a["b0"], a["heads"]
        q = a["q"].cpu().double().reshape(a["batch"], -1)[a["b0"]:, :a["n_q"] * a["q_ld"]].reshape(nb, a["n_q"], a["q_ld"])[..., :H * a["head_dim"]]
        k = a["k"].cpu().double().reshape(a["batch"], -1)[a["b0"]:, :a["len"] * a["k_ld"]].reshape(nb, a["len"], a["k_ld"])[..., :H * a["head_dim"]]
        q, k = (t.reshape(nb, -1, H, a["head_dim"]).permute(0, 2, 1, 3) for t in (q, k))
        want = torch.softmax(bc._f32(a["scale"]) * q @ k.transpose(-1, -2), -1)
        if a["tokens"] is not None:
            want = want[..., a["tokens"].long()]
        got = ref["probs"]
    elif e == "geglu":
        i = a["inner"]
        got, want = ref["out"], ext["x"][:, :i] * F.gelu(ext["x"][:, i:])
    elif e == "act":
        x = ext["x"]
        got, want = ref["out"], {1: F.silu(x), 2: F.gelu(x), 3: x * torch.sigmoid(1.702 * x)}.get(a["act"], x)
    elif e == "add":
        got, want = ref["out"], ext["a"] + ext["b"]
    else:
        from oracle import unet as ou
        got = ref["out"]
        want = ou.timestep_sinusoid(ext["t"], a["dim"], bool(a["flip"]), a["freq_shift"]).double()
        assert float((got - want).abs().max()) <= float(ext["t"].abs().max()) * 4 * bc.timestep_freq_eps() + 1e-6      # the oracle is fp32
        return
    assert _rel(got, want) <= 1e-12


def test_timestep_frequency_error_is_measured_on_the_oracle():
    """the worst relative error of the oracle's fp32 frequencies: about |exponent| x 2^-24 (ln(10000) = 9.2); the bound allows 4 x that"""
    eps = bc.timestep_freq_eps()
    print(f"timestep frequencies: oracle fp32 against fp64 eps = {eps:.3e}, allowance {bc.TIMESTEP_EPS_FACTOR * eps:.3e}")
    assert 2.0 ** -25 < eps < 16 * 9.3 * 2.0 ** -24


# ---- plan against the by-hand table ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c for c in ALL_CASES if bc.expected_kernel(c) is not None])
def test_plan_matches_the_table(cid):
    a, _ = _case(cid, torch.bfloat16)
    kernel, lds = bc.expected_kernel(cid)
    p = bc.plan(a)
    assert p["kernel"] == kernel and (lds is None or p["lds"] == lds), (p, kernel, lds)
    if a["entry"] == "conv_in":
        assert (kernel == "conv_in_mfma_kernel") <= bc.takes_dup(a["cin"], a["cout"])
    if a["entry"] == "conv_out":
        assert (kernel == "conv_out_mfma_kernel") == bc.takes_coef(a["cin"], a["h"], a["w"], a["cout"])
    assert (p["trips"] >= 2) == ("trip2" in cid)


def test_lds_gate_brackets_and_trip_counts():
    assert bc.conv_in_fast_lds(4, 440)[0] == 64512 and bc.conv_in_fast_lds(4, 448)[0] == 65664
    assert 9 * 448 * 8 * 2 == 64512 and 9 * 456 * 8 * 2 == 65664 and 9 * 512 * 8 * 2 == 73728
    assert bc.conv_out_mfma_lds(320, 8) == 163840 == 160 * 1024
    assert bc.conv_in_fast_lds(4, 24) == (27936, 85) and 85 * 3 == 255                       # one idle thread
    a, _ = _case("conv_out 2x8x32x128x4-gn-f32", torch.float16)
    assert bc.plan(a)["kernel"] == "conv_out_mfma_kernel"
    r = bc.make_case(*bc.CONV_OUT_REFUSED[:1], torch.float16, **bc.CONV_OUT_REFUSED[1])
    assert bc.plan(r)["kernel"] == "refused" and not bc.takes_coef(r["cin"], r["h"], r["w"], r["cout"])
    for cid, trips in (("geglu 1030x4104", 2), ("act n600000-act1", 2), ("add n4200005", 2), ("add n9", 1), ("dup_rows 1030x4104ld4112", 2),
                       ("gaussian 2x4x70001", 2), ("add_noise 3x180001", 2), ("shift 8x300x231-3+5", 2), ("compose 8x70001", 2), ("blend 8x70001-f16", 2),
                       ("timestep d1280f1s1-idx11-ts3r5p16", 5), ("timestep d256f1s0-ts1r5p0", 1)):
        assert bc.plan(_case(cid, torch.float16)[0])["trips"] == trips, cid


# ---- the models through the judge ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cid", list(ALL_CASES))
def test_model_passes_the_judge(cid, dtype):
    a, (ref, mag) = _case(cid, dtype)
    for r in bc.read_extents(a) + bc.written_region(a):
        r.view()                                                                             # inside its storage
    fails, metrics = bc.judge(a, bc.model(a), ref, mag)
    assert not fails, fails
    assert all(m["finite"] for m in metrics.values())


# fault -> the cases it is tried on (the smallest that cross the edge it breaks)
FAULT_CASES = {
    "pair_image_of_first": ("conv_in 3x5x7x3x16", "conv_out 3x5x7x64x3-f32", "conv_out 3x5x7x8x8-st"),
    "k_last_chunk_dropped": ("conv_in 3x5x7x4x320", "conv_in 3x5x7x8x64", "conv_out 1x3x5x456x8-f32", "conv_out 3x5x7x64x4-f32", "conv_out 3x8x16x64x1-f32"),
    "border_le": ("conv_in 3x5x7x4x320", "conv_in 3x5x7x4x24", "conv_in 3x5x7x4x5", "conv_out 3x5x7x64x3-f32", "conv_out 2x3x5x512x8-st",
                  "conv_out 1x16x16x192x5-f32"),
    "bias_before_halves": ("conv_in 3x5x7x4x320", "conv_in 2x1x40x4x480", "conv_in 1x9x1x4x640"),
    "prologue_on_padding": ("conv_out 2x8x32x128x4-gn-silu-f32", "conv_out 2x8x32x128x4-gn-st"),
    "second_trip_skipped": ("conv_in 2x260x260x4x160-trip2", "conv_in 1x130x130x3x128-trip2", "conv_out 2x97x96x64x4-trip2-f32", "geglu 1030x4104",
                            "act n600000-act3", "add n4200005", "dup_rows 1030x4104ld4112", "gaussian 2x4x70001", "add_noise 3x180001",
                            "shift 8x300x231-3+5", "compose 8x70001", "blend 8x70001-f16"),
    "transpose_ragged_dropped": ("transpose 1x127x64", "transpose 1x128x63", "transpose 3x1x1", "transpose 2x33x65"),
    "softmax_max_unscaled": ("softmax 5x72ld80", "softmax 4x512ld512-inplace"),
    "probs_slot_ignored": ("probs L77d40q5b0-tokens", "probs L256d64q5b0-pitched-tokens", "probs L65d64q1b0-tokens"),
    "add_tail_dropped": ("add n1", "add n7", "add n9", "add n4200005"),
}


def test_every_fault_is_tried_and_every_trial_fails():
    assert set(FAULT_CASES) == set(bc.FAULTS) and len(bc.FAULTS) >= 10
    table = {}
    for fault, cids in FAULT_CASES.items():
        for cid in cids:
            for dtype in DTYPES:
                a, (ref, mag) = _case(cid, dtype)
                fails, _ = bc.judge(a, bc.model(a, fault), ref, mag)
                table[(fault, cid, str(dtype))] = bool(fails)
    for fault in bc.FAULTS:
        rows = {k: v for k, v in table.items() if k[0] == fault}
        print(f"{fault}: caught in {sum(rows.values())} of {len(rows)} trials")
    missed = [k for k, v in table.items() if not v]
    assert not missed, f"faults that passed the judge: {missed}"


def test_faults_leave_the_other_branches_alone():
    """a switch changes only the branch it names: the aligned tile of the big transpose, an add without a tail, tokens below 64"""
    for fault, cid in (("transpose_ragged_dropped", "transpose 2x256x192"), ("add_tail_dropped", "add n8"), ("probs_slot_ignored", "probs L63d40q5b0"),
                       ("pair_image_of_first", "conv_out 1x8x16x384x4-f32"), ("second_trip_skipped", "add n9")):
        a, (ref, mag) = _case(cid, torch.float16)
        assert not bc.judge(a, bc.model(a, fault), ref, mag)[0], (fault, cid)


def test_unread_input_elements_hold_nan():
    """pad columns, guard rows, the rows of items below b0, the unread entries of the timestep table"""
    for cid in ("softmax 5x72ld80", "probs L65d40q5b1-pitched", "timestep d320f1s0-idx7-ts0r3p8", "dup_rows 3x24ld40", "conv_in 3x5x7x4x320",
                "gaussian 2x4x35-mode"):
        a, _ = _case(cid, torch.bfloat16)
        for r in bc.read_extents(a):
            if not r.t.is_floating_point():
                continue
            base = torch.empty(0, dtype=r.t.dtype).set_(r.t.untyped_storage(), 0, (r.t.untyped_storage().nbytes() // r.t.element_size(),), (1,))
            mask = torch.zeros(base.numel() * r.t.element_size(), dtype=torch.bool)
            for q in bc.read_extents(a):
                if q.t.untyped_storage().data_ptr() == r.t.untyped_storage().data_ptr():
                    q.byte_view(mask).fill_(True)
            unread = ~mask.reshape(-1, r.t.element_size())[:, 0]
            assert bool(unread.any()) and bool(torch.isnan(base[unread]).all()), (cid, r.name)
            assert not bool(torch.isnan(base[~unread]).any()), (cid, r.name)


# ---- refusals on the host, before any launch ---------------------------------------------------------------------------------------------
def test_entries_refuse_bad_arguments_on_the_host():
    from theatergen_amd import _lib
    h = _lib.lib()
    P = 4096                                                                                     # a non-NULL, 16-byte aligned pointer that is never followed
    ARG, UNSUP = -1, -3
    # tg_conv_in / tg_conv_in_dup: h, w > 0
    assert h.tg_conv_in(0, P, 2, 1, 4, 0, 16, P, None, 320, P, None) == ARG and b"tg_conv_in" in h.tg_last_error()
    assert h.tg_conv_in_dup(0, P, 2, 1, 4, 16, 0, P, None, 320, P, 0, None) == ARG
    assert h.tg_conv_in_dup(0, P, 2, 1, 4, 16, -3, P, None, 64, P, 0, None) == ARG
    # tg_conv_out / tg_conv_out_gn: h, w > 0, cout <= 8, cin % 8, NULL coef, coef on a problem the matrix-core kernel refuses
    assert h.tg_conv_out(0, P, 1, 64, 0, 16, P, None, 4, P, 1, None) == ARG and b"tg_conv_out" in h.tg_last_error()
    assert h.tg_conv_out(0, P, 1, 64, 8, 0, P, None, 4, P, 1, None) == ARG
    assert h.tg_conv_out(0, P, 1, 64, 8, 16, P, None, 9, P, 1, None) == ARG
    assert h.tg_conv_out(0, P, 1, 60, 8, 16, P, None, 4, P, 1, None) == ARG
    assert h.tg_conv_out(0, P, 1, 0, 8, 16, P, None, 4, P, 1, None) == ARG
    assert h.tg_conv_out_gn(0, P, None, 1, 1, 64, 8, 16, P, None, 4, P, 1, None) == ARG and b"null coef" in h.tg_last_error()
    assert h.tg_conv_out_takes_coef(128, 8, 24, 4) == 0
    assert h.tg_conv_out_gn(0, P, P, 1, 2, 128, 8, 24, P, None, 4, P, 1, None) == UNSUP and b"tg_conv_out_takes_coef" in h.tg_last_error()
    # tg_attn_probs: len <= 256, pitches that keep the 16-byte loads aligned, head_dim > 0, n_tokens > 0 with tokens
    ok = dict(dtype=0, batch=2, b0=0, heads=2, head_dim=40, n_q=5, q=P, q_ld=80, q_bs=400, k=P, k_ld=80, k_bs=6160, len=77, scale=0.158, tokens=None, n_tokens=0,
              probs=P, stream=None)
    for bad in (dict(len=257), dict(len=0), dict(q_ld=84), dict(k_ld=81), dict(head_dim=0), dict(head_dim=44), dict(tokens=P, n_tokens=0),
                dict(tokens=P, n_tokens=-2), dict(b0=2), dict(n_q=0)):
        assert h.tg_attn_probs(*dict(ok, **bad).values()) == ARG, bad
        assert b"tg_attn_probs" in h.tg_last_error()
    # the queries, against the Python statement of the gates
    for cin, cout in ((4, 160), (4, 320), (4, 640), (4, 800), (4, 64), (3, 160), (8, 320), (4, 0)):
        assert h.tg_conv_in_takes_dup(cin, cout) == int(bc.takes_dup(cin, cout))
    for cin, hh, ww, cout in ((320, 8, 16, 8), (384, 8, 16, 4), (64, 8, 16, 9), (64, 7, 16, 4), (64, 8, 24, 4), (32, 8, 16, 4), (64, 97, 96, 4), (128, 8, 32, 4)):
        assert h.tg_conv_out_takes_coef(cin, hh, ww, cout) == int(bc.takes_coef(cin, hh, ww, cout))
