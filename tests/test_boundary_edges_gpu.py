"""GPU: hand-made edge launches of the boundary convolutions and glue kernels (csrc/tg_elementwise.hip and ``tg_attn_probs``), kernel branch by
kernel branch, against the fp64 restatement of their C-ABI contracts (tests/boundary_contract.py).

The entries are called through ``theatergen_amd._lib`` directly, so alignment, pitches and offsets are set by hand.  Every case, in bf16 and fp16,
  * checks that every read and written region lies inside its storage and that no written element is read (but for the in-place operands);
  * fills the output storages (guard rows and pad columns included) with a sentinel byte first and checks that every byte outside the written
    region kept it;
  * judges per element (``boundary_contract.element_bound``, or bit equality where the contract is exact), per block (the block a workgroup, wave
    or thread owns: ``boundary_contract.blocks``) and for the whole tensor;
  * replays once into NaN-filled outputs: the same bits, no NaN (every element written, from the inputs alone);
  * asserts that the kernel ``boundary_contract.plan`` names is the one the gates in C choose, through ``tg_conv_in_takes_dup`` and
    ``tg_conv_out_takes_coef`` (the Python gates cannot drift from the C gates), and that it is the kernel of the by-hand table.
Every element of an input buffer that the contract does not read holds NaN, so a read outside the contract shows in the outputs.

Tolerances (none tuned on a kernel): per element the operation-count bounds derived in ``boundary_contract.element_bound``; whole tensor and every
block at 1.5 x launch_check's per-launch bound.  The fp32 models of the kernels pass every case at these bounds and every injected fault fails
(test_boundary_contract_cpu.py).  Measured figures: profiles/boundary_contract_findings.md.
"""
import pytest
import torch

from tests import boundary_contract as bc
from tests import gemm_contract as gc
from tests import launch_check as lc
from tests import parity_metrics as pm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
SENTINEL = 0xA5
ALL_CASES = bc.all_cases()


def _name(dtype):
    return str(dtype).replace("torch.", "")


def _fam(prefix):
    return [c for c in ALL_CASES if c.split(" ")[0] == prefix]


def launch(a):
    from theatergen_amd import _lib, ops
    L, p, e, s = _lib.lib(), ops._ptr, a["entry"], ops._stream()
    dt = ops._dt(torch.empty(0, dtype=a["dtype"])) if a["dtype"] != torch.float32 else None
    if e == "conv_in":
        args = (dt, p(a["sample"]), a["src_dtype"], a["batch"], a["cin"], a["h"], a["w"], p(a["weight"]), p(a["bias"]), a["cout"], p(a["out"]))
        rc = L.tg_conv_in_dup(*args, a["dup_offset"], s) if a["dup_offset"] else L.tg_conv_in(*args, s)
    elif e == "conv_out":
        tail = (a["batch"], a["cin"], a["h"], a["w"], p(a["weight"]), p(a["bias"]), a["cout"], p(a["out"]), a["out_f32"], s)
        rc = L.tg_conv_out_gn(dt, p(a["x"]), p(a["coef"]), a["a_silu"], *tail) if a["coef"] is not None else L.tg_conv_out(dt, p(a["x"]), *tail)
    elif e == "transpose":
        rc = L.tg_transpose(dt, p(a["src"]), a["batch"], a["rows"], a["cols"], p(a["dst"]), s)
    elif e == "softmax_rows":
        rc = L.tg_softmax_rows(dt, p(a["x"]), a["rows"], a["cols"], a["ldx"], a["scale"], p(a["out"]), a["ldo"], s)
    elif e == "attn_probs":
        rc = L.tg_attn_probs(dt, a["batch"], a["b0"], a["heads"], a["head_dim"], a["n_q"], p(a["q"]), a["q_ld"], a["q_bs"], p(a["k"]), a["k_ld"], a["k_bs"],
                             a["len"], a["scale"], p(a["tokens"]), a["n_tokens"], p(a["probs"]), s)
    elif e == "timestep":
        rc = L.tg_timestep_embedding(dt, p(a["t"]), p(a["index"]), a["t_stride"], a["rows"], a["dim"], a["flip"], a["freq_shift"], p(a["out"]), a["ldo"], s)
    elif e == "geglu":
        rc = L.tg_geglu(dt, p(a["x"]), a["rows"], a["inner"], p(a["out"]), s)
    elif e == "act":
        rc = L.tg_act(dt, p(a["x"]), a["n"], a["act"], p(a["out"]), s)
    elif e == "add":
        rc = L.tg_add(dt, p(a["a"]), p(a["b"]), a["n"], p(a["out"]), s)
    elif e == "dup_rows":
        rc = L.tg_dup_rows(p(a["src"]), p(a["dst"]), a["rows"], a["cols"], a["ld"], dt, s)
    elif e == "conv1x1":
        rc = L.tg_conv1x1_nchw(p(a["x"]), a["batch"], a["cin"], a["cout"], a["hw"], p(a["weight"]), p(a["bias"]), a["in_scale"], p(a["out"]), s)
    elif e == "gaussian":
        rc = L.tg_gaussian_sample(p(a["moments"]), p(a["noise"]), a["batch"], a["channels"], a["hw"], a["scale"], p(a["out"]), s)
    elif e == "add_noise":
        rc = L.tg_add_noise(p(a["x0"]), p(a["noise"]), p(a["ca"]), p(a["cb"]), a["steps"], a["n"], p(a["out"]), s)
    elif e == "shift":
        rc = L.tg_shift(p(a["src"]), a["planes"], a["h"], a["w"], a["dx"], a["dy"], p(a["dst"]), s)
    elif e == "compose":
        rc = L.tg_masked_compose(p(a["dst"]), p(a["src"]), p(a["mask"]), a["planes"], a["hw"], s)
    else:
        assert e == "blend", e
        rc = L.tg_blend_latents(p(a["bg"]), p(a["fg"]), p(a["mask"]), a["planes"], a["hw"], a["ratio"], a["sigma"], a["storage_dtype"], p(a["out"]), s)
    torch.cuda.synchronize()
    return rc


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


def check_gates(a, cid):
    """the kernel ``plan`` names is the one the C gates choose (the two queries), and the one of the by-hand table"""
    from theatergen_amd import _lib
    L, p = _lib.lib(), bc.plan(a)
    if a["entry"] == "conv_in":
        assert L.tg_conv_in_takes_dup(a["cin"], a["cout"]) == int(bc.takes_dup(a["cin"], a["cout"]))
        assert (p["kernel"] == "conv_in_mfma_kernel") == (bc.takes_dup(a["cin"], a["cout"]) and a["out"].data_ptr() % 16 == 0 and a["weight"].data_ptr() % 8 == 0)
    if a["entry"] == "conv_out":
        assert L.tg_conv_out_takes_coef(a["cin"], a["h"], a["w"], a["cout"]) == int(bc.takes_coef(a["cin"], a["h"], a["w"], a["cout"]))
        assert (p["kernel"] == "conv_out_mfma_kernel") == bool(L.tg_conv_out_takes_coef(a["cin"], a["h"], a["w"], a["cout"]))
    want = bc.expected_kernel(cid)
    if want is not None:
        assert p["kernel"] == want[0] and (want[1] is None or p["lds"] == want[1]), (cid, p, want)
    return p


def run_case(cid, dtype, quiet=False):
    """the checks of this file on one launch -> (launch dict, first outputs, {output: metrics})"""
    entry, kw = ALL_CASES[cid]
    a = bc.make_case(entry, dtype, device=DEV, **kw)
    what = f"boundary edge {cid} {_name(dtype)}"
    p = check_gates(a, cid)
    reads, writes = bc.read_extents(a), bc.written_region(a)
    lc.LaunchChecker._check_reads(reads + writes, what)
    masks = lc.LaunchChecker._write_masks(writes)
    lc.LaunchChecker._check_overlap(masks, reads, what, allowed=bc.in_place(a))
    ref, mag = bc.reference(a)                                     # before the launch: an in-place operand is overwritten by it
    bound = bc.element_bound(a, ref, mag)
    keep = {sp: lc._bytes(t).clone() for sp, (t, _) in masks.items()} if bc.in_place(a) else None
    if keep is None:
        for t, _ in masks.values():
            lc._bytes(t).fill_(SENTINEL)
    snaps = lc.LaunchChecker._snapshot(masks)
    assert launch(a) == 0, what
    lc.LaunchChecker._check_outside(masks, snaps, what)
    first = {w.name: w.view().clone() for w in writes}
    fails, metrics = bc.judge(a, first, ref, mag, bound)
    for name, m in metrics.items():
        pm.record(f"{what} {name}", m, kernel=p["kernel"], trips=p["trips"])
        if not quiet or fails:
            print(f"{what} {name} [{p['kernel']}, trips {p['trips']}]: over_bound={m['worst_over_element_bound']:.3f} rel_l2={m['rel_l2']:.3e} "
                  f"max={m['max_rel']:.3e} block={m['block_rel_l2']:.3e}@{m['block_at']} block_max={m['block_max_rel']:.3e}")
    l2, mx = bc.tols(dtype)
    assert not fails, f"{what}: {fails} (tolerances rel-L2 {l2:.1e}, max {mx:.1e}, whole tensor and every block; per-element bounds)"
    # replay: NaN everywhere the launch may write (an in-place operand gets its pre-launch bytes back)
    for sp, (t, _) in masks.items():
        if keep is not None:
            lc._bytes(t).copy_(keep[sp])
        else:
            gc._storage_tensor(t).fill_(float("nan"))
    assert launch(a) == 0, what
    for w in writes:
        again = w.view()
        assert not bool(torch.isnan(again).any()), f"{what}: {w.name} of the replay keeps NaN (an element was not written, or read stale memory)"
        assert torch.equal(_bits(again), _bits(first[w.name])), f"{what}: {w.name} of the replay differs from the first launch"
    return a, first, metrics


def _worst(metrics):
    return max(m["worst_over_element_bound"] for m in metrics.values())


# ---- tg_conv_in / tg_conv_in_dup -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cid", _fam("conv_in"))
def test_conv_in(dtype, cid):
    """the matrix-core kernel (one, two, three and four channel halves, one pixel, a second grid-stride trip, the second destination), the fp32-FMA
    fast kernel (K = 27 and 72, an idle thread, a second trip, the LDS gate from below) and the generic kernel (the LDS gate from above, the VAE
    decoder's 4 -> 512, cin 16, cout 5, a misaligned ``out``); samples in fp32, the storage type and the other half type"""
    a, first, metrics = run_case(cid, dtype, quiet="trip2" in cid)
    if a["dup_offset"]:
        assert torch.equal(_bits(first["out"]), _bits(first["out_dup"])), "both destinations of tg_conv_in_dup hold the same bits"
    assert _worst(metrics) <= 1.0


# ---- tg_conv_out / tg_conv_out_gn ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cid", _fam("conv_out"))
def test_conv_out(dtype, cid):
    """the matrix-core kernel (the 160 KiB LDS edge, cout 1 and 5, the GroupNorm prologue with and without SiLU), fast<4> and fast<8> (an odd pixel
    count: a pair straddles two images; nine active lanes; the LDS gate from below; a second trip) and the generic kernel (the gate from above, the
    VAE encoder's 512 -> 8), each for an fp32 and a storage-type output"""
    a, first, metrics = run_case(cid, dtype, quiet="trip2" in cid)
    assert _worst(metrics) <= 1.0
    if a["coef"] is not None:
        # the same kernel on the restatement's rounded activations: the prologue changes nothing but the staged operand
        b = bc.plain_twin(a, DEV)
        assert bc.plan(b)["kernel"] == bc.plan(a)["kernel"] == "conv_out_mfma_kernel"
        assert launch(b) == 0
        assert torch.equal(_bits(bc.written_region(b)[0].view()), _bits(first["out"])), \
            f"{cid}: tg_conv_out_gn differs from tg_conv_out on the normalised activations rounded to the storage type"


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv_out_gn_is_refused_where_the_matrix_core_kernel_is(dtype):
    """``coef`` on a problem tg_conv_out_takes_coef refuses (w % 16): TG_ERR_UNSUPPORTED, and the output keeps its sentinel bytes"""
    from theatergen_amd import _lib
    entry, kw = bc.CONV_OUT_REFUSED
    a = bc.make_case(entry, dtype, device=DEV, **kw)
    assert _lib.lib().tg_conv_out_takes_coef(a["cin"], a["h"], a["w"], a["cout"]) == 0 and bc.plan(a)["kernel"] == "refused"
    lc._bytes(a["out"]).fill_(SENTINEL)
    assert launch(a) == -3 and b"tg_conv_out_takes_coef" in _lib.lib().tg_last_error()
    assert bool((lc._bytes(a["out"]) == SENTINEL).all())
    a["coef"] = None                                                                            # the plain entry takes it (fast<4>)
    assert bc.plan(a)["kernel"] == "conv_out_fast_kernel<4>" and launch(a) == 0


# ---- tg_transpose, tg_dup_rows -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cid", _fam("transpose"))
def test_transpose(dtype, cid):
    """the 128 x 64 tile kernel (one tile, several tiles and items), the 32 x 32 kernel on ragged rows, ragged columns, one element, both ragged, and
    on a tile-sized problem whose ``src`` is not 16-byte aligned: bit equality"""
    run_case(cid, dtype)


# ---- tg_softmax_rows, tg_attn_probs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cid", _fam("softmax"))
def test_softmax_rows(dtype, cid):
    """one chunk, a partly filled wave with pad columns, 512 columns in place, lane 0 with two chunks, 4096 columns; a row of equal values, a row with
    -inf entries, rows near +60000 and -60000 at scale 0.044"""
    a, first, metrics = run_case(cid, dtype)
    assert _worst(metrics) <= 1.0
    s = first["out"].double().sum(-1)
    assert float((s - 1).abs().max()) <= bc.unit_roundoff(dtype) + 1e-5, "the roundings of a row's probabilities add up to at most one unit roundoff"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cid", _fam("probs"))
def test_attn_probs(dtype, cid):
    """len 1 / 63 / 64 / 65 / 77 / 256, head dims 8 / 40 / 64 / 160, 1 / 5 / 64 queries, b0 0 and 1 of 2 items (the rows of item 0 hold NaN), pitched
    rows and batch strides, all columns or a token list with tokens in every slot and duplicates"""
    a, first, metrics = run_case(cid, dtype)
    assert _worst(metrics) <= 1.0
    if a["tokens"] is None:
        assert float((first["probs"].double().sum(-1) - 1).abs().max()) <= 5e-5                  # fp32 rows: softmax_count(4, 256) 2^-24 (1 + ln 256) = 2e-5


# ---- tg_timestep_embedding ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cid", _fam("timestep"))
def test_timestep_embedding(dtype, cid):
    """dims 256 / 320 / 1280 (five trips of 128 threads), both flips and freq_shifts, t direct or through ``index`` into a 50-entry table whose other
    entries hold NaN, t_stride 0 / 1 / 3, ldo > dim; t in {0, 1, 500, 981, 999}"""
    _, _, metrics = run_case(cid, dtype)
    assert _worst(metrics) <= 1.0


# ---- tg_geglu, tg_act, tg_add ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cid", _fam("geglu") + _fam("act") + _fam("add"))
def test_geglu_act_add(dtype, cid):
    """one vector, odd sizes and a size past the 2048-workgroup cap each; every act code and an unknown one (the identity, bit-equal); the n % 8 tail
    of tg_add with 0, 1, 5 and 7 elements"""
    a, _, metrics = run_case(cid, dtype, quiet=True)
    assert _worst(metrics) <= 1.0
    if any(k in cid for k in ("1030x4104", "n600000", "n4200005")):
        assert bc.plan(a)["trips"] == 2


# ---- the fp32 helpers --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(bc.HELPER_CASES))
def test_fp32_helpers(cid):
    """tg_dup_rows, tg_conv1x1_nchw, tg_gaussian_sample (mode, sample, logvar clamped at both ends), tg_add_noise (three steps), tg_shift (|dx| >= w),
    tg_masked_compose, tg_blend_latents (three storage modes): an odd size and a size past the grid cap each"""
    for dtype in (DTYPES if cid.startswith("dup_rows") else DTYPES[:1]):
        _, _, metrics = run_case(cid, dtype, quiet=True)
        assert _worst(metrics) <= 1.0
