"""The C-ABI contracts of the boundary convolutions and glue kernels (csrc/tg_elementwise.hip and ``tg_attn_probs`` of csrc/tg_attention.hip)
restated in fp64 from include/theatergen_hip.h, for checking single launches, kernel branch by kernel branch.

A launch is a plain dict: ``entry``, ``dtype`` (the storage type) and the C argument names; tensors stand for the pointers.  Operands are read the
way the kernels read raw pointers, ``gemm_contract.Region`` over the operand's storage along the pitches of the call; a launch that reads past a
storage makes ``Region.view`` raise.

    conv_in     out[(b, y, x), n] = bias[n] + sum_{ky, kx, c} sample[b, c, y + ky - 1, x + kx - 1] weight[n, ky, kx, c]   (zero outside the image)
                + the same rows at out + dup_offset (tg_conv_in_dup)
    conv_out    out[b, n, y, x]  = bias[n] + sum A'[b, y + ky - 1, x + kx - 1, c] weight[n, ky, kx, c],  A' = x (tg_conv_out) or
                round_T(act(x a[b, c] + d[b, c])) (tg_conv_out_gn, coef = [batch][2][cin]); the zero padding is applied AFTER the prologue
    transpose   dst[b, c, r] = src[b, r, c]                      dup_rows  dst[r, c] = src[r ld + c]
    softmax     out[r, :] = softmax(scale x[r, :])               probs     softmax_j(scale q_i . k_j)[tokens[t]], items b0 .. batch - 1
    timestep    f_i = exp(-ln(10000) i / (dim / 2 - freq_shift)); (sin | cos)(t f_i), flip: (cos | sin); t = t[*index + r t_stride]
    geglu       x[:, :inner] gelu(x[:, inner:])                  act  0 identity, 1 SiLU, 2 GELU (erf), 3 x sigmoid(1.702 x), else identity
    add, conv1x1, gaussian_sample, add_noise, shift, masked_compose, blend_latents: as the header states them

  * ``reference(a)`` -> (ref, mag): {output: fp64 tensor shaped like the written region} and the same sums over absolute values;
  * ``plan(a)``: the kernel the C gates choose, its LDS bytes and grid-stride trips; ``blocks(a)``: the block a workgroup / wave / thread owns;
  * ``read_extents(a)`` / ``written_region(a)``: ``Region`` lists;
  * ``element_bound(a, ref, mag)``: per-element bounds from operation counts (derived in the docstrings, not tuned on a kernel);
  * ``model(a, fault=None)``: fp32 CPU models of the kernels' algorithms with one switch per injected fault (``FAULTS``);
  * ``judge(a, outs)``: every assertion the GPU edge test makes on the outputs of one launch, as a list of failures;
  * ``make_case`` / ``all_cases``: the launches of tests/test_boundary_edges_gpu.py, drawn on the CPU from a seed.  Every element of an input
    buffer that the contract does not read holds NaN (pad columns, guard rows, rows of items below b0, unread table entries).
Operands are at least 2^-10 in magnitude or exactly 0, so subnormal flushing in the matrix and dot instructions is not what a bound measures.
"""
import math

import torch

from tests import launch_check as lc
from tests.backward_contract import compare
from tests.gemm_contract import Region

LOG2E = 1.4426950408889634
U32 = 2.0 ** -24                                                   # unit roundoff of fp32
GRID_CAP = 2048                                                    # tg_blocks_1d
CIN_MFMA_BLOCKS, CIN_FAST_BLOCKS, COUT_FAST_BLOCKS = 1024, 512, 1024
EXACT = ("transpose", "dup_rows", "shift")                         # bit equality (blend: its two half-precision modes)
SRC_DTYPES = {torch.bfloat16: 0, torch.float16: 1, torch.float32: 2}
FAULTS = ("pair_image_of_first", "k_last_chunk_dropped", "border_le", "bias_before_halves", "prologue_on_padding", "second_trip_skipped",
          "transpose_ragged_dropped", "softmax_max_unscaled", "probs_slot_ignored", "add_tail_dropped")


def tols(dtype):
    """1.5 x the per-launch bound of launch_check, as the backward and attention edge tests: rel-L2 4.5e-3 / 6e-4, max 1.5e-2 / 3.75e-3"""
    return 1.5 * lc.l2_tol(dtype), 1.5 * lc.rel_tol(dtype)


def unit_roundoff(dtype):
    return torch.finfo(dtype).eps / 2


def _f32(v):
    return float(torch.tensor(float(v), dtype=torch.float32))


def _up8(n):
    return (n + 7) // 8 * 8


def _al(t, n):
    return t.data_ptr() % n == 0


# ---- the gates of the C entries ------------------------------------------------------------------------------------------------------
def conv_in_fast_lds(cin, cout):
    G = cout // 8
    groups = 256 // G if G > 0 else 0
    return (9 * cin * cout + groups * 2 * 9 * cin) * 4, groups


def conv_out_mfma_lds(cin, cout):
    return (180 * cin + cout * 9 * cin) * 2 + 2 * cin * 4


def takes_dup(cin, cout):
    """tg_conv_in_takes_dup"""
    return cin == 4 and cout > 0 and cout % 160 == 0 and cout <= 640


def takes_coef(cin, h, w, cout):
    """tg_conv_out_takes_coef"""
    return cin % 64 == 0 and cin <= 320 and 0 < cout <= 8 and h % 8 == 0 and w % 16 == 0


def _trips(units, cap_units):
    return max(1, -(-units // cap_units))


def plan(a):
    """-> {"kernel", "lds" (dynamic LDS bytes or None), "trips" (grid-stride trips of the busiest workgroup), "block" (what owns an output block)}"""
    e = a["entry"]
    if e == "conv_in":
        cin, cout, npix = a["cin"], a["cout"], a["batch"] * a["h"] * a["w"]
        if takes_dup(cin, cout) and _al(a["out"], 16) and _al(a["weight"], 8):
            return dict(kernel="conv_in_mfma_kernel", lds=(cout * 56 + 4 * 32 * 168) * 2, trips=_trips(npix, CIN_MFMA_BLOCKS * 128),
                        block="32-pixel group x 160-channel half")
        lds, groups = conv_in_fast_lds(cin, cout)
        if cout % 8 == 0 and groups >= 1 and _al(a["out"], 16) and lds <= 65536:
            return dict(kernel="conv_in_fast_kernel", lds=lds, trips=_trips(npix, CIN_FAST_BLOCKS * 2 * groups), groups=groups,
                        block="pixel pair x 8 channels")
        return dict(kernel="conv_in_kernel", lds=4 * 9 * cin * 4, trips=1, block="pixel")
    if e == "conv_out":
        cin, cout, h, w = a["cin"], a["cout"], a["h"], a["w"]
        npix = a["batch"] * h * w
        al = _al(a["x"], 16) and _al(a["weight"], 16)
        if takes_coef(cin, h, w, cout) and al:
            return dict(kernel="conv_out_mfma_kernel", lds=conv_out_mfma_lds(cin, cout), trips=1, block="8 x 16 tile")
        if a.get("coef") is not None:
            return dict(kernel="refused", lds=None, trips=0, block="")
        lds = cout * 9 * cin * 2
        if lds <= 65536 and al:
            return dict(kernel=f"conv_out_fast_kernel<{4 if cout <= 4 else 8}>", lds=lds, trips=_trips((npix + 1) // 2, COUT_FAST_BLOCKS * 4),
                        block="pixel pair")
        return dict(kernel="conv_out_kernel", lds=0, trips=1, block="pixel")
    if e == "transpose":
        big = a["rows"] % 128 == 0 and a["cols"] % 64 == 0 and _al(a["src"], 16) and _al(a["dst"], 16)
        return dict(kernel="transpose_big_kernel" if big else "transpose_kernel", lds=None, trips=1, block="128 x 64 tile" if big else "32 x 32 tile")
    if e in ("softmax_rows", "attn_probs", "timestep"):
        k = {"softmax_rows": "softmax_rows_kernel", "attn_probs": "attn_probs_kernel", "timestep": "timestep_embedding_kernel"}[e]
        return dict(kernel=k, lds=None, trips=-(-(a["dim"] // 2) // 128) if e == "timestep" else 1, block="row")
    units, name = _units_1d(a)
    if e == "conv1x1":
        return dict(kernel=name, lds=None, trips=1, block="256 pixels")
    return dict(kernel=name, lds=None, trips=_trips(units, GRID_CAP * 256), block="grid-stride trip")


def _units_1d(a):
    """(work items of the 1-D grid-stride loop, kernel name); an item is 8 elements in geglu / add / dup_rows, else one element"""
    e = a["entry"]
    if e == "geglu":
        return a["rows"] * a["inner"] // 8, "geglu_kernel"
    if e == "act":
        return a["n"], "act_kernel"
    if e == "add":
        return a["n"] // 8, "add_kernel"
    if e == "dup_rows":
        return a["rows"] * a["cols"] // 8, "dup_rows_kernel"
    if e == "conv1x1":
        return a["batch"] * a["hw"], "conv1x1_nchw_kernel"
    if e == "gaussian":
        return a["batch"] * a["channels"] * a["hw"], "gaussian_sample_kernel"
    if e == "add_noise":
        return a["steps"] * a["n"], "add_noise_kernel"
    if e == "shift":
        return a["planes"] * a["h"] * a["w"], "shift_kernel"
    if e == "compose":
        return a["planes"] * a["hw"], "compose_kernel"
    assert e == "blend", e
    return a["planes"] * a["hw"], "blend_kernel<%d>" % {-1: 0, 1: 1, 0: 2}[a["storage_dtype"]]      # -1 fp32, TG_F16 = 1, TG_BF16 = 0


# ---- regions -------------------------------------------------------------------------------------------------------------------------
def _reg(name, t, sizes, strides=None, offset=0):
    sizes = tuple(int(s) for s in sizes)
    if strides is None:
        strides, n = [], 1
        for s in reversed(sizes):
            strides.insert(0, n)
            n *= s
    return Region(name, t, int(offset), sizes, tuple(int(s) for s in strides))


def _opt(regs):
    return [r for r in regs if r.t is not None]


def read_extents(a):
    e = a["entry"]
    if e == "conv_in":
        K = 9 * a["cin"]
        return _opt([_reg("sample", a["sample"], (a["batch"], a["cin"], a["h"], a["w"])), _reg("weight", a["weight"], (a["cout"], K)),
                     _reg("bias", a.get("bias"), (a["cout"],))])
    if e == "conv_out":
        K = 9 * a["cin"]
        return _opt([_reg("x", a["x"], (a["batch"], a["h"], a["w"], a["cin"])), _reg("weight", a["weight"], (a["cout"], K)),
                     _reg("bias", a.get("bias"), (a["cout"],)), _reg("coef", a.get("coef"), (a["batch"], 2, a["cin"]))])
    if e == "transpose":
        return [_reg("src", a["src"], (a["batch"], a["rows"], a["cols"]))]
    if e == "softmax_rows":
        return [_reg("x", a["x"], (a["rows"], a["cols"]), (a["ldx"], 1))]
    if e == "attn_probs":
        nb, H, hd = a["batch"] - a["b0"], a["heads"], a["head_dim"]
        regs = [_reg("q", a["q"], (nb, H, a["n_q"], hd), (a["q_bs"], hd, a["q_ld"], 1), a["b0"] * a["q_bs"]),
                _reg("k", a["k"], (nb, H, a["len"], hd), (a["k_bs"], hd, a["k_ld"], 1), a["b0"] * a["k_bs"])]
        return regs + ([_reg("tokens", a["tokens"], (a["n_tokens"],))] if a.get("tokens") is not None else [])
    if e == "timestep":
        regs = [_reg("t", a["t"], (a["rows"],), (a["t_stride"],), a.get("index_value", 0))]
        return regs + ([_reg("index", a["index"], (1,))] if a.get("index") is not None else [])
    if e == "geglu":
        return [_reg("x", a["x"], (a["rows"], 2 * a["inner"]))]
    if e == "act":
        return [_reg("x", a["x"], (a["n"],))]
    if e == "add":
        return [_reg("a", a["a"], (a["n"],)), _reg("b", a["b"], (a["n"],))]
    if e == "dup_rows":
        return [_reg("src", a["src"], (a["rows"], a["cols"]), (a["ld"], 1))]
    if e == "conv1x1":
        return _opt([_reg("x", a["x"], (a["batch"], a["cin"], a["hw"])), _reg("weight", a["weight"], (a["cout"], a["cin"])),
                     _reg("bias", a.get("bias"), (a["cout"],))])
    if e == "gaussian":
        B, Cc, hw = a["batch"], a["channels"], a["hw"]
        parts = 2 if a.get("noise") is not None else 1
        return _opt([_reg("moments", a["moments"], (B, parts * Cc, hw), (2 * Cc * hw, hw, 1)), _reg("noise", a.get("noise"), (B, Cc, hw))])
    if e == "add_noise":
        return [_reg("x0", a["x0"], (a["n"],)), _reg("noise", a["noise"], (a["n"],)), _reg("ca", a["ca"], (a["steps"],)), _reg("cb", a["cb"], (a["steps"],))]
    if e == "shift":
        return [_reg("src", a["src"], (a["planes"], a["h"], a["w"]))]
    if e == "compose":
        return [_reg("dst", a["dst"], (a["planes"], a["hw"])), _reg("src", a["src"], (a["planes"], a["hw"])), _reg("mask", a["mask"], (a["hw"],))]
    assert e == "blend", e
    return [_reg("bg", a["bg"], (a["planes"], a["hw"])), _reg("fg", a["fg"], (a["planes"], a["hw"])), _reg("mask", a["mask"], (a["hw"],))]


def written_region(a):
    e = a["entry"]
    if e == "conv_in":
        npix = a["batch"] * a["h"] * a["w"]
        regs = [_reg("out", a["out"], (npix, a["cout"]))]
        return regs + ([_reg("out_dup", a["out"], (npix, a["cout"]), None, a["dup_offset"])] if a.get("dup_offset") else [])
    if e == "conv_out":
        return [_reg("out", a["out"], (a["batch"], a["cout"], a["h"], a["w"]))]
    if e == "transpose":
        return [_reg("dst", a["dst"], (a["batch"], a["cols"], a["rows"]))]
    if e == "softmax_rows":
        return [_reg("out", a["out"], (a["rows"], a["cols"]), (a["ldo"], 1))]
    if e == "attn_probs":
        nt = a["n_tokens"] if a.get("tokens") is not None else a["len"]
        return [_reg("probs", a["probs"], (a["batch"] - a["b0"], a["heads"], a["n_q"], nt))]
    if e == "timestep":
        return [_reg("out", a["out"], (a["rows"], a["dim"]), (a["ldo"], 1))]
    if e == "geglu":
        return [_reg("out", a["out"], (a["rows"], a["inner"]))]
    if e in ("act", "add"):
        return [_reg("out", a["out"], (a["n"],))]
    if e == "dup_rows":
        return [_reg("dst", a["dst"], (a["rows"], a["cols"]))]
    if e == "conv1x1":
        return [_reg("out", a["out"], (a["batch"], a["cout"], a["hw"]))]
    if e == "gaussian":
        return [_reg("out", a["out"], (a["batch"], a["channels"], a["hw"]))]
    if e == "add_noise":
        return [_reg("out", a["out"], (a["steps"], a["n"]))]
    if e == "shift":
        return [_reg("dst", a["dst"], (a["planes"], a["h"], a["w"]))]
    if e == "compose":
        return [_reg("dst", a["dst"], (a["planes"], a["hw"]))]
    assert e == "blend", e
    return [_reg("out", a["out"], (a["planes"], a["hw"]))]


def in_place(a):
    """operands that ARE the output: tg_softmax_rows with out == x, tg_masked_compose's dst"""
    if a["entry"] == "compose":
        return ("dst",)
    if a["entry"] == "softmax_rows" and a["out"].data_ptr() == a["x"].data_ptr():
        return ("x",)
    return ()


def _ext(a, dt=torch.float64, cpu=False):
    out = {}
    for r in read_extents(a):
        v = r.view()
        v = v.cpu() if cpu else v
        out[r.name] = v.to(dt) if v.is_floating_point() else v
    return out


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def _taps(v, h, w):
    """v [B, h, w, C] -> [B, h, w, 9, C]: the 3 x 3 window of every pixel, zero outside the image, tap = 3 ky + kx"""
    p = torch.nn.functional.pad(v, (0, 0, 1, 1, 1, 1))
    return torch.stack([p[:, ky:ky + h, kx:kx + w] for ky in range(3) for kx in range(3)], dim=3)


def _gelu64(v):
    return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))


def _act64(v, act):
    if act == 1:
        return v * torch.sigmoid(v)
    if act == 2:
        return _gelu64(v)
    if act == 3:
        return v * torch.sigmoid(1.702 * v)
    return v


def gn_activations(a, ext=None):
    """fp64 [B, h, w, cin] operand of the convolution of a conv_out launch: x, or the conv_norm_out prologue rounded to the storage type"""
    ext = _ext(a) if ext is None else ext
    x = ext["x"]
    if a.get("coef") is None:
        return x
    co = ext["coef"]
    f = x * co[:, 0][:, None, None, :] + co[:, 1][:, None, None, :]
    f = _act64(f, 1) if a["a_silu"] else f
    return f.to(a["dtype"]).double()


def _softmax64(s):
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    return e / e.sum(-1, keepdim=True)


def blend_constants(a):
    """(s1, s2, sigma) as the entry forms them: fp32 roundings of the double square roots of the fp32 ``ratio``"""
    r = _f32(a["ratio"])
    return _f32(math.sqrt(1.0 - r)), _f32(math.sqrt(r)), _f32(a["sigma"])


def _blend_exact(a, ext32):
    """the kernel's comment, operation by operation in fp32 with a rounding to the storage type after each half-precision tensor op: bit-exact
    where every fp32 product with the mask is exact (mask values in {0, 1/4, 1/2, 3/4, 1}: a fused multiply-add then rounds like the plain sum)"""
    T = {1: torch.float16, 0: torch.bfloat16}[a["storage_dtype"]]

    def rs(v):
        return v.to(T).float()
    s1, s2, sg = blend_constants(a)
    bg, fg, m = ext32["bg"], ext32["fg"], ext32["mask"].reshape(1, -1)
    inner = rs(rs(bg * s1) + rs(fg * s2))
    return rs(rs(bg * (1.0 - m) + inner * m) * sg)


def reference(a):
    """-> (ref, mag): fp64 outputs and the same expression over absolute values (the scale an error of the arithmetic is measured against)"""
    e, ext = a["entry"], _ext(a)
    if e in ("conv_in", "conv_out"):
        B, h, w, cin, cout = a["batch"], a["h"], a["w"], a["cin"], a["cout"]
        v = ext["sample"].permute(0, 2, 3, 1) if e == "conv_in" else gn_activations(a, ext)
        P = _taps(v, h, w).reshape(B * h * w, 9 * cin)
        W = ext["weight"]
        bias = ext["bias"] if "bias" in ext else torch.zeros(cout, dtype=torch.float64, device=W.device)
        ref, mag = P @ W.t() + bias, P.abs() @ W.abs().t() + bias.abs()
        if e == "conv_out":
            ref, mag = (t.reshape(B, h, w, cout).permute(0, 3, 1, 2).contiguous() for t in (ref, mag))
            return {"out": ref}, {"out": mag}
        if a.get("dup_offset"):
            return {"out": ref, "out_dup": ref}, {"out": mag, "out_dup": mag}
        return {"out": ref}, {"out": mag}
    if e == "transpose":
        r = ext["src"].transpose(1, 2).contiguous()
        return {"dst": r}, {"dst": r.abs()}
    if e == "dup_rows":
        return {"dst": ext["src"].clone()}, {"dst": ext["src"].abs()}
    if e == "softmax_rows":
        r = _softmax64(_f32(a["scale"]) * ext["x"])
        return {"out": r}, {"out": r}
    if e == "attn_probs":
        s = _f32(a["scale"]) * torch.einsum("bhid,bhjd->bhij", ext["q"], ext["k"])
        r = _softmax64(s)
        if "tokens" in ext:
            r = r[..., ext["tokens"].long()]
        return {"probs": r}, {"probs": r}
    if e == "timestep":
        half = a["dim"] // 2
        f = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float64, device=ext["t"].device) / (half - _f32(a["freq_shift"])))
        ang = ext["t"][:, None] * f[None, :]
        s, c = torch.sin(ang), torch.cos(ang)
        r = torch.cat([c, s], 1) if a["flip"] else torch.cat([s, c], 1)
        return {"out": r}, {"out": r.abs()}
    if e == "geglu":
        i = a["inner"]
        r = ext["x"][:, :i] * _gelu64(ext["x"][:, i:])
        return {"out": r}, {"out": (ext["x"][:, :i] * ext["x"][:, i:]).abs()}
    if e == "act":
        return {"out": _act64(ext["x"], a["act"])}, {"out": ext["x"].abs()}
    if e == "add":
        return {"out": ext["a"] + ext["b"]}, {"out": ext["a"].abs() + ext["b"].abs()}
    if e == "conv1x1":
        xs = ext["x"] * _f32(a["in_scale"])
        bias = ext["bias"] if "bias" in ext else torch.zeros(a["cout"], dtype=torch.float64, device=xs.device)
        return ({"out": torch.einsum("oc,bcp->bop", ext["weight"], xs) + bias[None, :, None]},
                {"out": torch.einsum("oc,bcp->bop", ext["weight"].abs(), xs.abs()) + bias.abs()[None, :, None]})
    if e == "gaussian":
        Cc, sc = a["channels"], _f32(a["scale"])
        mean = ext["moments"][:, :Cc]
        if "noise" not in ext:
            return {"out": sc * mean}, {"out": abs(sc) * mean.abs()}
        z = torch.exp(0.5 * ext["moments"][:, Cc:].clamp(-30.0, 20.0)) * ext["noise"]
        return {"out": sc * (mean + z)}, {"out": abs(sc) * (mean.abs() + z.abs())}
    if e == "add_noise":
        p, q = ext["ca"][:, None] * ext["x0"][None, :], ext["cb"][:, None] * ext["noise"][None, :]
        return {"out": p + q}, {"out": p.abs() + q.abs()}
    if e == "shift":
        P, h, w, dx, dy = a["planes"], a["h"], a["w"], a["dx"], a["dy"]
        r = torch.zeros_like(ext["src"])
        ys = torch.arange(h, device=r.device)
        xs = torch.arange(w, device=r.device)
        sy, sx = ys - dy, xs - dx
        oky, okx = (sy >= 0) & (sy < h), (sx >= 0) & (sx < w)
        if bool(oky.any()) and bool(okx.any()):
            r[:, ys[oky][:, None], xs[okx][None, :]] = ext["src"][:, sy[oky][:, None], sx[okx][None, :]]
        return {"dst": r}, {"dst": r.abs()}
    if e == "compose":
        m = ext["mask"][None, :]
        p, q = ext["dst"] * (1.0 - m), ext["src"] * m
        return {"dst": p + q}, {"dst": p.abs() + q.abs()}
    assert e == "blend", e
    if a["storage_dtype"] >= 0:
        r = _blend_exact(a, _ext(a, torch.float32)).double()
        return {"out": r}, {"out": r.abs()}
    s1, s2, sg = blend_constants(a)
    m = ext["mask"][None, :]
    inner = ext["bg"] * s1 + ext["fg"] * s2
    return ({"out": (ext["bg"] * (1.0 - m) + inner * m) * sg},
            {"out": (ext["bg"].abs() * (1.0 - m) + (ext["bg"].abs() * s1 + ext["fg"].abs() * s2) * m) * abs(sg)})


# ---- ownership -----------------------------------------------------------------------------------------------------------------------
def blocks(a):
    """-> (ids, grid): int64 tensor shaped like the entry's (first) output with the index of the block that owns each element"""
    e, p = a["entry"], plan(a)
    w0 = written_region(a)[0]
    dev = w0.t.device

    def ar(n):
        return torch.arange(n, device=dev)
    if e == "conv_in":
        npix, cout = w0.sizes
        pix, ch = ar(npix)[:, None], ar(cout)[None, :]
        if p["kernel"] == "conv_in_mfma_kernel":
            nh = cout // 160
            return (pix // 32) * nh + ch // 160, ((npix + 31) // 32, nh)
        if p["kernel"] == "conv_in_fast_kernel":
            return (pix // 2) * (cout // 8) + ch // 8, ((npix + 1) // 2, cout // 8)
        return pix.expand(npix, cout).contiguous(), (npix,)
    if e == "conv_out":
        B, cout, h, w = w0.sizes
        b, y, x = ar(B)[:, None, None, None], ar(h)[None, None, :, None], ar(w)[None, None, None, :]
        if p["kernel"] == "conv_out_mfma_kernel":
            ids, grid = (b * (h // 8) + y // 8) * (w // 16) + x // 16, (B, h // 8, w // 16)
        else:
            pix = (b * h + y) * w + x
            ids, grid = (pix // 2, ((B * h * w + 1) // 2,)) if "fast" in p["kernel"] else (pix, (B * h * w,))
        return ids.expand(B, cout, h, w).contiguous(), grid
    if e == "transpose":
        B, cols, rows = w0.sizes
        tr, tc = (128, 64) if p["kernel"] == "transpose_big_kernel" else (32, 32)
        nr, nc = -(-rows // tr), -(-cols // tc)
        ids = (ar(B)[:, None, None] * nr + ar(rows)[None, None, :] // tr) * nc + ar(cols)[None, :, None] // tc
        return ids.contiguous(), (B, nr, nc)
    if e in ("softmax_rows", "timestep", "attn_probs"):
        sizes = w0.sizes
        nrow = int(math.prod(sizes[:-1]))
        return ar(nrow).reshape(*sizes[:-1], 1).expand(*sizes).contiguous(), (nrow,)
    n = int(math.prod(w0.sizes))
    per = 8 if e in ("geglu", "add", "dup_rows") else 1
    if e == "conv1x1":
        B, co, hw = w0.sizes
        pix = ar(B)[:, None, None] * hw + ar(hw)[None, None, :]
        return (pix // 256).expand(B, co, hw).contiguous(), (-(-B * hw // 256),)
    return (ar(n) // (GRID_CAP * 256 * per)).reshape(w0.sizes), (max(p["trips"], 1),)


# ---- per-element bounds --------------------------------------------------------------------------------------------------------------
def _rounding(ref, dtype, n=1):
    """n roundings of |ref| to ``dtype``: n x unit roundoff x |ref|, no smaller than n halves of the smallest subnormal step; 0 for fp32 out"""
    if dtype == torch.float32:
        return torch.zeros_like(ref)
    return n * torch.clamp(unit_roundoff(dtype) * ref.abs(), min=torch.finfo(dtype).smallest_normal * torch.finfo(dtype).eps / 2)


def softmax_count(adds_per_lane, n):
    """c of the softmax bound  u_out ref + c 2^-24 ref (1 + |scale (x - max)|), in units of the fp32 unit roundoff:
         the element's own exponential: 2 (one ulp of the hardware exp2) and, times |arg|, 3 (scale x log2(e) rounded twice, the fma once);
         the normalising sum: ``adds_per_lane`` sequential adds in a lane + 6 butterfly adds; its terms carry the same 2, and 3 times their
         |arg|, whose p-weighted mean is at most ln(n) (sum_j p_j (max - s_j) = H - ln Z' <= ln n);  the reciprocal 1 and the product with it 1.
       The error of the subtracted maximum is common to every term of a row and cancels in the ratio."""
    return 2 + 3 + adds_per_lane + 6 + 2 + 3 * math.log(max(n, 2)) + 2


def timestep_freq_eps():
    """worst relative error of the fp32 frequencies of ``oracle.unet.timestep_sinusoid`` (exp of the fp32 exponent) against fp64, over the
    dims and freq_shifts of the cases: measured on the CPU oracle, never on the kernel.  The bound allows 4 x this for the hardware's faster
    exponential (``TIMESTEP_EPS_FACTOR``)."""
    worst = 0.0
    for dim in (256, 320, 1280):
        for shift in (0.0, 1.0):
            half = dim // 2
            f32 = torch.exp(-math.log(10000) * torch.arange(0, half, dtype=torch.float32) / (half - shift)).double()
            f64 = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float64) / (half - shift))
            worst = max(worst, float(((f32 - f64) / f64).abs().max()))
    return worst


TIMESTEP_EPS_FACTOR = 4.0


def element_bound(a, ref, mag):
    """{output: fp64 bound on |got - ref| per element}, from operation counts:
      convs       u_out |ref| + (K + 2) 2^-24 (sum_k |x_k w_k| + |bias|): K fp32 accumulations (any order), the bias add and the final sum of
                  the wave / accumulator, each at most one fp32 rounding of a partial sum no larger than the sum of magnitudes; products of two
                  storage-type values are exact in fp32.  u_out = 0 for an fp32 output.  conv_in on the matrix cores with a sample wider than the
                  storage type: + u_T^2 sum_k |x_k w_k| (x = head + tail, each a storage-type value: what the tail drops is at most u_T^2 |x|);
      softmax     u_out ref + c 2^-24 ref (1 + |scale (x - max)|), c = ``softmax_count(cols / 64, cols)``;
      probs       the same with u_out = 0, c = ``softmax_count(4, len)``, and the scores' own error: a sequential fp32 dot product of head_dim terms,
                  d_j = (head_dim + 1) 2^-24 |scale| sum_d |q_d k_jd|, moves p_i by at most p_i (d_i + max_j d_j);
      timestep    u_T |ref| + |t| f_i eps + 2^-22: eps = 4 x ``timestep_freq_eps()``; 2^-22: two ulps of sinf / cosf at magnitude <= 1 and the rounding of t f_i
                  is inside eps;
      geglu       u_T |ref| + (1.5e-7 + 16 2^-24) |a g|: the documented absolute error of the erfc polynomial, and 16 fp32 ulps: rcp 1, exp2 2, the
                  rounding of z^2 in its argument (2 z^2 e^{-z^2} <= 1), five fma of the polynomial, three products, the select's 1 - e, the final a gelu(g);
      act         0: bit equality; 2: as geglu with a = 1; 1 and 3: u_T |ref| + 16 2^-24 (1 + |x|) |ref| (exp2 2 + its argument's rounding k |x| <= 2.5 |x|,
                  the add, rcp 1, the product);
      add         u_T |ref| + 2 2^-24 (|a| + |b|) (the fp32 sum is rounded before the storage rounding);
      conv1x1     (2 cin + 2) 2^-24 sum |w (s x)|;  gaussian 8 2^-24 |scale| (|mean| + |e^{lv / 2} noise|) (expf 2 ulps, three products, one add);
      add_noise, masked_compose 4 2^-24 of the sum of magnitudes;  blend fp32 mode 8 2^-24 of the same;
      transpose, dup_rows, shift, blend in the half-precision modes: 0 (bit equality)."""
    e, T = a["entry"], a["dtype"]
    out = {}
    for name, r in ref.items():
        m = mag[name]
        if e in ("conv_in", "conv_out"):
            K = 9 * a["cin"]
            odt = torch.float32 if (e == "conv_out" and a["out_f32"]) else T
            b = _rounding(r, odt) + (K + 2) * U32 * m
            if e == "conv_in" and plan(a)["kernel"] == "conv_in_mfma_kernel" and a["sample"].dtype != T:
                b = b + unit_roundoff(T) ** 2 * m
        elif e == "softmax_rows":
            sc = _f32(a["scale"])
            x = _ext(a)["x"]
            arg = torch.nan_to_num((sc * (x - x.max(-1, keepdim=True).values)).abs(), posinf=0.0)
            b = _rounding(r, T) + softmax_count(a["cols"] / 64.0, a["cols"]) * U32 * r * (1.0 + arg)
        elif e == "attn_probs":
            ext, sc = _ext(a), _f32(a["scale"])
            s = sc * torch.einsum("bhid,bhjd->bhij", ext["q"], ext["k"])
            d = (a["head_dim"] + 1) * U32 * abs(sc) * torch.einsum("bhid,bhjd->bhij", ext["q"].abs(), ext["k"].abs())
            arg, dm = (s - s.max(-1, keepdim=True).values).abs(), d.max(-1, keepdim=True).values
            if "tokens" in ext:
                arg, d = arg[..., ext["tokens"].long()], d[..., ext["tokens"].long()]
            b = r * (softmax_count(4, a["len"]) * U32 * (1.0 + arg) + d + dm)
        elif e == "timestep":
            half = a["dim"] // 2
            t = _ext(a)["t"].abs()
            f = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float64, device=t.device) / (half - _f32(a["freq_shift"])))
            ph = t[:, None] * f[None, :] * (TIMESTEP_EPS_FACTOR * timestep_freq_eps())
            b = _rounding(r, T) + torch.cat([ph, ph], 1) + 2.0 ** -22
        elif e == "geglu" or (e == "act" and a["act"] == 2):
            b = _rounding(r, T) + (1.5e-7 + 16 * U32) * m
        elif e == "act":
            b = _rounding(r, T) + 16 * U32 * (1.0 + m) * r.abs() if a["act"] in (1, 3) else torch.zeros_like(r)
        elif e == "add":
            b = _rounding(r, T) + 2 * U32 * m
        elif e == "conv1x1":
            b = (2 * a["cin"] + 2) * U32 * m
        elif e == "gaussian":
            b = 8 * U32 * m
        elif e in ("add_noise", "compose"):
            b = 4 * U32 * m
        elif e == "blend" and a["storage_dtype"] < 0:
            b = 8 * U32 * m
        else:
            b = torch.zeros_like(r)
        out[name] = b
    return out


# ---- fp32 models of the kernels ------------------------------------------------------------------------------------------------------
def _gather(flat, idx, ok):
    """flat[idx] where ok else 0; an index outside the buffer (the ``border_le`` fault) reads 0.25"""
    inside = (idx >= 0) & (idx < flat.numel())
    v = torch.where(inside, flat[idx.clamp(0, flat.numel() - 1)], torch.full((), 0.25, dtype=flat.dtype))
    return torch.where(ok, v, torch.zeros((), dtype=flat.dtype))


def _patches(flat, nchw, B, C, h, w, b, y, x, fault):
    """fp32 [npix, 9, C]: the window of pixel (b, y, x) (index tensors [npix]) read from the flat operand the way the kernels index it"""
    c = torch.arange(C)[None, :]
    out = []
    for tap in range(9):
        yy, xx = (y + tap // 3 - 1)[:, None], (x + tap % 3 - 1)[:, None]
        ok = (yy >= 0) & (xx >= 0) & ((yy <= h) & (xx <= w) if fault == "border_le" else (yy < h) & (xx < w))
        idx = ((b[:, None] * C + c) * h + yy) * w + xx if nchw else ((b[:, None] * h + yy) * w + xx) * C + c
        out.append(_gather(flat, idx, ok.expand(-1, C)))
    return torch.stack(out, 1)


def _pix(B, h, w, fault, paired):
    """(b, y, x) of every pixel; ``pair_image_of_first``: the odd pixel of a pair takes the image index of the even one"""
    pix = torch.arange(B * h * w)
    b, r = pix // (h * w), pix % (h * w)
    if paired and fault == "pair_image_of_first":
        b = (pix // 2 * 2) // (h * w)
    return b, r // w, r % w


def _model_conv_in(a, fault):
    B, cin, h, w, cout, T = a["batch"], a["cin"], a["h"], a["w"], a["cout"], a["dtype"]
    ext = _ext(a, torch.float32, cpu=True)
    p, K, npix = plan(a), 9 * cin, B * h * w
    W = ext["weight"]
    bias = ext["bias"] if "bias" in ext else torch.zeros(cout)
    b, y, x = _pix(B, h, w, fault, p["kernel"] == "conv_in_fast_kernel")
    P = _patches(ext["sample"].reshape(-1), True, B, cin, h, w, b, y, x, fault).reshape(npix, K)
    if p["kernel"] == "conv_in_mfma_kernel":
        hi = P.to(T).float()
        lo = (P - hi).to(T).float()
        hi, lo, Wp = (torch.nn.functional.pad(t, (0, 48 - K)) for t in (hi, lo, W))           # k = 36 .. 47: the zero padding of the weight rows
        acc = torch.zeros(npix, cout)
        for ks in range(3):                                                 # three k-steps of 16: the tails first, then the heads
            if fault == "k_last_chunk_dropped" and ks == 2:
                continue
            sl = slice(16 * ks, 16 * ks + 16)
            acc = acc + lo[:, sl] @ Wp[:, sl].t()
            acc = acc + hi[:, sl] @ Wp[:, sl].t()
        bb = bias[:160].repeat(cout // 160) if fault == "bias_before_halves" else bias
        out = (acc + bb).to(T)
        done = CIN_MFMA_BLOCKS * 128
    elif p["kernel"] == "conv_in_fast_kernel":
        acc = bias[None, :].expand(npix, cout).clone()
        for k in range(K - (8 if fault == "k_last_chunk_dropped" else 0)):      # one fma per k, bias as the accumulator's first value
            acc = acc + P[:, k:k + 1] * W[None, :, k]
        out = acc.to(T)
        done = CIN_FAST_BLOCKS * 2 * p["groups"]
    else:
        acc = bias[None, :].expand(npix, cout).clone()
        for k in range(K):
            acc = acc + P[:, k:k + 1] * W[None, :, k]
        out = acc.to(T)
        done = npix
    if fault == "second_trip_skipped":
        out[done:] = float("nan")
    res = {"out": out}
    if a.get("dup_offset"):
        res["out_dup"] = out.clone()
    return res


def _lane_sum(prod):
    """prod fp32 [..., nchunk, 8] -> [...]: chunk i belongs to lane i % 64 (a lane adds its chunks in order), then the wave sum"""
    nch = prod.shape[-2]
    pad = (-nch) % 64
    v = torch.nn.functional.pad(prod.sum(-1), (0, pad)).reshape(*prod.shape[:-2], (nch + pad) // 64, 64)
    return v.sum(-2).sum(-1)


def _model_conv_out(a, fault):
    B, cin, h, w, cout, T = a["batch"], a["cin"], a["h"], a["w"], a["cout"], a["dtype"]
    ext = _ext(a, torch.float32, cpu=True)
    p, K, npix = plan(a), 9 * cin, B * h * w
    W = ext["weight"]
    bias = ext["bias"] if "bias" in ext else torch.zeros(cout)
    paired = "fast" in p["kernel"]
    b, y, x = _pix(B, h, w, fault, paired)
    act = ext["x"]
    pad_value = None
    if a.get("coef") is not None:
        ca, cd = ext["coef"][:, 0][:, None, None, :], ext["coef"][:, 1][:, None, None, :]
        f = act * ca + cd
        act = (f * torch.sigmoid(f) if a["a_silu"] else f).to(T).float()
        if fault == "prologue_on_padding":
            f0 = ext["coef"][:, 1]
            pad_value = (f0 * torch.sigmoid(f0) if a["a_silu"] else f0).to(T).float()          # act(0 a + d) [B, cin]
    P = _patches(act.reshape(-1), False, B, cin, h, w, b, y, x, fault)                         # [npix, 9, cin]
    if pad_value is not None:
        inside = _patches(torch.ones(B * h * w * cin), False, B, cin, h, w, b, y, x, None)
        P = torch.where(inside > 0, P, pad_value[b][:, None, :].expand(-1, 9, -1))
    P = P.reshape(npix, K)
    if p["kernel"] == "conv_out_mfma_kernel":
        acc = torch.zeros(npix, cout)
        for tap in range(9):                                                                    # tap-major, cin / 16 k-steps inside
            sl = slice(tap * cin, (tap + 1) * cin - (8 if fault == "k_last_chunk_dropped" and tap == 8 else 0))
            acc = acc + P[:, sl] @ W[:, sl].t()
        s = acc
    else:
        nch = K // 8 - (1 if fault == "k_last_chunk_dropped" else 0)
        s = torch.stack([_lane_sum((P * W[n][None, :]).reshape(npix, K // 8, 8)[:, :nch]) for n in range(cout)], 1)
    s = s + bias[None, :]
    if fault == "second_trip_skipped" and paired:
        s[COUT_FAST_BLOCKS * 4 * 2:] = float("nan")
    out = s.reshape(B, h, w, cout).permute(0, 3, 1, 2).contiguous()
    return {"out": out if a["out_f32"] else out.to(T)}


def _model_transpose(a, fault):
    src = _ext(a, a["dtype"], cpu=True)["src"]
    out = src.transpose(1, 2).contiguous()
    if fault == "transpose_ragged_dropped" and plan(a)["kernel"] == "transpose_kernel":
        r, c = a["rows"] // 32 * 32, a["cols"] // 32 * 32
        out[:, c:, :] = float("nan")
        out[:, :, r:] = float("nan")
    return {"dst": out}


def _model_softmax(a, fault):
    x = _ext(a, torch.float32, cpu=True)["x"]
    sc = torch.tensor(_f32(a["scale"]), dtype=torch.float32)
    L = torch.tensor(LOG2E, dtype=torch.float32)
    mx = x.max(-1, keepdim=True).values
    mx = mx if fault == "softmax_max_unscaled" else mx * sc
    e = torch.exp2(x * (sc * L) - mx * L)
    return {"out": (e * (1.0 / e.sum(-1, keepdim=True))).to(a["dtype"])}


def _model_probs(a, fault):
    ext = _ext(a, torch.float32, cpu=True)
    s = torch.einsum("bhid,bhjd->bhij", ext["q"], ext["k"]) * _f32(a["scale"])
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    pr = e * (1.0 / e.sum(-1, keepdim=True))
    if "tokens" in ext:
        tok = ext["tokens"].long()
        pr = pr[..., tok % 64 if fault == "probs_slot_ignored" else tok]
    return {"probs": pr}


def _model_timestep(a, fault):
    half = a["dim"] // 2
    t = _ext(a, torch.float32, cpu=True)["t"]
    f = torch.exp(torch.tensor(-9.210340371976184, dtype=torch.float32) * torch.arange(half, dtype=torch.float32)
                  / (torch.tensor(float(half), dtype=torch.float32) - _f32(a["freq_shift"])))
    ang = t[:, None] * f[None, :]
    s, c = torch.sin(ang), torch.cos(ang)
    return {"out": (torch.cat([c, s], 1) if a["flip"] else torch.cat([s, c], 1)).to(a["dtype"])}


def _gelu32(x):
    """gelu_erf_f of tg_common.h: erfc(|z|) by Abramowitz-Stegun 7.1.26"""
    z = x.abs() * 0.70710678118654752440
    t = 1.0 / (0.3275911 * z + 1.0)
    poly = 1.061405429 * t - 1.453152027
    for cf in (1.421413741, -0.284496736, 0.254829592):
        poly = poly * t + cf
    he = 0.5 * poly * t * torch.exp2(-LOG2E * z * z)
    return x * torch.where(x >= 0, 1.0 - he, he)


def _act32(x, act):
    if act == 1:
        return x * (1.0 / (1.0 + torch.exp2(-LOG2E * x)))
    if act == 2:
        return _gelu32(x)
    if act == 3:
        return x * (1.0 / (1.0 + torch.exp2(-1.702 * LOG2E * x)))
    return x


def _skip_trip(flat, a, fault, per):
    if fault == "second_trip_skipped":
        flat[GRID_CAP * 256 * per:] = float("nan")
    return flat


def _model_1d(a, fault):
    e, T = a["entry"], a["dtype"]
    ext = _ext(a, torch.float32, cpu=True)
    if e == "geglu":
        i = a["inner"]
        v = (ext["x"][:, :i] * _gelu32(ext["x"][:, i:])).to(T)
        return {"out": _skip_trip(v.reshape(-1), a, fault, 8).reshape(v.shape)}
    if e == "act":
        return {"out": _skip_trip(_act32(ext["x"], a["act"]).to(T), a, fault, 1)}
    if e == "add":
        v = _skip_trip((ext["a"] + ext["b"]).to(T), a, fault, 8)
        if fault == "add_tail_dropped":
            v[a["n"] // 8 * 8:] = float("nan")
        return {"out": v}
    if e == "dup_rows":
        v = _ext(a, T, cpu=True)["src"].clone()
        return {"dst": _skip_trip(v.reshape(-1), a, fault, 8).reshape(v.shape)}
    if e == "conv1x1":
        xs = ext["x"] * _f32(a["in_scale"])
        bias = ext["bias"] if "bias" in ext else torch.zeros(a["cout"])
        acc = bias[None, :, None].expand(a["batch"], a["cout"], a["hw"]).clone()
        for c in range(a["cin"]):
            acc = acc + ext["weight"][None, :, c, None] * xs[:, None, c, :]
        return {"out": acc}
    if e == "gaussian":
        Cc, sc = a["channels"], _f32(a["scale"])
        v = ext["moments"][:, :Cc]
        if "noise" in ext:
            v = v + torch.exp(0.5 * ext["moments"][:, Cc:].clamp(-30.0, 20.0)) * ext["noise"]
        v = sc * v
        return {"out": _skip_trip(v.reshape(-1).clone(), a, fault, 1).reshape(v.shape)}
    if e == "add_noise":
        v = ext["ca"][:, None] * ext["x0"][None, :] + ext["cb"][:, None] * ext["noise"][None, :]
        return {"out": _skip_trip(v.reshape(-1), a, fault, 1).reshape(v.shape)}
    if e == "shift":
        v = reference(dict(a, src=a["src"].cpu()))[0]["dst"].float()
        return {"dst": _skip_trip(v.reshape(-1), a, fault, 1).reshape(v.shape)}
    if e == "compose":
        m = ext["mask"][None, :]
        v = ext["dst"] * (1.0 - m) + ext["src"] * m
        return {"dst": _skip_trip(v.reshape(-1), a, fault, 1).reshape(v.shape)}
    assert e == "blend", e
    if a["storage_dtype"] >= 0:
        v = _blend_exact(a, ext)
    else:
        s1, s2, sg = blend_constants(a)
        m = ext["mask"][None, :]
        v = (ext["bg"] * (1.0 - m) + (ext["bg"] * s1 + ext["fg"] * s2) * m) * sg
    return {"out": _skip_trip(v.reshape(-1).clone(), a, fault, 1).reshape(v.shape)}


def model(a, fault=None):
    """{output name: tensor shaped like the written region, in the output's type}: the fp32 model of the kernel this launch runs"""
    assert fault is None or fault in FAULTS, fault
    fn = {"conv_in": _model_conv_in, "conv_out": _model_conv_out, "transpose": _model_transpose, "softmax_rows": _model_softmax,
          "attn_probs": _model_probs, "timestep": _model_timestep}.get(a["entry"], _model_1d)
    return fn(a, fault)


# ---- the verdict on one launch -------------------------------------------------------------------------------------------------------
def exact(a):
    return a["entry"] in EXACT or (a["entry"] == "blend" and a["storage_dtype"] >= 0) or (a["entry"] == "act" and a["act"] not in (1, 2, 3))


def judge(a, outs, ref=None, mag=None, bound=None):
    """every assertion on the outputs of one launch -> (failures, {output: metrics}).  ``outs``: {name: tensor shaped like the written region}
      * entries whose contract is exact: bit equality with the restatement;
      * the others: whole tensor and every block against the fp64 restatement at ``tols``, finite, and every element within ``element_bound``;
      * tg_conv_in_dup: both destinations bit-equal."""
    if ref is None:
        ref, mag = reference(a)
    l2, mx = tols(a["dtype"])
    ids, grid = blocks(a)
    bound = element_bound(a, ref, mag) if bound is None else bound        # an in-place launch: formed before it, from the inputs
    fails, metrics = [], {}
    for name, r in ref.items():
        got = outs[name]
        r = r.to(got.device)
        if exact(a):
            same = bool((got.double() == r).all())
            metrics[name] = {"rel_l2": 0.0 if same else float("inf"), "max_rel": 0.0 if same else float("inf"), "block_rel_l2": 0.0, "block_at": [],
                             "block_max_rel": 0.0, "finite": bool(torch.isfinite(got).all()), "worst_over_element_bound": 0.0 if same else float("inf")}
            if not same:
                bad = (got.double() != r) | torch.isnan(got)
                fails.append(f"{name}: {int(bad.sum())} elements differ from the restatement (bit equality), first at "
                             f"{[int(i) for i in torch.unravel_index(torch.argmax(bad.reshape(-1).int()), tuple(bad.shape))]}")
            continue
        ok, m = compare(got, r, ids.to(got.device), grid, l2, mx, mag[name].to(got.device) if a["entry"] in ("conv_in", "conv_out") else None)
        m["l2_tol"], m["max_tol"] = l2, mx
        if not ok:
            fails.append(f"{name}: {m}")
        err = (got.double() - r).abs()
        bd = bound[name].to(got.device)
        over = torch.where(err <= bd, err / bd.clamp_min(1e-300), torch.full_like(err, float("inf")))
        over = torch.where(err == 0, torch.zeros_like(err), over)
        m["worst_over_element_bound"] = float(over.max())
        if not bool((over <= 1.0).all()):
            bad = torch.nan_to_num(err / bd.clamp_min(1e-300), nan=float("inf"))
            at = [int(i) for i in torch.unravel_index(torch.argmax(bad), tuple(bad.shape))]
            fails.append(f"{name}: element {at} is {float(bad.max()):.3f} x its bound ({int((bad > 1).sum())} elements over)")
        metrics[name] = m
    if "out_dup" in outs and not torch.equal(outs["out"], outs["out_dup"]):
        fails.append("out_dup: the second destination differs from the first")
    return fails, metrics


# ---- test operands -------------------------------------------------------------------------------------------------------------------
def _guarded(values, row, device, shift=0, fill=float("nan")):
    """``values`` inside a buffer of its own with one guard row (``row`` elements, rounded up to 8 so that 16-byte alignment is kept) of ``fill`` in
    front of and behind it; ``shift``: that many more elements in front (a misaligned pointer)"""
    g = _up8(max(int(row), 8))
    buf = torch.full((g + shift + values.numel() + g,), fill if values.is_floating_point() else 0, dtype=values.dtype)
    buf[g + shift:g + shift + values.numel()] = values.reshape(-1)
    buf = buf.to(device)
    return buf[g + shift:g + shift + values.numel()].view(values.shape)


def _out(shape, dtype, row, device, shift=0):
    return _guarded(torch.full(tuple(shape), float("nan"), dtype=dtype), row, device, shift=shift)


def _clamp(v):
    """at least 2^-10 in magnitude, or exactly 0"""
    return torch.where(v.abs() < 2.0 ** -10, torch.zeros_like(v), v)


def other_half(dtype):
    return torch.float16 if dtype == torch.bfloat16 else torch.bfloat16


def _mant(dtype):
    return {torch.bfloat16: 7, torch.float16: 10}[dtype]


def _near_tie(f, dtype, slack):
    """fp64 values whose rounding to ``dtype`` an absolute perturbation of ``slack`` could change"""
    t = f.to(dtype).double()
    ulp = torch.exp2(torch.floor(torch.log2(t.abs().clamp_min(1e-30))) - _mant(dtype))
    return (0.5 * ulp - (f - t).abs()) <= slack


def make_case(entry, dtype, *, device="cpu", seed=0, **k):
    """one launch with operands drawn on the CPU from ``seed`` (the same bits on every device); every tensor sits in a storage of its own between
    two guard rows; input guards and pads hold NaN, outputs come back NaN-filled.  Keywords per entry: see ``all_cases``."""
    g = torch.Generator().manual_seed(104729 * seed + sum(ord(ch) for ch in entry))
    T = dtype

    def rn(*shape):
        return torch.randn(shape, generator=g)

    def st(v, dt=None):
        return _clamp(v.to(dt or T).float()).to(dt or T)
    if entry == "conv_in":
        B, h, w, cin, cout = k["B"], k["h"], k["w"], k["cin"], k["cout"]
        sdt = {"f32": torch.float32, "storage": T, "other": other_half(T)}[k.get("sample", "f32")]
        K, npix = 9 * cin, B * h * w
        dup = _up8(npix * cout) + 64 if k.get("dup") else 0
        out = _out((npix * cout + dup,), T, cout, device, shift=int(k.get("out_shift", 0)))
        return dict(entry=entry, dtype=T, batch=B, cin=cin, h=h, w=w, cout=cout, src_dtype=SRC_DTYPES[sdt], dup_offset=dup,
                    sample=_guarded(st(rn(B, cin, h, w), sdt), w, device), weight=_guarded(st(rn(cout, K) / math.sqrt(K)), K, device),
                    bias=_guarded(st(rn(cout)), cout, device) if k.get("bias", True) else None, out=out)
    if entry == "conv_out":
        B, h, w, cin, cout = k["B"], k["h"], k["w"], k["cin"], k["cout"]
        K, f32o = 9 * cin, int(k.get("out_f32", 1))
        x = st(rn(B, h, w, cin))
        a = dict(entry=entry, dtype=T, batch=B, cin=cin, h=h, w=w, cout=cout, out_f32=f32o, coef=None, a_silu=0,
                 weight=_guarded(st(rn(cout, K) / math.sqrt(K)), K, device), bias=_guarded(st(rn(cout)), cout, device),
                 out=_out((B, cout, h, w), torch.float32 if f32o else T, w, device))
        if k.get("coef"):
            # coefficients of a GroupNorm (gain near 1, offsets near 0); activations whose rounding to the storage type an fp32 evaluation of the
            # prologue (2^-19 of the terms' magnitudes) could move across a tie are redrawn, so that the kernel's activations are the restatement's
            a["a_silu"] = int(k.get("a_silu", 1))
            co = torch.stack([1.0 + 0.2 * rn(B, cin), 0.3 * rn(B, cin)], 1)
            xd = x.double()
            for _ in range(16):
                ca, cd = co[:, 0].double()[:, None, None, :], co[:, 1].double()[:, None, None, :]
                f = xd * ca + cd
                fa = _act64(f, 1) if a["a_silu"] else f
                bad = _near_tie(fa, T, 2.0 ** -19 * ((xd * ca).abs() + cd.abs() + fa.abs()))
                if not bool(bad.any()):
                    break
                xd = torch.where(bad, st(rn(B, h, w, cin)).double(), xd)
            assert not bool(bad.any())
            x = xd.to(T)
            a["coef"] = _guarded(co, cin, device)
        a["x"] = _guarded(x, cin, device)
        return a
    if entry == "transpose":
        B, rows, cols = k["B"], k["rows"], k["cols"]
        return dict(entry=entry, dtype=T, batch=B, rows=rows, cols=cols, src=_guarded(st(rn(B, rows, cols)), cols, device, shift=int(k.get("src_shift", 0))),
                    dst=_out((B, cols, rows), T, rows, device))
    if entry == "dup_rows":
        rows, cols, ld = k["rows"], k["cols"], k["ld"]
        full = torch.full((rows, ld), float("nan"), dtype=T)
        full[:, :cols] = st(rn(rows, cols))
        return dict(entry=entry, dtype=T, rows=rows, cols=cols, ld=ld, src=_guarded(full, ld, device), dst=_out((rows, cols), T, cols, device))
    if entry == "softmax_rows":
        rows, cols, ld = k["rows"], k["cols"], k["ld"]
        x = 30.0 * rn(rows, cols)
        for r in range(rows):                                  # random, equal values, some -inf, near +60000, near -60000
            kind = r % 5
            if kind == 1:
                x[r] = 3.25
            elif kind == 2:
                x[r, torch.randperm(cols, generator=g)[:max(cols // 3, 1)]] = float("-inf")
            elif kind in (3, 4):
                x[r] = (60000.0 - 32.0 * torch.randint(0, 16, (cols,), generator=g)) * (1.0 if kind == 3 else -1.0)
        full = torch.full((rows, ld), float("nan"), dtype=T)
        full[:, :cols] = x.to(T)
        xin = _guarded(full, ld, device)
        return dict(entry=entry, dtype=T, rows=rows, cols=cols, ldx=ld, ldo=ld, scale=0.044, x=xin,
                    out=xin if k.get("inplace") else _out((rows, ld), T, ld, device))
    if entry == "attn_probs":
        L, hd, nq, b0, H, batch = k["len"], k["head_dim"], k["n_q"], k["b0"], 2, 2
        pad = 8 if k.get("pitched") else 0
        q_ld, k_ld = H * hd + pad, H * hd + 2 * pad
        q_bs, k_bs = nq * q_ld + 2 * pad, L * k_ld + 3 * pad
        q = torch.full((batch, q_bs), float("nan"), dtype=T)
        kk = torch.full((batch, k_bs), float("nan"), dtype=T)
        for b in range(b0, batch):
            q[b, :nq * q_ld].reshape(nq, q_ld)[:, :H * hd] = st(rn(nq, H * hd))
            kk[b, :L * k_ld].reshape(L, k_ld)[:, :H * hd] = st(rn(L, H * hd))
        tok = None
        if k.get("tokens"):
            tl = [t for t in (0, 1, 63, 64, 200, L - 1) if t < L]
            tok = _guarded(torch.tensor(tl + tl[:2], dtype=torch.int32), 8, device)
        nt = int(tok.numel()) if tok is not None else L
        return dict(entry=entry, dtype=T, batch=batch, b0=b0, heads=H, head_dim=hd, n_q=nq, len=L, q_ld=q_ld, q_bs=q_bs, k_ld=k_ld, k_bs=k_bs,
                    scale=hd ** -0.5, q=_guarded(q, q_ld, device), k=_guarded(kk, k_ld, device), tokens=tok, n_tokens=nt if tok is not None else 0,
                    probs=_out((batch - b0, H, nq, nt), torch.float32, nt, device))
    if entry == "timestep":
        dim, rows, ts = k["dim"], k["rows"], k["t_stride"]
        ldo = dim + int(k.get("pad", 0))
        tv = torch.tensor([0.0, 1.0, 500.0, 981.0, 999.0])[:rows]
        idx = int(k["index"]) if k.get("index") is not None else 0
        n = 50 if k.get("index") is not None else max(1 + (rows - 1) * ts, 1)
        table = torch.full((n,), float("nan"))
        for r in range(rows):
            table[idx + r * ts] = tv[r] if ts else tv[min(2, rows - 1)]
        return dict(entry=entry, dtype=T, rows=rows, dim=dim, flip=int(k["flip"]), freq_shift=float(k["shift"]), t_stride=ts, ldo=ldo, index_value=idx,
                    t=_guarded(table, 8, device), index=_guarded(torch.tensor([idx], dtype=torch.int32), 8, device) if k.get("index") is not None else None,
                    out=_out((rows, ldo), T, ldo, device))
    if entry == "geglu":
        rows, inner = k["rows"], k["inner"]
        x = 2.0 * rn(rows, 2 * inner)
        return dict(entry=entry, dtype=T, rows=rows, inner=inner, x=_guarded(st(x), 2 * inner, device), out=_out((rows, inner), T, inner, device))
    if entry == "act":
        n = k["n"]
        return dict(entry=entry, dtype=T, n=n, act=int(k["act"]), x=_guarded(st(3.0 * rn(n)), 8, device), out=_out((n,), T, 8, device))
    if entry == "add":
        n = k["n"]
        return dict(entry=entry, dtype=T, n=n, a=_guarded(st(rn(n)), 8, device), b=_guarded(st(rn(n)), 8, device), out=_out((n,), T, 8, device))
    F = torch.float32

    def f32(v):
        return _clamp(v.float())
    if entry == "conv1x1":
        B, cin, cout, hw = k["B"], k["cin"], k["cout"], k["hw"]
        return dict(entry=entry, dtype=F, batch=B, cin=cin, cout=cout, hw=hw, in_scale=1.0 / 0.18215, x=_guarded(f32(rn(B, cin, hw)), hw, device),
                    weight=_guarded(f32(rn(cout, cin)), cin, device), bias=_guarded(f32(rn(cout)), cout, device), out=_out((B, cout, hw), F, hw, device))
    if entry == "gaussian":
        B, Cc, hw = k["B"], k["C"], k["hw"]
        mo = f32(rn(B, 2 * Cc, hw))
        mo[:, Cc:] = f32(4.0 * rn(B, Cc, hw))
        mo[0, Cc, 0], mo[0, Cc, 1] = -40.0, 30.0                                  # the clamp of logvar, both sides
        if not k.get("noise", True):
            mo[:, Cc:] = float("nan")                                             # noise NULL: the mode, logvar is not read
        return dict(entry=entry, dtype=F, batch=B, channels=Cc, hw=hw, scale=0.18215, moments=_guarded(mo, hw, device),
                    noise=_guarded(f32(rn(B, Cc, hw)), hw, device) if k.get("noise", True) else None, out=_out((B, Cc, hw), F, hw, device))
    if entry == "add_noise":
        steps, n = k["steps"], k["n"]
        ab = torch.rand(steps, generator=g) * 0.98 + 0.01
        return dict(entry=entry, dtype=F, steps=steps, n=n, x0=_guarded(f32(rn(n)), 8, device), noise=_guarded(f32(rn(n)), 8, device),
                    ca=_guarded(ab.sqrt(), 8, device), cb=_guarded((1 - ab).sqrt(), 8, device), out=_out((steps, n), F, n, device))
    if entry == "shift":
        P, h, w = k["planes"], k["h"], k["w"]
        return dict(entry=entry, dtype=F, planes=P, h=h, w=w, dx=int(k["dx"]), dy=int(k["dy"]), src=_guarded(f32(rn(P, h, w)), w, device),
                    dst=_out((P, h, w), F, w, device))
    if entry == "compose":
        P, hw = k["planes"], k["hw"]
        return dict(entry=entry, dtype=F, planes=P, hw=hw, dst=_guarded(f32(rn(P, hw)), hw, device), src=_guarded(f32(rn(P, hw)), hw, device),
                    mask=_guarded(_clamp(torch.rand(hw, generator=g)), hw, device))
    assert entry == "blend", entry
    P, hw, mode = k["planes"], k["hw"], int(k["mode"])
    H = {1: torch.float16, 0: torch.bfloat16}.get(mode)

    def lat(v):
        return f32(v) if H is None else _clamp(v.to(H).float())
    mask = torch.randint(0, 5, (hw,), generator=g).float() / 4.0
    return dict(entry=entry, dtype=F, planes=P, hw=hw, ratio=0.3, sigma=14.6146, storage_dtype=mode, bg=_guarded(lat(rn(P, hw)), hw, device),
                fg=_guarded(lat(rn(P, hw)), hw, device), mask=_guarded(mask, hw, device), out=_out((P, hw), F, hw, device))


# ---- the launches of tests/test_boundary_edges_gpu.py ----------------------------------------------------------------------------------
def _ci(B, h, w, cin, cout, **k):
    return ("conv_in", dict(B=B, h=h, w=w, cin=cin, cout=cout, **k))


def _co(B, h, w, cin, cout, **k):
    return ("conv_out", dict(B=B, h=h, w=w, cin=cin, cout=cout, **k))


# id -> ((entry, keywords), the kernel the C gates choose, dynamic LDS bytes): the by-hand table test_boundary_contract_cpu.py holds ``plan`` to
CONV_IN_CASES = {
    "3x5x7x4x320": (_ci(3, 5, 7, 4, 320), "conv_in_mfma_kernel", 78848),
    "1x1x1x4x160": (_ci(1, 1, 1, 4, 160, sample="storage"), "conv_in_mfma_kernel", 60928),
    "2x1x40x4x480": (_ci(2, 1, 40, 4, 480, sample="other"), "conv_in_mfma_kernel", 96768),                 # three channel halves
    "1x9x1x4x640": (_ci(1, 9, 1, 4, 640), "conv_in_mfma_kernel", 114688),
    "2x260x260x4x160-trip2": (_ci(2, 260, 260, 4, 160, sample="storage"), "conv_in_mfma_kernel", 60928),    # 135 200 pixels > 1024 x 128
    "2x8x8x4x320-dup": (_ci(2, 8, 8, 4, 320, dup=True), "conv_in_mfma_kernel", 78848),
    "3x5x7x4x320-outshift4": (_ci(3, 5, 7, 4, 320, out_shift=4), "conv_in_kernel", 576),                   # out not 16-byte aligned
    "3x5x7x3x16": (_ci(3, 5, 7, 3, 16), "conv_in_fast_kernel", 29376),                                     # ControlNet conditioning, K = 27
    "2x6x5x3x128": (_ci(2, 6, 5, 3, 128, sample="other"), "conv_in_fast_kernel", 17280),                   # VAE encoder, K = 27
    "1x130x130x3x128-trip2": (_ci(1, 130, 130, 3, 128, sample="storage"), "conv_in_fast_kernel", 17280),    # 16 900 pixels > 512 x 32
    "3x5x7x4x24": (_ci(3, 5, 7, 4, 24), "conv_in_fast_kernel", 27936),                                     # G = 3, groups = 85: thread 255 idle
    "2x5x7x4x440": (_ci(2, 5, 7, 4, 440), "conv_in_fast_kernel", 64512),                                   # the LDS gate, below
    "2x5x7x4x448": (_ci(2, 5, 7, 4, 448), "conv_in_kernel", 576),                                          # the LDS gate, above: 65 664 B
    "2x5x7x4x512": (_ci(2, 5, 7, 4, 512, sample="storage"), "conv_in_kernel", 576),                        # VAE decoder
    "3x5x7x8x64": (_ci(3, 5, 7, 8, 64), "conv_in_fast_kernel", 36864),
    "2x5x7x16x64": (_ci(2, 5, 7, 16, 64), "conv_in_kernel", 2304),                                         # 73 728 B
    "3x5x7x4x5": (_ci(3, 5, 7, 4, 5, sample="other"), "conv_in_kernel", 576),                              # cout % 8
}
CONV_OUT_CASES = {
    "1x8x16x320x8": (_co(1, 8, 16, 320, 8), "conv_out_mfma_kernel", 163840),                               # exactly the 160 KiB the attribute allows
    "3x8x16x64x1": (_co(3, 8, 16, 64, 1), "conv_out_mfma_kernel", 24704),
    "1x16x16x192x5": (_co(1, 16, 16, 192, 5), "conv_out_mfma_kernel", 87936),
    "2x8x32x128x4-gn-silu": (_co(2, 8, 32, 128, 4, coef=True, a_silu=1), "conv_out_mfma_kernel", 56320),
    "2x8x32x128x4-gn": (_co(2, 8, 32, 128, 4, coef=True, a_silu=0), "conv_out_mfma_kernel", 56320),
    "3x5x7x64x3": (_co(3, 5, 7, 64, 3), "conv_out_fast_kernel<4>", 3456),                                  # 105 pixels: a pair straddles two images
    "3x5x7x64x4": (_co(3, 5, 7, 64, 4), "conv_out_fast_kernel<4>", 4608),
    "3x5x7x8x8": (_co(3, 5, 7, 8, 8), "conv_out_fast_kernel<8>", 1152),                                    # nine active lanes
    "1x8x16x384x4": (_co(1, 8, 16, 384, 4), "conv_out_fast_kernel<4>", 27648),                             # cin > 320
    "1x3x5x448x8": (_co(1, 3, 5, 448, 8), "conv_out_fast_kernel<8>", 64512),                               # the LDS gate, below
    "1x3x5x456x8": (_co(1, 3, 5, 456, 8), "conv_out_kernel", 0),                                           # above: 65 664 B
    "2x3x5x512x8": (_co(2, 3, 5, 512, 8), "conv_out_kernel", 0),                                           # VAE encoder, 73 728 B
    "2x97x96x64x4-trip2": (_co(2, 97, 96, 64, 4), "conv_out_fast_kernel<4>", 4608),                         # 9 312 pairs > 1024 x 4
}
CONV_OUT_REFUSED = _co(2, 8, 24, 128, 4, coef=True)                                                        # w % 16: tg_conv_out_takes_coef says no
TRANSPOSE_CASES = {
    "1x128x64": (("transpose", dict(B=1, rows=128, cols=64)), "transpose_big_kernel"),
    "2x256x192": (("transpose", dict(B=2, rows=256, cols=192)), "transpose_big_kernel"),
    "1x127x64": (("transpose", dict(B=1, rows=127, cols=64)), "transpose_kernel"),
    "1x128x63": (("transpose", dict(B=1, rows=128, cols=63)), "transpose_kernel"),
    "3x1x1": (("transpose", dict(B=3, rows=1, cols=1)), "transpose_kernel"),
    "2x33x65": (("transpose", dict(B=2, rows=33, cols=65)), "transpose_kernel"),
    "1x128x64-srcshift4": (("transpose", dict(B=1, rows=128, cols=64, src_shift=4)), "transpose_kernel"),
}
SOFTMAX_CASES = {f"{r}x{c}ld{ld}{'-inplace' if ip else ''}": ("softmax_rows", dict(rows=r, cols=c, ld=ld, inplace=ip))
                 for r, c, ld, ip in ((1, 8, 8, False), (5, 72, 80, False), (4, 512, 512, True), (3, 520, 528, False), (2, 4096, 4096, False))}
PROBS_CASES = {f"L{L}d{hd}q{nq}b{b0}{'-pitched' if p else ''}{'-tokens' if t else ''}":
               ("attn_probs", dict(len=L, head_dim=hd, n_q=nq, b0=b0, pitched=p, tokens=t))
               for L, hd, nq, b0, p, t in ((1, 8, 1, 0, False, False), (63, 40, 5, 0, False, False), (64, 64, 64, 0, False, False), (65, 40, 5, 1, True, False),
                                           (77, 40, 5, 0, False, True), (77, 160, 5, 1, True, True), (256, 64, 5, 0, True, True), (256, 8, 64, 1, False, False),
                                           (256, 160, 1, 1, True, True), (65, 64, 1, 0, False, True), (64, 160, 64, 0, True, False), (1, 40, 5, 1, True, True))}
TIMESTEP_CASES = {f"d{d}f{f}s{s}{'-idx%d' % i if i is not None else ''}-ts{ts}r{r}p{p}":
                  ("timestep", dict(dim=d, flip=f, shift=s, index=i, t_stride=ts, rows=r, pad=p))
                  for d, f, s, i, ts, r, p in ((256, 1, 0, None, 1, 5, 0), (320, 1, 0, 7, 0, 3, 8), (320, 0, 1, 3, 1, 5, 0), (1280, 1, 1, 11, 3, 5, 16),
                                               (1280, 0, 0, None, 0, 2, 0), (256, 0, 1, None, 1, 5, 8))}
GEGLU_CASES = {f"{r}x{i}": ("geglu", dict(rows=r, inner=i)) for r, i in ((1, 8), (3, 24), (1030, 4104))}
ACT_CASES = {f"n{n}-act{act}": ("act", dict(n=n, act=act)) for n in (1, 7, 600000) for act in (0, 1, 2, 3, 9)}
ADD_CASES = {f"n{n}": ("add", dict(n=n)) for n in (1, 7, 8, 9, 4200005)}
HELPER_CASES = {
    "dup_rows 3x24ld40": ("dup_rows", dict(rows=3, cols=24, ld=40)),
    "dup_rows 1030x4104ld4112": ("dup_rows", dict(rows=1030, cols=4104, ld=4112)),
    "conv1x1 3x4x4x35": ("conv1x1", dict(B=3, cin=4, cout=4, hw=35)),
    "conv1x1 2x8x5x300000": ("conv1x1", dict(B=2, cin=8, cout=5, hw=300000)),
    "gaussian 2x4x35": ("gaussian", dict(B=2, C=4, hw=35)),
    "gaussian 2x4x35-mode": ("gaussian", dict(B=2, C=4, hw=35, noise=False)),
    "gaussian 2x4x70001": ("gaussian", dict(B=2, C=4, hw=70001)),
    "add_noise 3x35": ("add_noise", dict(steps=3, n=35)),
    "add_noise 3x180001": ("add_noise", dict(steps=3, n=180001)),
    "shift 3x5x7+2-1": ("shift", dict(planes=3, h=5, w=7, dx=2, dy=-1)),
    "shift 3x5x7-9+0": ("shift", dict(planes=3, h=5, w=7, dx=-9, dy=0)),                 # |dx| >= w: all zero
    "shift 8x300x231-3+5": ("shift", dict(planes=8, h=300, w=231, dx=-3, dy=5)),
    "compose 3x35": ("compose", dict(planes=3, hw=35)),
    "compose 8x70001": ("compose", dict(planes=8, hw=70001)),
    "blend 3x35-fp32": ("blend", dict(planes=3, hw=35, mode=-1)),
    "blend 3x35-f16": ("blend", dict(planes=3, hw=35, mode=1)),
    "blend 3x35-bf16": ("blend", dict(planes=3, hw=35, mode=0)),
    "blend 8x70001-f16": ("blend", dict(planes=8, hw=70001, mode=1)),
}


def all_cases():
    """{id: (entry, make_case keywords)} of every GPU launch.  The storage-type convs also run with out_f32 = 0 (``conv_out_variants``)."""
    out = {}
    for fam, cs in (("conv_in", {k: v[0] for k, v in CONV_IN_CASES.items()}), ("conv_out", conv_out_variants()),
                    ("transpose", {k: v[0] for k, v in TRANSPOSE_CASES.items()}), ("softmax", SOFTMAX_CASES), ("probs", PROBS_CASES),
                    ("timestep", TIMESTEP_CASES), ("geglu", GEGLU_CASES), ("act", ACT_CASES), ("add", ADD_CASES)):
        out.update({f"{fam} {k}": v for k, v in cs.items()})
    out.update(HELPER_CASES)
    return out


def conv_out_variants():
    """every conv_out case for both out_f32 values"""
    out = {}
    for key, ((entry, kw), _, _) in CONV_OUT_CASES.items():
        for f in (1, 0):
            out[f"{key}-{'f32' if f else 'st'}"] = (entry, dict(kw, out_f32=f))
    return out


def plain_twin(a, device):
    """the tg_conv_out launch on the restatement's rounded activations of a tg_conv_out_gn launch: same weight, bias and output type, an output of its own"""
    x = gn_activations(a).to(a["dtype"]).cpu()
    odt = torch.float32 if a["out_f32"] else a["dtype"]
    return dict(a, coef=None, a_silu=0, x=_guarded(x, a["cin"], device), out=_out((a["batch"], a["cout"], a["h"], a["w"]), odt, a["w"], device))


def expected_kernel(cid):
    """the by-hand kernel (and LDS bytes, or None) of a case id of ``all_cases``"""
    fam, _, key = cid.partition(" ")
    if fam == "conv_in":
        return CONV_IN_CASES[key][1:]
    if fam == "conv_out":
        return CONV_OUT_CASES[key.rsplit("-", 1)[0]][1:]
    if fam == "transpose":
        return TRANSPOSE_CASES[key][1], None
    return None
