"""The C-ABI contracts of ``tg_gemm`` and ``tg_attention`` (include/theatergen_hip.h) restated in fp64, for checking single launches.

Every function takes the keyword arguments of ``theatergen_amd.ops.gemm`` / ``ops.attention`` (``gemm_args`` / ``attention_args`` bind a
call's positional arguments to those names) and reads the operands the way the kernels read raw pointers: ``torch.as_strided`` over the
operand's storage, starting at its ``data_ptr`` and walking the pitches of the descriptor (``lda`` / ``ldw``, ``c0`` / ``c1``, ``ldres``,
``ldbvec``, ``a_rows_per_batch`` / ``a_batch_stride``, ``ldt``, the attention ``_ld`` / ``_bs`` pitches), never the tensor's logical shape.
A descriptor that reads past its operand's storage makes ``as_strided`` raise, so these functions also catch out-of-bounds reads.

  * ``gemm_reference(**args)``       -> (out fp64 [M, n_main], out_t fp64 [B, N - n_split, rows_per_batch] or None)
  * ``gn_partials_reference(out, groups, batch, hw)`` -> fp64 [batch, hw / 64, groups, 2] (sum, sum of squares) of the STORED output
  * ``written_region(args)``         -> the storage elements of ``out`` / ``out_t`` the contract writes (``Region`` list)
  * ``read_extents(args)``           -> the storage regions every operand is read from (``Region`` list)
  * ``attention_reference(**args)``  -> fp64 [batch, n_q, heads * head_dim]

The references run on the operands' device (fp64 matrix products; the conv as nine shifted products, no im2col buffer).
"""
import inspect
import math
from dataclasses import dataclass

import torch

ACT_NONE, ACT_SILU, ACT_GELU, ACT_QUICK_GELU = 0, 1, 2, 3


@dataclass
class Region:
    """``sizes`` / ``strides`` elements of ``t``'s dtype starting ``offset`` elements after ``t.data_ptr()``"""
    name: str
    t: torch.Tensor
    offset: int
    sizes: tuple
    strides: tuple

    @property
    def esize(self):
        return self.t.element_size()

    def storage_byte_offset(self):
        """byte offset of the first element from the start of ``t``'s storage"""
        return self.t.data_ptr() - self.t.untyped_storage().data_ptr() + self.offset * self.esize

    def byte_range(self):
        """[lo, hi) bytes of the storage the region touches (empty region: None)"""
        if any(s <= 0 for s in self.sizes):
            return None
        lo = self.storage_byte_offset()
        span = sum((s - 1) * st for s, st in zip(self.sizes, self.strides))
        return lo, lo + (span + 1) * self.esize

    def view(self):
        """the region as a tensor over ``t``'s storage (raises when it leaves the storage)"""
        base = _storage_tensor(self.t)
        return base.as_strided(self.sizes, self.strides, self.storage_byte_offset() // self.esize)

    def byte_view(self, mask):
        """the region's bytes as a view of a uint8 / bool tensor ``mask`` over the whole storage"""
        es = self.esize
        return mask.as_strided(tuple(self.sizes) + (es,), tuple(s * es for s in self.strides) + (1,), self.storage_byte_offset())


def _storage_tensor(t):
    """1-D tensor of t's dtype over t's whole storage"""
    st = t.untyped_storage()
    base = torch.empty(0, dtype=t.dtype, device=t.device)
    base.set_(st, 0, (st.nbytes() // t.element_size(),), (1,))
    return base


def _rd(t, offset, sizes, strides):
    return Region("", t, int(offset), tuple(int(s) for s in sizes), tuple(int(s) for s in strides)).view()


# ---- argument binding --------------------------------------------------------------------------------------------------------------
def _bind(fn, args, kwargs):
    sig = inspect.signature(fn)
    b = sig.bind(*args, **kwargs)
    b.apply_defaults()
    return dict(b.arguments)


def gemm_args(args, kwargs, fn=None):
    """``fn``: the ``ops.gemm`` whose signature binds them (the original one where a test has wrapped the attribute)"""
    from theatergen_amd import ops
    return _bind(fn or ops.gemm, args, kwargs)


def attention_args(args, kwargs, fn=None):
    from theatergen_amd import ops
    return _bind(fn or ops.attention, args, kwargs)


def _geometry(a):
    """the descriptor fields ops.gemm derives from its arguments"""
    M, N, K = int(a["M"]), int(a["N"]), int(a["K"])
    mode = int(a.get("mode") or 0)
    c0 = int(a["c0"] if a.get("c0") is not None else (K if mode == 0 else K // 9))
    c1 = int(a.get("c1") or 0) if a.get("a1") is not None else 0
    n_split = int(a.get("n_split") or 0)
    geglu = bool(a.get("geglu"))
    n_main = n_split if n_split > 0 else (N // 2 if geglu else N)
    rpb = int(a.get("rows_per_batch") or 0)
    return M, N, K, mode, c0, c1, n_split, geglu, n_main, rpb


# ---- activations -------------------------------------------------------------------------------------------------------------------
def _act(v, act):
    if act == ACT_SILU:
        return v * torch.sigmoid(v)
    if act == ACT_GELU:
        return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))
    if act == ACT_QUICK_GELU:
        return v * torch.sigmoid(1.702 * v)
    assert act == ACT_NONE, act
    return v


def _gelu(v):
    return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))


# ---- operand views -----------------------------------------------------------------------------------------------------------------
def _a_rows_region(a):
    """mode 0: the A rows of a0 (and a1) as regions of [M, c] shape (batched A: [B, rows, c])"""
    M, N, K, mode, c0, c1, *_ = _geometry(a)
    arpb, abs_ = int(a.get("a_rows_per_batch") or 0), int(a.get("a_batch_stride") or 0)
    lda = int(a.get("lda") or 0) or c0
    if a.get("a1") is not None:
        return [Region("a0", a["a0"], 0, (M, c0), (c0, 1)), Region("a1", a["a1"], 0, (M, c1), (c1, 1))]
    if arpb > 0:
        assert M % arpb == 0, "batched A with a partial last batch item"
        return [Region("a0", a["a0"], 0, (M // arpb, arpb, c0), (abs_, c0, 1))]
    return [Region("a0", a["a0"], 0, (M, c0), (lda, 1))]


def _conv_input_regions(a):
    conv = [int(v) for v in a["conv"]]
    batch, in_h, in_w = conv[0], conv[1], conv[2]
    M, N, K, mode, c0, c1, *_ = _geometry(a)
    regs = [Region("a0", a["a0"], 0, (batch, in_h, in_w, c0), (in_h * in_w * c0, in_w * c0, c0, 1))]
    if a.get("a1") is not None:
        regs.append(Region("a1", a["a1"], 0, (batch, in_h, in_w, c1), (in_h * in_w * c1, in_w * c1, c1, 1)))
    return regs


def _round(x, dtype):
    return x.to(dtype).to(torch.float64)


def _conv_reference(a, W):
    """fp64 [M, N] implicit-GEMM 3x3 conv of the header's mode 1 (tap-major W [N, 9 C])"""
    batch, in_h, in_w, out_h, out_w, stride, upsample = [int(v) for v in a["conv"]]
    pad_mode = int(a.get("pad_mode") or 0)
    regs = _conv_input_regions(a)
    x = torch.cat([r.view() for r in regs], dim=3)
    dtype = x.dtype
    x = x.to(torch.float64)
    Ct = x.shape[3]
    if a.get("a_coef") is not None:
        # A' = act(A * a[b, c] + d[b, c]) in fp32, rounded to the storage dtype; the zero padding stays zero
        coef = _rd(a["a_coef"], 0, (batch, 2, Ct), (2 * Ct, Ct, 1)).to(torch.float32)
        xf = x.to(torch.float32) * coef[:, 0, None, None, :] + coef[:, 1, None, None, :]
        if a.get("a_silu"):
            xf = xf * torch.sigmoid(xf)
        x = _round(xf, dtype)
    if upsample:
        x = x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    H, Wd = x.shape[1], x.shape[2]
    lo = 0 if pad_mode == 1 else 1
    xp = torch.zeros((batch, H + 2, Wd + 2, Ct), dtype=torch.float64, device=x.device)
    xp[:, lo:lo + H, lo:lo + Wd] = x
    Wt = W.reshape(W.shape[0], 9, Ct)
    acc = torch.zeros((batch * out_h * out_w, W.shape[0]), dtype=torch.float64, device=x.device)
    for ky in range(3):
        for kx in range(3):
            win = xp[:, ky:ky + stride * (out_h - 1) + 1:stride, kx:kx + stride * (out_w - 1) + 1:stride]
            acc += win.reshape(-1, Ct) @ Wt[:, 3 * ky + kx].t()
    return acc


def a_matrix(a):
    """mode 0: fp64 A [M, K] as the kernel reads it"""
    regs = _a_rows_region(a)
    M = int(a["M"])
    return torch.cat([r.view().reshape(M, -1) for r in regs], dim=1).to(torch.float64)


def ln_row_stats(a):
    """fp64 (mean, rstd) of the A rows (biased variance over the stored values, nn.LayerNorm)"""
    A = a_matrix(a)
    mean = A.mean(dim=1)
    var = ((A - mean[:, None]) ** 2).mean(dim=1)
    return mean, 1.0 / torch.sqrt(var + float(a["ln"][2]))


def gemm_reference(**a):
    """fp64 (out [M, n_main], out_t [B, N - n_split, rows_per_batch] or None) of one ``ops.gemm`` call"""
    M, N, K, mode, c0, c1, n_split, geglu, n_main, rpb = _geometry(a)
    ldw = int(a.get("ldw") or 0) or K
    W = _rd(a["w"], 0, (N, K), (ldw, 1)).to(torch.float64)
    if mode == 1:
        acc = _conv_reference(a, W)
    else:
        acc = a_matrix(a) @ W.t()
    dev = acc.device
    ln = a.get("ln")
    if ln is not None:
        # out = epilogue( rstd[m] * (sum_k A W' - mean[m] * ln_u[n]) + ln_v[n] )
        u = _rd(ln[0], 0, (N,), (1,)).to(torch.float64)
        v = _rd(ln[1], 0, (N,), (1,)).to(torch.float64)
        if len(ln) > 3 and ln[3] is not None:
            st = _rd(ln[3], 0, (M, 2), (2, 1)).to(torch.float64)            # (rstd, -rstd * mean) as the kernel is given them
            acc = st[:, 0:1] * acc + st[:, 1:2] * u[None, :] + v[None, :]
        else:
            mean, rstd = ln_row_stats(a)
            acc = rstd[:, None] * (acc - mean[:, None] * u[None, :]) + v[None, :]
    if a.get("bias") is not None:
        acc = acc + _rd(a["bias"], 0, (N,), (1,)).to(torch.float64)[None, :]
    if a.get("bvec") is not None:
        bv = a["bvec"]
        nb = (M + rpb - 1) // rpb
        rows = _rd(bv, 0, (nb, N), (int(bv.stride(0)), 1)).to(torch.float64)
        acc = acc + rows[torch.arange(M, device=dev) // rpb]
    if a.get("res") is not None:
        r = a["res"]
        acc = acc + _rd(r, 0, (M, N), (int(r.stride(0)), 1)).to(torch.float64)
    scale = float(a.get("out_scale", 1.0))
    if geglu:
        g = acc.reshape(M, N // 64, 2, 32)
        return (g[:, :, 0, :] * _gelu(g[:, :, 1, :])).reshape(M, N // 2) * scale, None
    acc = _act(acc, int(a.get("act") or 0)) * scale
    if n_split > 0:
        B = M // rpb
        out_t = acc[:, n_split:].reshape(B, rpb, N - n_split).transpose(1, 2)
        return acc[:, :n_split], out_t
    return acc, None


def gn_partials_reference(out, groups, batch, hw):
    """fp64 [batch, hw / 64, groups, 2]: (sum, sum of squares) of the stored output per 64-pixel block and channel group"""
    C = out.shape[-1]
    x = out.to(torch.float64).reshape(batch, hw // 64, 64, groups, C // groups)
    return torch.stack([x.sum(dim=(2, 4)), (x * x).sum(dim=(2, 4))], dim=-1)


# ---- where a launch reads and writes -----------------------------------------------------------------------------------------------
def written_region(a):
    """the ``out`` (and ``out_t``) storage elements the contract writes"""
    M, N, K, mode, c0, c1, n_split, geglu, n_main, rpb = _geometry(a)
    out = a["out"]
    regs = [Region("out", out, 0, (M, n_main), (int(out.stride(0)), 1))]
    if n_split > 0:
        B, nt, ldt = M // rpb, N - n_split, int(a["ldt"])
        regs.append(Region("out_t", a["out_t"], 0, (B, nt, rpb), (nt * ldt, ldt, 1)))
    return regs


def read_extents(a):
    """every operand's read region (the epilogue operands over the N columns the contract adds them to)"""
    M, N, K, mode, c0, c1, n_split, geglu, n_main, rpb = _geometry(a)
    regs = _conv_input_regions(a) if mode == 1 else _a_rows_region(a)
    ldw = int(a.get("ldw") or 0) or K
    regs.append(Region("w", a["w"], 0, (N, K), (ldw, 1)))
    if a.get("bias") is not None:
        regs.append(Region("bias", a["bias"], 0, (N,), (1,)))
    if a.get("bvec") is not None:
        regs.append(Region("bvec", a["bvec"], 0, ((M + rpb - 1) // rpb, N), (int(a["bvec"].stride(0)), 1)))
    if a.get("res") is not None:
        regs.append(Region("res", a["res"], 0, (M, N), (int(a["res"].stride(0)), 1)))
    if a.get("a_coef") is not None:
        regs.append(Region("a_coef", a["a_coef"], 0, (int(a["conv"][0]) * 2 * (c0 + c1),), (1,)))
    ln = a.get("ln")
    if ln is not None:
        regs += [Region("ln_u", ln[0], 0, (N,), (1,)), Region("ln_v", ln[1], 0, (N,), (1,))]
        if len(ln) > 3 and ln[3] is not None:
            regs.append(Region("ln_rows", ln[3], 0, (M, 2), (2, 1)))
    return regs


def attention_written_region(a):
    HD = int(a["heads"]) * int(a["head_dim"])
    return [Region("out", a["out"], 0, (int(a["batch"]), int(a["n_q"]), HD), (int(a["out_bs"]), int(a["out_ld"]), 1))]


def attention_read_extents(a):
    B, HD, nq = int(a["batch"]), int(a["heads"]) * int(a["head_dim"]), int(a["n_q"])
    regs = [Region("q", a["q"], 0, (B, nq, HD), (int(a["q_bs"]), int(a["q_ld"]), 1))]
    for s in ("0", "1"):
        L = int(a["len" + s])
        if L <= 0:
            continue
        regs.append(Region("k" + s, a["k" + s], 0, (B, L, HD), (int(a[f"k{s}_bs"]), int(a[f"k{s}_ld"]), 1)))
        regs.append(Region("vt" + s, a["vt" + s], 0, (B, HD, L), (int(a[f"vt{s}_bs"]), int(a[f"vt{s}_ld"]), 1)))
    if a.get("mask") is not None:
        bs, hs, qs = attention_mask_strides(a)
        # exactly the elements read: a zero stride reads one item / head / row for all
        regs.append(Region("mask", a["mask"], 0, (B if bs else 1, int(a["heads"]) if hs else 1, nq if qs else 1, int(a["len0"])), (bs, hs, qs, 1)))
    if a.get("w1_dev") is not None and int(a["len1"]) > 0:
        regs.append(Region("w1_dev", a["w1_dev"], 0, (attention_w1_count(a),), (1,)))
    return regs


def attention_mask_strides(a):
    """(mask_bs, mask_hs, mask_qs) in elements: the descriptor's own fields where the dict has them (the mask is then a pointer), else what
    ``ops.attention`` derives from a contiguous [Bm, Hm, Qm, len0] tensor"""
    if "mask_bs" in a:
        return int(a["mask_bs"]), int(a["mask_hs"]), int(a["mask_qs"])
    bm, hm, qm, L = a["mask"].shape
    return (hm * qm * L if bm > 1 else 0), (qm * L if hm > 1 else 0), (L if qm > 1 else 0)


def attention_w1_count(a):
    """floats behind ``w1_dev``: ``ip_scale_count`` of tg_attention_ps where the dict has it (0 and 1 both mean one), else ``ops.attention``'s
    rule (a tensor of ``batch`` elements is per item)"""
    if a.get("ip_scale_count") is not None:
        return max(1, int(a["ip_scale_count"]))
    return int(a["batch"]) if a["w1_dev"].numel() == int(a["batch"]) else 1


# ---- attention ---------------------------------------------------------------------------------------------------------------------
def _segment(q, k, vt, scale, bias=None, causal=False, q0=0):
    """softmax(scale q k^T + bias) v for one (batch item, head chunk): q [h, n, d], k [h, L, d], vt [h, d, L], fp64"""
    s = scale * (q @ k.transpose(1, 2))
    if bias is not None:
        s = s + bias
    if causal:
        i = torch.arange(q0, q0 + q.shape[1], device=q.device)[:, None]
        j = torch.arange(k.shape[1], device=q.device)[None, :]
        s = s.masked_fill(j > i, float("-inf"))
    return torch.softmax(s, dim=-1) @ vt.transpose(1, 2)


def attention_reference(q_chunk=2048, **a):
    """fp64 [batch, n_q, heads * head_dim]: O = softmax(s Q K0^T + mask [causal]) V0 + w1[b] softmax(s Q K1^T) V1, per (batch item, head) and
    query chunk so that self-attention at n = 9216 fits.  ``mask``: a contiguous [Bm, Hm, Qm, len0] tensor as ``ops.attention`` takes it, or a
    pointer with ``mask_bs`` / ``mask_hs`` / ``mask_qs`` (the descriptor's fields); ``w1_dev``: one float or, with ``ip_scale_count`` = batch
    (tg_attention_ps), one per batch item; causal and mask both apply when both are set"""
    B, H, D, nq = int(a["batch"]), int(a["heads"]), int(a["head_dim"]), int(a["n_q"])
    HD = H * D
    regs = {r.name: r for r in attention_read_extents(a)}
    scale = float(a["scale"])
    if a.get("w1_dev") is not None and "w1_dev" in regs:
        w1s = [float(v) for v in regs["w1_dev"].view().tolist()]                  # one float, or one per batch item (tg_attention_ps)
        w1s = w1s if len(w1s) > 1 else w1s * B
    else:
        w1s = [float(a.get("w1") or 0.0)] * B
    mask = None
    if a.get("mask") is not None:
        mask = _rd(a["mask"], 0, (B, H, nq, int(a["len0"])), attention_mask_strides(a) + (1,))     # broadcast by the zero strides
    q_all = regs["q"].view()
    out = torch.empty((B, nq, HD), dtype=torch.float64, device=q_all.device)
    segs = [s for s in ("0", "1") if int(a["len" + s]) > 0]
    kv = {s: (regs["k" + s].view(), regs["vt" + s].view()) for s in segs}
    for b in range(B):
        for h in range(H):
            cs = slice(h * D, (h + 1) * D)
            for i0 in range(0, nq, q_chunk):
                i1 = min(nq, i0 + q_chunk)
                q = q_all[b, i0:i1, cs].to(torch.float64)[None]
                acc = 0
                for s in segs:
                    k = kv[s][0][b, :, cs].to(torch.float64)[None]
                    vt = kv[s][1][b, cs, :].to(torch.float64)[None]
                    bias = None
                    if s == "0" and mask is not None:
                        bias = mask[b, h, i0:i1].to(torch.float64)[None]
                    o = _segment(q, k, vt, scale, bias, bool(a.get("causal")) and s == "0", i0)     # causal and mask: both apply
                    acc = acc + (o if s == "0" else w1s[b] * o)
                out[b, i0:i1, cs] = acc[0]
    return out


# ---- the comparison ----------------------------------------------------------------------------------------------------------------
def compare(got, ref, l2_tol, max_tol, block=64):
    """metrics of a stored kernel output against its fp64 reference: the whole-tensor rel-L2 and max|err| / max|ref| of
    ``parity_metrics.metrics``, plus the worst rel-L2 over ``block`` x ``block`` tiles of the 2-D (rows, columns) view.  A fault
    confined to one tile of a large output (a tile scaled by 2 %, one column tile without its bias) moves the whole-tensor numbers by
    the tile's share only; the tile-local number sees it at full size.  Tiles whose reference is under a tenth of the tensor's rms
    are measured against that floor (no division by a near-zero tile).  The tile bound is twice ``l2_tol``: one rounding to the storage
    dtype is up to 2^-8 (bf16) / 2^-11 (fp16) of an element, above ``l2_tol``, and 4096 elements average it less than a whole tensor
    does; a tile scaled by 1.02 is still 3x over it.  -> (ok, metrics)"""
    g = got.detach().to(torch.float64)
    r = ref.detach().to(torch.float64).to(g.device)
    assert g.shape == r.shape, f"{tuple(g.shape)} vs {tuple(r.shape)}"
    g2, r2 = g.reshape(-1, g.shape[-1]), r.reshape(-1, r.shape[-1])
    d = g2 - r2
    ref_norm = float(r2.norm())
    m = {"rel_l2": float(d.norm()) / max(ref_norm, 1e-30), "max_rel": float(d.abs().max()) / max(float(r2.abs().max()), 1e-30),
         "finite": bool(torch.isfinite(g).all())}
    R, Cn = r2.shape
    rb, cb = (R + block - 1) // block, (Cn + block - 1) // block
    pad = (0, cb * block - Cn, 0, rb * block - R)
    dd = torch.nn.functional.pad(d * d, pad).reshape(rb, block, cb, block).sum(dim=(1, 3))
    rr = torch.nn.functional.pad(r2 * r2, pad).reshape(rb, block, cb, block).sum(dim=(1, 3))
    cnt = torch.nn.functional.pad(torch.ones_like(r2), pad).reshape(rb, block, cb, block).sum(dim=(1, 3))
    floor = (0.1 * ref_norm / math.sqrt(max(R * Cn, 1))) ** 2 * cnt
    tile = torch.sqrt(dd / torch.maximum(rr, floor).clamp_min(1e-300))
    m["tile_rel_l2"] = float(tile.max())
    ok = m["finite"] and m["rel_l2"] <= l2_tol and m["max_rel"] <= max_tol and m["tile_rel_l2"] <= 2 * l2_tol
    return ok, m


def check(got, ref, what, l2_tol, max_tol, record=True, **extra):
    """``compare`` + record (parity_metrics.jsonl; a failure always) + assert"""
    from tests import parity_metrics as pm
    ok, m = compare(got, ref, l2_tol, max_tol)
    if record or not ok:
        pm.record(what, m, l2_tol=l2_tol, max_tol=max_tol, **extra)
    assert ok, f"{what}: {m} (tolerances rel-L2 {l2_tol:.1e}, max {max_tol:.1e})"
    return m
