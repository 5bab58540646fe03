"""The C-ABI contracts of ``tg_attention_bwd`` and ``tg_attention_bwd_cross`` (include/theatergen_hip.h: ``tg_attn_bwd_desc``,
``tg_attn_bwd_cross_desc``) restated in fp64, for checking single launches of the attention reverse pass.

A descriptor is a plain dict with the header's field names; tensors stand for the pointers (a tensor's ``data_ptr`` is the pointer, so a
column slice of a fused buffer is a valid operand).  Operands are read the way the kernel reads raw pointers — ``torch.as_strided`` over
the operand's storage along ``ld`` / ``bs`` / ``q_ld`` / ``q_bs`` / ``k_ld`` / ``k_bs`` / ``t_ld`` / ``t_bs`` / ``extra_ld``
(``gemm_contract.Region``), never the tensor's logical shape; a descriptor that reads past a storage makes ``as_strided`` raise.

    P  = softmax(scale Q K^T)                 dP = dO V^T (+ extra)                D = rowsum(P o dP)
    dS = ds_scale P o (dP - D)                (self-attention: ds_scale = scale)
    dQ = r(dS) K,   dK = r(dS)^T Q,   dV = r(P)^T dO        r = one rounding to the storage dtype ("P and dS are rounded to the storage
                                                            dtype where they enter a product"); D is formed from the unrounded P

  * ``self_reference(a)``  -> {"dq", "dk", "dv"} fp64 [batch, n, heads * head_dim];  ``cross_reference(a)`` -> {"dq"} [batch, n_q, ...]
        ``rounded=False`` switches the two roundings off (then it is autograd's formula), ``work=torch.float32`` runs every product in fp32,
        ``round_out=True`` rounds the outputs once to the storage dtype (the fp32 restatement of tests/test_attn_bwd_contract_cpu.py)
  * ``self_read_extents`` / ``cross_read_extents``, ``self_written_region`` / ``cross_written_region``  (``Region`` lists; the written
        region includes the ``stats`` scratch the launches fill)
  * ``transposes_consistent(a)``: qt / kt / doutt ARE the transposes of q / k / dout over the columns the contract reads
  * ``magnitude=True``: the same sums over absolute values, the scale a reference that cancels to zero is measured against (``compare``)
  * ``block_rel_l2(got, ref, heads)`` -> fp64 [batch, heads, blocks]: rel-L2 of every (batch item, head, 128-row block) — the unit one
        workgroup owns — and ``compare`` / ``check``: whole-tensor rel-L2 and max|err| / max|ref| plus the worst block of both.
"""
import math

import torch

from tests.gemm_contract import Region

BLOCK = 128


# ---- descriptors -------------------------------------------------------------------------------------------------------------------
def self_desc(q, k, v, dout, qt, kt, doutt, stats, dq, dk, dv, *, batch, heads, head_dim, n, ld, bs, t_ld, t_bs, scale):
    return dict(batch=int(batch), heads=int(heads), head_dim=int(head_dim), n=int(n), q=q, k=k, v=v, dout=dout, ld=int(ld), bs=int(bs),
                qt=qt, kt=kt, doutt=doutt, t_ld=int(t_ld), t_bs=int(t_bs), stats=stats, dq=dq, dk=dk, dv=dv, scale=float(scale))


def cross_desc(q, dout, k, v, kt, extra, stats, dq, *, batch, heads, head_dim, n_q, n_k, q_ld, q_bs, k_ld, k_bs, t_ld, t_bs, extra_ld, scale,
               ds_scale):
    return dict(batch=int(batch), heads=int(heads), head_dim=int(head_dim), n_q=int(n_q), n_k=int(n_k), q=q, dout=dout, q_ld=int(q_ld),
                q_bs=int(q_bs), k=k, v=v, k_ld=int(k_ld), k_bs=int(k_bs), kt=kt, t_ld=int(t_ld), t_bs=int(t_bs), extra=extra,
                extra_ld=int(extra_ld), stats=stats, dq=dq, scale=float(scale), ds_scale=float(ds_scale))


def _rows(name, t, B, n, inner, ld, bs):
    return Region(name, t, 0, (B, n, inner), (bs, ld, 1))


def _cols(name, t, B, inner, n, t_ld, t_bs):
    return Region(name, t, 0, (B, inner, n), (t_bs, t_ld, 1))


def _stats(a, n):
    return Region("stats", a["stats"], 0, (a["batch"], a["heads"], n, 2), (a["heads"] * n * 2, n * 2, 2, 1))


def self_read_extents(a):
    B, n, inner = a["batch"], a["n"], a["heads"] * a["head_dim"]
    return [_rows(x, a[x], B, n, inner, a["ld"], a["bs"]) for x in ("q", "k", "v", "dout")] + \
           [_cols(x, a[x], B, inner, n, a["t_ld"], a["t_bs"]) for x in ("qt", "kt", "doutt")]


def self_written_region(a):
    B, n, inner = a["batch"], a["n"], a["heads"] * a["head_dim"]
    return [_rows(x, a[x], B, n, inner, a["ld"], a["bs"]) for x in ("dq", "dk", "dv")] + [_stats(a, n)]


def cross_read_extents(a):
    B, nq, nk, inner = a["batch"], a["n_q"], a["n_k"], a["heads"] * a["head_dim"]
    regs = [_rows(x, a[x], B, nq, inner, a["q_ld"], a["q_bs"]) for x in ("q", "dout")]
    regs += [_rows(x, a[x], B, nk, inner, a["k_ld"], a["k_bs"]) for x in ("k", "v")]
    regs.append(_cols("kt", a["kt"], B, inner, (nk + 7) // 8 * 8, a["t_ld"], a["t_bs"]))       # the zero padding is part of the contract
    if a.get("extra") is not None:
        H = a["heads"]
        regs.append(Region("extra", a["extra"], 0, (B, H, nq, nk), (H * nq * a["extra_ld"], nq * a["extra_ld"], a["extra_ld"], 1)))
    return regs


def cross_written_region(a):
    return [_rows("dq", a["dq"], a["batch"], a["n_q"], a["heads"] * a["head_dim"], a["q_ld"], a["q_bs"]), _stats(a, a["n_q"])]


def transposes_consistent(a):
    """True when the transposed operands hold the transposes of the row-major ones (self: qt, kt, doutt; cross: kt with zero padding)"""
    ext = {r.name: r.view() for r in (cross_read_extents(a) if "n_q" in a else self_read_extents(a))}
    if "n_q" in a:
        nk = a["n_k"]
        kt, pad = ext["kt"], ext["kt"][:, :, nk:]
        return torch.equal(kt[:, :, :nk], ext["k"].transpose(1, 2)) and (pad.numel() == 0 or float(pad.float().abs().max()) == 0.0)
    return all(torch.equal(ext[t], ext[s].transpose(1, 2)) for s, t in (("q", "qt"), ("k", "kt"), ("dout", "doutt")))


# ---- test operands -----------------------------------------------------------------------------------------------------------------
def _randn(shape, g, std, dtype):
    return (torch.randn(shape, generator=g) * std).to(dtype)


def _t_padded(src, B, n, inner, t_ld, transpose, fill):
    """[B, inner, t_ld]: columns < n = src^T (through ``transpose``: ops.transpose on the GPU), the rest ``fill``"""
    t = transpose(src.contiguous(), B, n, inner)
    if t_ld == n:
        return t
    out = torch.full((B, inner, t_ld), fill, dtype=src.dtype, device=src.device)
    out[:, :, :n] = t
    return out


def _torch_transpose(src, B, rows, cols):
    return src.reshape(B, rows, cols).transpose(1, 2).contiguous()


def make_self_case(dtype, B, n, heads, d, *, device="cpu", qmul=1.0, layout="plain", seed=0, transpose=None):
    """a ``tg_attn_bwd_desc`` with N(0, 1) q (x ``qmul``), k, v and N(0, 0.25) dout, drawn on the CPU from ``seed`` (the same bits on every
    device).  ``layout="fused"``: q, k, v are column slices of ONE [batch * (n + 5) + 3, 3 * inner + 8] buffer (ld = 3 * inner + 8, a gap of five
    rows between batch items), dout / dq / dk / dv are buffers of that pitch of their own (the descriptor has one ``ld`` / ``bs`` for all
    seven), t_ld = n + 8; every element the contract does not read is NaN.  Outputs and ``stats`` come back NaN-filled."""
    transpose = transpose or _torch_transpose
    inner = heads * d
    g = torch.Generator().manual_seed(1000 * seed + 17 * B + n + 3 * heads + d)
    q, k, v, do = [_randn((B, n, inner), g, s, dtype).to(device) for s in (qmul, 1.0, 1.0, 0.5)]
    nan = float("nan")
    if layout == "plain":
        ld, bs, t_ld = inner, n * inner, n
        dq, dk, dv = (torch.full((B, n, inner), nan, dtype=dtype, device=device) for _ in range(3))
    else:
        assert layout == "fused", layout
        ld, rows, t_ld = 3 * inner + 8, B * (n + 5) + 3, n + 8
        bs = (n + 5) * ld
        fused = torch.full((rows, ld), nan, dtype=dtype, device=device)
        dbuf = torch.full((rows, ld), nan, dtype=dtype, device=device)
        for b in range(B):
            r = slice(b * (n + 5), b * (n + 5) + n)
            fused[r, 0:inner], fused[r, inner:2 * inner], fused[r, 2 * inner:3 * inner], dbuf[r, :inner] = q[b], k[b], v[b], do[b]
        qv, kv, vv, dov = fused[:, 0:inner], fused[:, inner:2 * inner], fused[:, 2 * inner:3 * inner], dbuf[:, :inner]
        dq, dk, dv = (torch.full((rows, ld), nan, dtype=dtype, device=device) for _ in range(3))
    qt, kt, dot = (_t_padded(t, B, n, inner, t_ld, transpose, nan) for t in (q, k, do))
    if layout == "fused":
        q, k, v, do = qv, kv, vv, dov
    stats = torch.full((B, heads, n, 2), nan, dtype=torch.float32, device=device)
    return self_desc(q, k, v, do, qt, kt, dot, stats, dq, dk, dv, batch=B, heads=heads, head_dim=d, n=n, ld=ld, bs=bs, t_ld=t_ld,
                     t_bs=inner * t_ld, scale=d ** -0.5)


def make_cross_case(dtype, B, n_q, n_k, heads, d, *, device="cpu", qmul=1.0, with_extra=True, weight=0.4, layout="plain", seed=0,
                    transpose=None):
    """a ``tg_attn_bwd_cross_desc``: ds_scale = ``weight`` x scale, ``extra`` N(0, 1) fp32.  ``layout="pitched"``: q / dout / dq rows of pitch
    inner + 8 with a two-row gap between items, k / v rows of pitch inner + 16, extra_ld = n_k + 3, kt of pitch roundup8(n_k) + 8 — zero in
    columns [n_k, roundup8(n_k)) as the header requires, NaN in every other element the contract does not read."""
    transpose = transpose or _torch_transpose
    inner, lp = heads * d, (n_k + 7) // 8 * 8
    g = torch.Generator().manual_seed(1000 * seed + 17 * B + n_q + 5 * n_k + 3 * heads + d)
    q, do = _randn((B, n_q, inner), g, qmul, dtype).to(device), _randn((B, n_q, inner), g, 0.5, dtype).to(device)
    k, v = _randn((B, n_k, inner), g, 1.0, dtype).to(device), _randn((B, n_k, inner), g, 1.0, dtype).to(device)
    ex = torch.randn((B, heads, n_q, n_k), generator=g).to(device) if with_extra else None
    nan = float("nan")
    kt_cols = transpose(k.contiguous(), B, n_k, inner)
    if layout == "plain":
        q_ld, q_bs, k_ld, k_bs, t_ld, e_ld = inner, n_q * inner, inner, n_k * inner, lp, n_k
        dq = torch.full((B, n_q, inner), nan, dtype=dtype, device=device)
        extra = ex
    else:
        assert layout == "pitched", layout
        q_ld, k_ld, t_ld, e_ld = inner + 8, inner + 16, lp + 8, n_k + 3
        q_bs, k_bs = (n_q + 2) * q_ld, (n_k + 1) * k_ld

        def pitched(src, n, ld, bs):
            buf = torch.full((B * bs // ld, ld), nan, dtype=dtype, device=device)
            for b in range(B):
                buf[b * bs // ld:b * bs // ld + n, :inner] = src[b]
            return buf
        q, do, k, v = pitched(q, n_q, q_ld, q_bs), pitched(do, n_q, q_ld, q_bs), pitched(k, n_k, k_ld, k_bs), pitched(v, n_k, k_ld, k_bs)
        dq = torch.full((B * (n_q + 2), q_ld), nan, dtype=dtype, device=device)
        extra = None
        if with_extra:
            extra = torch.full((B, heads, n_q, e_ld), nan, dtype=torch.float32, device=device)
            extra[..., :n_k] = ex
    kt = torch.full((B, inner, t_ld), nan, dtype=dtype, device=device)
    kt[:, :, :lp] = 0
    kt[:, :, :n_k] = kt_cols
    stats = torch.full((B, heads, n_q, 2), nan, dtype=torch.float32, device=device)
    scale = d ** -0.5
    return cross_desc(q, do, k, v, kt, extra, stats, dq, batch=B, heads=heads, head_dim=d, n_q=n_q, n_k=n_k, q_ld=q_ld, q_bs=q_bs, k_ld=k_ld,
                      k_bs=k_bs, t_ld=t_ld, t_bs=inner * t_ld, extra_ld=e_ld, scale=scale, ds_scale=weight * scale)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def head_grads(q, k, v, do, scale, ds_scale, extra, dtype, work=torch.float64, rounded=True, want_kv=True, magnitude=False):
    """one (batch item, head): q, do [n_q, d], k, v [n_k, d], extra [n_q, n_k] or None -> (dq, dk, dv) in ``work`` precision.
    ``magnitude``: the same sums over the absolute values of their terms, with |dP| + |D| for dP - D (what the results cancel from)"""
    q, k, v, do = (t.to(work) for t in (q, k, v, do))
    P = torch.softmax(scale * (q @ k.t()), dim=-1)
    dP = do @ v.t()
    if extra is not None:
        dP = dP + extra.to(work)
    D = (P * dP).sum(dim=-1, keepdim=True)
    if magnitude:
        dS = abs(ds_scale) * P * (dP.abs() + D.abs())
        return dS @ k.abs(), dS.t() @ q.abs(), P.t() @ do.abs()
    dS = ds_scale * P * (dP - D)
    if rounded:
        P, dS = P.to(dtype).to(work), dS.to(dtype).to(work)
    dq = dS @ k
    if not want_kv:
        return dq, None, None
    return dq, dS.t() @ q, P.t() @ do


def _finish(x, dtype, round_out):
    return x.to(dtype).to(torch.float64) if round_out else x.to(torch.float64)


def self_reference(a, work=torch.float64, rounded=True, round_out=False, magnitude=False):
    B, H, D, n = a["batch"], a["heads"], a["head_dim"], a["n"]
    ext = {r.name: r.view() for r in self_read_extents(a) if r.name in ("q", "k", "v", "dout")}
    dtype, dev = ext["q"].dtype, ext["q"].device
    out = {x: torch.empty((B, n, H * D), dtype=torch.float64, device=dev) for x in ("dq", "dk", "dv")}
    for b in range(B):
        for h in range(H):
            cs = slice(h * D, (h + 1) * D)
            g = head_grads(ext["q"][b, :, cs], ext["k"][b, :, cs], ext["v"][b, :, cs], ext["dout"][b, :, cs], a["scale"], a["scale"], None,
                           dtype, work, rounded, magnitude=magnitude)
            for x, t in zip(("dq", "dk", "dv"), g):
                out[x][b, :, cs] = _finish(t, dtype, round_out)
    return out


def cross_reference(a, work=torch.float64, rounded=True, round_out=False, magnitude=False):
    B, H, D, nq = a["batch"], a["heads"], a["head_dim"], a["n_q"]
    ext = {r.name: r.view() for r in cross_read_extents(a) if r.name != "kt"}
    dtype, dev = ext["q"].dtype, ext["q"].device
    dq = torch.empty((B, nq, H * D), dtype=torch.float64, device=dev)
    for b in range(B):
        for h in range(H):
            cs = slice(h * D, (h + 1) * D)
            ex = ext["extra"][b, h] if "extra" in ext else None
            g = head_grads(ext["q"][b, :, cs], ext["k"][b, :, cs], ext["v"][b, :, cs], ext["dout"][b, :, cs], a["scale"], a["ds_scale"], ex,
                           dtype, work, rounded, want_kv=False, magnitude=magnitude)
            dq[b, :, cs] = _finish(g[0], dtype, round_out)
    return {"dq": dq}


# ---- the comparison ----------------------------------------------------------------------------------------------------------------
def _blocks(x, heads):
    """[B, n, heads * d] -> [B, heads, blocks, BLOCK * d] zero-padded to whole blocks"""
    B, n, inner = x.shape
    nb = (n + BLOCK - 1) // BLOCK
    x = torch.nn.functional.pad(x, (0, 0, 0, nb * BLOCK - n))
    return x.reshape(B, nb, BLOCK, heads, inner // heads).permute(0, 3, 1, 2, 4).reshape(B, heads, nb, -1)


CANCEL = 2.0 ** -10


def block_rel_l2(got, ref, heads, mag=None):
    """fp64 [batch, heads, blocks]: ||got - ref|| / ||ref|| over each (batch item, head, 128-row block).  A block whose reference is under
    a tenth of the tensor's rms per element is measured against that floor (no division by a near-zero block); ``mag``: see ``compare``."""
    g, r = got.detach().to(torch.float64), ref.detach().to(torch.float64).to(got.device)
    assert g.shape == r.shape, f"{tuple(g.shape)} vs {tuple(r.shape)}"
    dd = (_blocks(g - r, heads) ** 2).sum(-1)
    rr = (_blocks(r, heads) ** 2).sum(-1)
    cnt = _blocks(torch.ones_like(r), heads).sum(-1)
    floor = (0.1 * float(r.norm()) / math.sqrt(max(r.numel(), 1))) ** 2 * cnt
    if mag is not None:
        floor = torch.maximum(floor, CANCEL ** 2 * (_blocks(mag.to(torch.float64).to(g.device), heads) ** 2).sum(-1))
    return torch.sqrt(dd / torch.maximum(rr, floor).clamp_min(1e-300))


def compare(got, ref, heads, l2_tol, max_tol, mag=None):
    """-> (ok, metrics): ``rel_l2`` / ``max_rel`` of the whole tensor (parity_metrics' definitions), ``block_rel_l2`` and ``block_max_rel``
    (max|err| of a block over the larger of the block's peak and a tenth of the tensor's) of the worst (item, head, 128-row block) with
    its coordinates ``block_at``.  Both tolerances hold for the whole tensor AND for every block.
    ``mag`` (the ``magnitude=True`` restatement): a reference that cancels to nothing — one key: P = 1, dP - D = 0, dQ = 0 identically — has no
    scale of its own.  dP - D is formed in fp32, a few 2^-24 of |dP| + |D| off; norms and peaks of the reference are therefore taken no
    smaller than ``CANCEL`` = 2^-10 of the magnitude restatement's, which admits errors of l2_tol x 2^-10 = 2^-18 (bf16) / 2^-21 (fp16) of the
    terms.  Inert for every reference that does not cancel (a sum of ~n random-signed terms keeps ~n^-1/2 of its magnitude)."""
    g, r = got.detach().to(torch.float64), ref.detach().to(torch.float64).to(got.device)
    assert g.shape == r.shape, f"{tuple(g.shape)} vs {tuple(r.shape)}"
    d = g - r
    peak, norm = float(r.abs().max()), float(r.norm())
    if mag is not None:
        mag = mag.to(torch.float64).to(g.device)
        peak, norm = max(peak, CANCEL * float(mag.abs().max())), max(norm, CANCEL * float(mag.norm()))
    peak, norm = max(peak, 1e-30), max(norm, 1e-30)
    blk = block_rel_l2(g, r, heads, mag)
    bmax = _blocks(d, heads).abs().amax(-1) / _blocks(r, heads).abs().amax(-1).clamp_min(0.1 * peak)
    at = [int(i) for i in torch.unravel_index(torch.argmax(blk), blk.shape)]
    m = {"rel_l2": float(d.norm()) / norm, "max_rel": float(d.abs().max()) / peak,
         "block_rel_l2": float(blk.max()), "block_at": at, "block_max_rel": float(bmax.max()), "finite": bool(torch.isfinite(g).all())}
    ok = m["finite"] and max(m["rel_l2"], m["block_rel_l2"]) <= l2_tol and max(m["max_rel"], m["block_max_rel"]) <= max_tol
    return ok, m


def check(got, ref, heads, what, l2_tol, max_tol, mag=None, **extra):
    """``compare`` + record (parity_metrics.jsonl) + assert"""
    from tests import parity_metrics as pm
    ok, m = compare(got, ref, heads, l2_tol, max_tol, mag)
    pm.record(what, m, l2_tol=l2_tol, max_tol=max_tol, **extra)
    assert ok, f"{what}: {m} (tolerances rel-L2 {l2_tol:.1e}, max {max_tol:.1e}, whole tensor and every block)"
    return m
