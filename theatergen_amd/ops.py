"""Tensor-level wrappers over the C ABI (one function per kernel family).

PyTorch is used ONLY for device memory (``torch.empty`` / views / data_ptr) and the current HIP stream;
every computation is a call into libtheatergen_hip.so.  Activations are token-major 2-D views
``[rows, channels]`` (``rows = batch * h * w``) in bf16 or fp16.
"""
import ctypes as C
import os

import torch

from . import _lib
from ._lib import ACT_GELU, ACT_NONE, ACT_QUICK_GELU, ACT_SILU, AttnDesc, GemmDesc  # noqa: F401

_workspaces = {}


def _dt(t):
    if t.dtype == torch.bfloat16:
        return _lib.TG_BF16
    if t.dtype == torch.float16:
        return _lib.TG_F16
    raise RuntimeError(f"theatergen_amd: unsupported activation dtype {t.dtype} (bf16 / fp16 only)")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _need_cuda(t):
    if not t.is_cuda:
        raise RuntimeError("theatergen_amd: tensors must live on the GPU (no CPU fallback)")


_ws_slot = 0


class workspace_slot:
    """Kernels launched inside this context take their scratch (GroupNorm partial sums, K-split partial tiles) from slot
    ``slot``: denoising chains that run CONCURRENTLY on different streams must not share one scratch buffer."""

    def __init__(self, slot):
        self.slot = int(slot)

    def __enter__(self):
        global _ws_slot
        self._prev, _ws_slot = _ws_slot, self.slot

    def __exit__(self, *exc):
        global _ws_slot
        _ws_slot = self._prev
        return False


def workspace(nbytes, device):
    """Persistent fp32 scratch per (device, slot) (split-K partials, GroupNorm partial sums, the key-split partials of ``attention_wide``)."""
    key = (device.index, "ws", _ws_slot)
    buf = _workspaces.get(key)
    if buf is None or buf.numel() * 4 < nbytes:
        buf = torch.empty(max(int(nbytes) // 4 + 1, 1 << 20), dtype=torch.float32, device=device)
        _workspaces[key] = buf
    return buf


def gemm(a0, w, M, N, K, *, mode=0, a1=None, c0=None, c1=0, conv=None, bias=None, bvec=None, rows_per_batch=0,
         res=None, act=ACT_NONE, out_scale=1.0, out=None, n_split=0, out_t=None, ldt=0, force_split_k=0, force_tile=0,
         a_rows_per_batch=0, a_batch_stride=0, geglu=False, pad_mode=0, a_coef=None, a_silu=False, plan_only=False, ln=None, lda=0, ldw=0,
         gn_out=None, pair_out=None):
    """out[M, N] = epilogue(A[M, K] @ W[N, K]^T); see tg_gemm in include/theatergen_hip.h.
    ``conv`` = (batch, in_h, in_w, out_h, out_w, stride, upsample) for mode 1.
    ``pair_out`` (dense [2 M, N]): the result goes to its rows [0, M) and, by one ``dup_rows`` copy, to [M, 2 M) (no tg_gemm kernel stores twice: the
    slab conv has no registers to spare for it); returns ``pair_out[:M]``."""
    _need_cuda(a0)
    if pair_out is not None:
        if out is not None or n_split > 0 or geglu or pair_out.shape != (2 * M, N) or not pair_out.is_contiguous() or pair_out.dtype != a0.dtype:
            raise RuntimeError("gemm: pair_out must be the only output, a dense [2 M, N] tensor of the activation dtype")
        out = pair_out[:M]
    L = _lib.lib()
    d = GemmDesc()
    d.dtype = _dt(a0)
    d.mode = mode
    d.a0, d.a1 = _ptr(a0), _ptr(a1)
    d.c0 = int(c0 if c0 is not None else (K if mode == 0 else K // 9))
    d.c1 = int(c1)
    if conv is not None:
        d.batch, d.in_h, d.in_w, d.out_h, d.out_w, d.stride, d.upsample = [int(v) for v in conv]
    d.w = _ptr(w)
    d.M, d.N, d.K = int(M), int(N), int(K)
    d.bias = _ptr(bias)
    d.bvec = _ptr(bvec)
    d.ldbvec = int(bvec.stride(0)) if bvec is not None else 0
    d.rows_per_batch = int(rows_per_batch)
    d.res = _ptr(res)
    d.ldres = int(res.stride(0)) if res is not None else 0
    d.act = act
    d.geglu = 1 if geglu else 0
    d.out_scale = float(out_scale)
    n_main = n_split if n_split > 0 else (N // 2 if geglu else N)
    if out is None:
        out = torch.empty((M, n_main), dtype=a0.dtype, device=a0.device)
    d.out = _ptr(out)
    d.ldc = int(out.stride(0))
    d.n_split = int(n_split)
    d.out_t = _ptr(out_t)
    d.ldt = int(ldt)
    d.force_split_k = force_split_k
    d.force_tile = force_tile
    d.a_rows_per_batch, d.a_batch_stride = int(a_rows_per_batch), int(a_batch_stride)
    d.pad_mode = int(pad_mode)
    d.a_coef = _ptr(a_coef)
    d.a_silu = 1 if a_silu else 0
    d.lda, d.ldw = int(lda), int(ldw)                    # row pitches of A / W when the caller padded them (plain single-source GEMM only; 0 = K)
    if ln is not None:                  # (u fp32 [N], v fp32 [N], eps[, rows]): LayerNorm of the A rows folded into this GEMM (``pack_ln_linear``);
        d.ln_u, d.ln_v, d.ln_eps = _ptr(ln[0]), _ptr(ln[1]), float(ln[2])     # rows = ``layernorm_stats`` output, None: taken inside the kernel
        if len(ln) > 3 and ln[3] is not None:
            if ln[3].dtype != torch.float32 or ln[3].numel() != 2 * M or not ln[3].is_contiguous():
                raise RuntimeError("gemm: ln rows must be the contiguous fp32 [M, 2] tensor of layernorm_stats")
            d.ln_rows = _ptr(ln[3])
    if gn_out is not None and not plan_only:
        # gn_out = {"groups": G}: GroupNorm(G) partial sums of the OUTPUT from the epilogue where the planner's kernel writes them (the two-wave slab conv,
        # unsplit); filled in with "partials" (fp32 [batch, nblk, G, 2]) and "nblk" for ``groupnorm_from_partials``; left alone otherwise.
        d.out_gn_groups = int(gn_out["groups"])
        nb = L.tg_gemm_gn_partial_blocks(C.byref(d))
        if nb > 0:
            gn_out["partials"] = torch.empty((int(conv[0]), nb, d.out_gn_groups, 2), dtype=torch.float32, device=a0.device)
            gn_out["nblk"] = nb
            d.out_gn_partials = gn_out["partials"].data_ptr()
        else:
            d.out_gn_groups = 0
    if plan_only:
        tm, tn, sp, kk = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        _lib.check(L.tg_gemm_plan(C.byref(d), C.byref(tm), C.byref(tn), C.byref(sp), C.byref(kk)))
        return tm.value, tn.value, sp.value, kk.value
    need = L.tg_gemm_workspace_bytes(C.byref(d))
    if need < 0:
        _lib.check(-1)
    if need > 0:
        ws = workspace(need, a0.device)
        d.workspace = ws.data_ptr()
        d.workspace_bytes = ws.numel() * 4
    def launch():
        _lib.check(L.tg_gemm(C.byref(d), _stream()))
        if pair_out is not None:
            dup_rows(out, pair_out[M:])
    if _gemm_profile is None:
        launch()
        return out
    # profiling mode (bench.py roofline leg): HIP events on the launch stream around this one launch
    tm, tn, sp, kk = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    _lib.check(L.tg_gemm_plan(C.byref(d), C.byref(tm), C.byref(tn), C.byref(sp), C.byref(kk)))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    launch()
    e1.record()
    # label = the kernel template the planner names + the variant / tile as the profiles have always spelled them (bench.py groups by these strings)
    variant = {0: "plain,", 1: "conv,", 6: "plain+ln,"}.get(kk.value, "")
    tail = ((",geglu" if geglu else "") + (",ln" if ln is not None else "")) if kk.value == 7 else ""
    kname = f"{L.tg_gemm_kernel_name(C.byref(d)).decode()}<{variant}{tm.value}x{tn.value}{tail}>" + ("+gn" if kk.value == 4 and a_coef is not None else "")
    _gemm_profile.append(dict(kernel=kname, splits=sp.value,
                              M=int(M), N=int(N), K=int(K), flops=2.0 * M * N * K, events=(e0, e1),
                              has_res=res is not None, n_out=int(n_main if n_split <= 0 else N)))
    return out


_gemm_profile = None


def _profiled(launch, kernel, M, N, K, flops, has_res=False, alg_bytes=None):
    """run ``launch()``; in profiling mode (bench.py roofline leg) bracket it with HIP events on the launch stream and record it"""
    if _gemm_profile is None:
        launch()
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    launch()
    e1.record()
    _gemm_profile.append(dict(kernel=kernel, splits=1, M=int(M), N=int(N), K=int(K), flops=float(flops), events=(e0, e1),
                              has_res=bool(has_res), n_out=int(N), **({"alg_bytes": float(alg_bytes)} if alg_bytes is not None else {})))


def gemm_profile_start():
    global _gemm_profile
    _gemm_profile = []


def gemm_profile_stop():
    """-> list of per-launch records with ``ms`` filled in (call after torch.cuda.synchronize())."""
    global _gemm_profile
    recs, _gemm_profile = _gemm_profile, None
    for r in recs or []:
        e0, e1 = r.pop("events")
        r["ms"] = e0.elapsed_time(e1)
    return recs or []


def linear(x, w, bias=None, **kw):
    """x [rows, K] (row pitch = K) @ w[N, K]^T"""
    M, K = x.shape
    N = w.shape[0]
    if x.stride(0) != K or w.shape[1] != K or w.stride(0) != K:
        # padded row pitches (round 5: the FeedForward hidden tensor and its packed net.2 weight): views [:, :K] of wider buffers
        assert x.stride(1) == 1 and w.stride(1) == 1 and w.shape[1] == K and x.stride(0) >= K and w.stride(0) >= K
        return gemm(x, w, M, N, K, bias=bias, lda=x.stride(0), ldw=w.stride(0), **kw)
    return gemm(x, w, M, N, K, bias=bias, **kw)


def dup_rows(src, dst):
    """dst (dense [rows, cols]) = src ([rows, cols], any row pitch): ``tg_dup_rows``, the copy behind ``pair_out`` where a producer cannot store twice"""
    _need_cuda(src)
    rows, cols = src.shape
    if src.stride(1) != 1 or dst.shape != src.shape or not dst.is_contiguous() or dst.dtype != src.dtype:
        raise RuntimeError("dup_rows: src [rows, cols] with unit column stride, dst a dense tensor of the same shape and dtype")
    _lib.check(_lib.lib().tg_dup_rows(_ptr(src), _ptr(dst), int(rows), int(cols), int(src.stride(0)), _dt(src), _stream()))
    return dst


def rc_linear(x, wpk, N, *, res=None, ln_eps=None, out=None, pair_out=None, _reserved=0):
    """Row-chain projection (csrc/tg_rowchain.hip): out = [LayerNorm-folded] x @ W^T + v (+ res) with the token rows in registers;
    ``wpk`` = ``weights_pack.rc_pack(W, v, u)`` (uint8 chunk stream), x [M, 320].  ``pair_out`` (dense [2 M, N]): both halves receive the
    result from the kernel's epilogue (``tg_rc_linear_dup``); returns ``pair_out[:M]``.  ``_reserved``: the descriptor's reserved word (the entry refuses
    anything but 0; the refusal test sets it)."""
    from ._lib import RcLinearDesc
    _need_cuda(x)
    M, K = x.shape
    if pair_out is not None:
        if out is not None or pair_out.shape != (2 * M, N) or not pair_out.is_contiguous() or pair_out.dtype != x.dtype:
            raise RuntimeError("rc_linear: pair_out must be the only output, a dense [2 M, N] tensor of the activation dtype")
        out = pair_out[:M]
    dup = int(M) * int(N) if pair_out is not None else 0
    assert x.stride(1) == 1 and wpk.dtype == torch.uint8
    if K != 320:
        raise RuntimeError(f"rc_linear: K = {K} (the row-chain projection keeps a 320-channel token row in registers)")
    assert wpk.numel() == (N // 64) * (128 * K + 1024), (wpk.numel(), N, K)
    if out is None:
        out = torch.empty(M, N, dtype=x.dtype, device=x.device)
    d = RcLinearDesc()
    d.dtype = _dt(x)
    d.x, d.ldx, d.wpk = _ptr(x), int(x.stride(0)), _ptr(wpk)
    d.res, d.ldres = (_ptr(res), int(res.stride(0))) if res is not None else (None, 0)
    d.out, d.ldc = _ptr(out), int(out.stride(0))
    d.M, d.N, d.K = int(M), int(N), int(K)
    d.ln, d.ln_eps = (1, float(ln_eps)) if ln_eps is not None else (0, 0.0)
    d.variant = int(_reserved)
    _profiled(lambda: _lib.check(_lib.lib().tg_rc_linear_dup(C.byref(d), dup, _stream()) if dup else _lib.lib().tg_rc_linear(C.byref(d), _stream())),
              "rc_linear_kernel<320>" + ("+ln" if ln_eps is not None else ""),
              M, N, K, 2.0 * M * N * K, res is not None)
    return out


def rc_kv_pack(k, vt, ldt, L, kip, vtip, ldi, T, batch, out=None):
    """text K [batch * L, 320] / V^T [batch, 320, ldt] (+ image K / V^T) -> the fragment blocks ``rc_xattn`` streams: uint8-free view
    [batch, 8, 24 * 512] of the storage dtype"""
    _need_cuda(k)
    if out is None:
        out = torch.empty((batch, 8, 24 * 512), dtype=k.dtype, device=k.device)
    _lib.check(_lib.lib().tg_rc_kv_pack(_dt(k), int(batch), _ptr(k), _ptr(vt), int(ldt), int(L), _ptr(kip), _ptr(vtip), int(ldi), int(T),
                                       _ptr(out), _stream()))
    return out


def xq_kv_pack(k, vt, ldt, L, kip, vtip, ldi, T, batch, C_, head_dim, out=None):
    """text K [batch * L, C] / V^T [batch, C, ldt] (+ image K / V^T) -> the MFMA fragments ``xq_attn`` streams (uint8 blob; tg_xq_kv_pack)"""
    _need_cuda(k)
    need = _lib.lib().tg_xq_kv_bytes(int(batch), int(C_), int(head_dim))
    if need < 0:
        raise RuntimeError(f"xq_kv_pack: C = {C_}, head_dim = {head_dim} not supported")
    if out is None:
        out = torch.empty(need, dtype=torch.uint8, device=k.device)
    assert out.numel() == need and out.dtype == torch.uint8
    _lib.check(_lib.lib().tg_xq_kv_pack(_dt(k), int(batch), int(C_), int(head_dim), _ptr(k), _ptr(vt), int(ldt), int(L), _ptr(kip), _ptr(vtip),
                                       int(ldi), int(T), _ptr(out), _stream()))
    return out


def _ip_scale_count(ip_scale, batch, who):
    """Element count of a device IP scale: 1 (one value for the launch) or ``batch`` (one per batch item); anything else is refused here, before the library."""
    if ip_scale is None:
        return 0
    if ip_scale.dtype != torch.float32 or not ip_scale.is_cuda or not ip_scale.is_contiguous():
        raise RuntimeError(f"{who}: the IP scale must be a contiguous fp32 device tensor")
    n = int(ip_scale.numel())
    if n != 1 and n != int(batch):
        raise RuntimeError(f"{who}: the IP scale has {n} elements, the launch takes 1 or its batch ({int(batch)})")
    return n


def xq_attn(x, wq, ln_u, ln_v, ln_eps, kv, head_dim, rows_per_batch, text_len, ip_tokens, ip_scale=None, out=None):
    """norm2 + attn2.to_q + (decoupled text + image) cross-attention of an inner-level block in one launch -> O [M, C]; see tg_xq_attn.
    ``ip_scale``: fp32 device tensor of 1 element or of M / rows_per_batch (one per batch item: tg_xq_attn_ps)."""
    from ._lib import XqAttnDesc
    _need_cuda(x)
    M, Cc = x.shape
    n_ips = _ip_scale_count(ip_scale, M // max(int(rows_per_batch), 1), "xq_attn")
    assert x.stride(1) == 1 and x.stride(0) == Cc and wq.shape == (Cc, Cc)
    if out is None:
        out = torch.empty(M, Cc, dtype=x.dtype, device=x.device)
    d = XqAttnDesc()
    d.dtype = _dt(x)
    d.x, d.ldx, d.wq = _ptr(x), int(x.stride(0)), _ptr(wq)
    d.ln_u, d.ln_v, d.ln_eps = _ptr(ln_u), _ptr(ln_v), float(ln_eps)
    d.kv, d.ip_scale = _ptr(kv), _ptr(ip_scale)
    d.out, d.ldc = _ptr(out), int(out.stride(0))
    d.M, d.C, d.head_dim, d.rows_per_batch, d.text_len, d.ip_tokens = int(M), int(Cc), int(head_dim), int(rows_per_batch), int(text_len), int(ip_tokens)
    L_ = text_len + ip_tokens
    # algorithmic count: to_q + QK^T + PV on the live keys.  It does not depend on the tile (head dim 64: 128 x 128 tiles whose two heads fill every O^T
    # block; 80: 128 x 160 with a shared block) — the padded key slots and zero rows a tile multiplies are not counted as work
    flops = 2.0 * M * Cc * Cc + 4.0 * M * L_ * Cc
    tile = "128x128" if int(head_dim) == 64 else "128x160"
    launch = ((lambda: _lib.check(_lib.lib().tg_xq_attn_ps(C.byref(d), n_ips, _stream()))) if n_ips > 1 else
              (lambda: _lib.check(_lib.lib().tg_xq_attn(C.byref(d), _stream()))))
    _profiled(launch, f"gemm_glds_kernel<plain+ln+xattn d{head_dim},{tile}>", M, Cc, Cc, flops,
              alg_bytes=2.0 * (2 * M * Cc + Cc * Cc) + 2.0 * (M // rows_per_batch) * 2 * L_ * Cc)
    return out


def rc_xattn(h, wq, kv, wo, rows_per_batch, ln_eps, ip_tokens, ip_scale=None, out=None, text_len=77):
    """norm2 + cross-attention (+ decoupled image keys) + to_out + residual in one launch; see tg_rc_xattn.
    ``ip_scale``: fp32 device tensor of 1 element or of M / rows_per_batch (one per batch item: tg_rc_xattn_ps)."""
    from ._lib import RcXattnDesc
    _need_cuda(h)
    M, Cc = h.shape
    n_ips = _ip_scale_count(ip_scale, M // max(int(rows_per_batch), 1), "rc_xattn")
    assert Cc == 320 and h.stride(1) == 1
    if out is None:
        out = torch.empty(M, 320, dtype=h.dtype, device=h.device)
    d = RcXattnDesc()
    d.dtype = _dt(h)
    d.h, d.ldh = _ptr(h), int(h.stride(0))
    d.wq, d.kv, d.wo = _ptr(wq), _ptr(kv), _ptr(wo)
    d.out, d.ldc = _ptr(out), int(out.stride(0))
    d.M, d.rows_per_batch = int(M), int(rows_per_batch)
    d.text_len, d.ip_tokens = int(text_len), int(ip_tokens)
    d.ln_eps = float(ln_eps)
    d.ip_scale = _ptr(ip_scale)
    # algorithmic work: to_q + to_out (2 x 2 M 320^2) + scores and PV over the real keys (4 M 320 (L + T))
    launch = ((lambda: _lib.check(_lib.lib().tg_rc_xattn_ps(C.byref(d), n_ips, _stream()))) if n_ips > 1 else
              (lambda: _lib.check(_lib.lib().tg_rc_xattn(C.byref(d), _stream()))))
    _profiled(launch, f"rc_xattn_kernel<77+{int(ip_tokens)}>",
              M, 320, 320, 4.0 * M * 320 * 320 + 4.0 * M * 320 * (int(text_len) + int(ip_tokens)), True,
              alg_bytes=2.0 * (3 * M * 320 + 2 * 320 * 320) + 2.0 * kv.numel())     # rows in, residual re-read, rows out; to_q, to_out; K / V^T fragments
    return out


def rc_ff(h, w1, w2, b2, inner, ln_eps, wpo=None, res0=None, out=None, _reserved=0):
    """norm3 + GEGLU feed-forward + residual (+ proj_out + its residual) in one launch; see tg_rc_ff.  The streams are ``rowchain.pack_ff2`` /
    ``pack_po2`` and the launch is ``rc_ff2_kernel`` (two waves per SIMD).  ``_reserved``: as in ``rc_linear``"""
    from ._lib import RcFfDesc
    _need_cuda(h)
    M, Cc = h.shape
    assert Cc == 320 and h.stride(1) == 1
    if out is None:
        out = torch.empty(M, 320, dtype=h.dtype, device=h.device)
    d = RcFfDesc()
    d.dtype = _dt(h)
    d.h, d.ldh = _ptr(h), int(h.stride(0))
    d.w1, d.w2, d.b2, d.wpo = _ptr(w1), _ptr(w2), _ptr(b2), _ptr(wpo)
    d.res0, d.ldres = (_ptr(res0), int(res0.stride(0))) if res0 is not None else (None, 0)
    d.out, d.ldc = _ptr(out), int(out.stride(0))
    d.M, d.inner, d.ln_eps, d.dbg = int(M), int(inner), float(ln_eps), int(_reserved) | _lib.RC_FF_TWO_WAVE
    fl = 2.0 * M * 320 * (3 * int(inner)) + (2.0 * M * 320 * 320 if wpo is not None else 0.0)
    _profiled(lambda: _lib.check(_lib.lib().tg_rc_ff(C.byref(d), _stream())), "rc_ff2_kernel<320>" + ("+proj_out" if wpo is not None else ""),
              M, 320, 3 * int(inner), fl, True,
              alg_bytes=2.0 * ((4 if wpo is not None else 3) * M * 320 + 3 * 320 * int(inner) + (320 * 320 if wpo is not None else 0)))
    return out


def rc_front(x, coef, win, wqkv, rows_per_batch, ln_eps, y=None, qk=None, vt=None, _reserved=0):
    """GroupNorm (coefficients) + proj_in + LayerNorm1 + q | k | v in one launch; see tg_rc_front.  Returns (y, qk, vt, ldt).  ``_reserved``: as in ``rc_linear``"""
    from ._lib import RcFrontDesc
    _need_cuda(x)
    M, Cc = x.shape
    assert Cc == 320 and x.stride(1) == 1 and coef.dtype == torch.float32
    B = M // rows_per_batch
    ldt = (rows_per_batch + 7) // 8 * 8
    if y is None:
        y = torch.empty(M, 320, dtype=x.dtype, device=x.device)
    if qk is None:
        qk = torch.empty(M, 640, dtype=x.dtype, device=x.device)
    if vt is None:
        vt = torch.empty(B, 320, ldt, dtype=x.dtype, device=x.device)
    d = RcFrontDesc()
    d.dtype = _dt(x)
    d.x, d.ldx, d.coef, d.win, d.wqkv = _ptr(x), int(x.stride(0)), _ptr(coef), _ptr(win), _ptr(wqkv)
    d.y, d.ldy, d.qk, d.ldqk, d.vt, d.ldt = _ptr(y), int(y.stride(0)), _ptr(qk), int(qk.stride(0)), _ptr(vt), int(vt.stride(1))
    d.M, d.rows_per_batch, d.ln_eps, d.dbg = int(M), int(rows_per_batch), float(ln_eps), int(_reserved)
    fl = 2.0 * M * 320 * (320 + 960)
    _profiled(lambda: _lib.check(_lib.lib().tg_rc_front(C.byref(d), _stream())), "rc_front_kernel<320>", M, 960, 320, fl, False,
              alg_bytes=2.0 * (5 * M * 320 + 4 * 320 * 320))
    return y, qk, vt, int(vt.stride(1))


def skinny_gemm(x, wpk, N, *, ln=None, bias=None, act=ACT_NONE, res=None, out=None, segs=None, rows_per_batch=None):
    """A handful of rows against a fragment-packed weight (``weights_pack.skinny_pack``); see tg_skinny_gemm.  ``ln`` = (u fp32 [N], v fp32 [N], eps): x is the
    un-normalised stream.  ``segs``: up to three ``(tensor_or_pointer, ld, batch_stride, n_end, transposed)`` output segments (default: one plain [M, N] tensor,
    returned).  Output pointers in ``segs`` are raw addresses (``tensor.data_ptr() + byte offset``): the caller keeps the tensors alive."""
    from ._lib import SkinnyDesc
    _need_cuda(x)
    M, K = x.shape
    assert x.stride(1) == 1 and wpk.numel() == N * K, (x.shape, wpk.numel(), N)
    d = SkinnyDesc()
    d.dtype, d.x, d.ldx, d.wpk, d.M, d.N, d.K = _dt(x), _ptr(x), int(x.stride(0)), _ptr(wpk), int(M), int(N), int(K)
    if ln is not None:
        d.ln, d.ln_u, d.ln_v, d.ln_eps = 1, _ptr(ln[0]), _ptr(ln[1]), float(ln[2])
    d.bias, d.act = _ptr(bias), int(act)
    if res is not None:
        d.res, d.ldres = _ptr(res), int(res.stride(0))
    if segs is None:
        if out is None:
            out = torch.empty(M, N, dtype=x.dtype, device=x.device)
        segs = [(out.data_ptr(), int(out.stride(0)), 0, N, 0)]
        rows_per_batch = M
    d.nseg, d.rows_per_batch = len(segs), int(rows_per_batch)
    for i, (ptr, ld, bs, n_end, tr) in enumerate(segs):
        d.seg[i].ptr, d.seg[i].ld, d.seg[i].batch_stride, d.seg[i].n_end, d.seg[i].transposed = int(ptr), int(ld), int(bs), int(n_end), int(tr)
    _lib.check(_lib.lib().tg_skinny_gemm(C.byref(d), _stream()))
    return out


def conv3x3(x, w_packed, batch, in_h, in_w, cin, *, x1=None, c1=0, stride=1, upsample=False, bias=None, pad_mode=0, **kw):
    """3x3 pad-1 convolution as implicit GEMM over token-major x [batch*in_h*in_w, cin] (+ optional concat x1).
    w_packed: [cout, 9*(cin+c1)] tap-major.  ``pad_mode=1``: zero padding on the bottom / right edge only (the VAE
    encoder's ``Downsample2D(padding=0)``: ``F.pad(x, (0, 1, 0, 1))`` then a stride-2 conv)."""
    if upsample:
        oh, ow = 2 * in_h, 2 * in_w
    else:
        pad2 = 1 if pad_mode == 1 else 2
        oh, ow = (in_h + pad2 - 3) // stride + 1, (in_w + pad2 - 3) // stride + 1
    N = w_packed.shape[0]
    K = 9 * (cin + c1)
    return gemm(x, w_packed, batch * oh * ow, N, K, mode=1, a1=x1, c0=cin, c1=c1,
                conv=(batch, in_h, in_w, oh, ow, stride, 1 if upsample else 0), bias=bias, pad_mode=pad_mode, **kw)


def _up2_desc(dtype, batch, in_h, in_w, cin, cout):
    d = GemmDesc()
    d.dtype = _lib.TG_BF16 if dtype == torch.bfloat16 else _lib.TG_F16
    d.mode, d.stride, d.upsample = 1, 1, 1
    d.c0 = int(cin)
    d.batch, d.in_h, d.in_w, d.out_h, d.out_w = int(batch), int(in_h), int(in_w), 2 * int(in_h), 2 * int(in_w)
    d.M, d.N, d.K = 4 * int(batch) * int(in_h) * int(in_w), int(cout), 16 * int(cin)
    d.out_scale = 1.0
    d.ldc = int(cout)
    return d


_up2_plans = {}


def conv_up2_eligible(dtype, batch, in_h, in_w, cin, cout):
    """True when ``conv_up2`` (tg_conv_up2: the nearest-x2 folded into four 2x2-tap convs) takes this Upsample2D layer with a contiguous output."""
    key = (dtype, batch, in_h, in_w, cin, cout)
    hit = _up2_plans.get(key)
    if hit is None:
        if dtype not in (torch.bfloat16, torch.float16):
            return False
        d = _up2_desc(dtype, batch, in_h, in_w, cin, cout)
        d.a0 = d.w = d.out = 16                      # eligibility only: pointers are not dereferenced, just non-NULL and aligned
        hit = _up2_plans[key] = bool(_lib.lib().tg_conv_up2_eligible(C.byref(d)))
    return hit


def conv_up2(x, w_folded, batch, in_h, in_w, cin, bias=None, out=None):
    """Upsample2D (nearest x2 + conv3x3 pad 1) over token-major x [batch*in_h*in_w, cin] with ``w_folded`` = ``weights_pack.pack_conv3x3_up2``
    ([4, cout, 4*cin]) -> [batch*2*in_h*2*in_w, cout]; see tg_conv_up2.  Raises where the kernel does not take the layer (no fallback here)."""
    _need_cuda(x)
    assert w_folded.dim() == 3 and w_folded.shape[0] == 4 and w_folded.shape[2] == 4 * cin and w_folded.is_contiguous(), tuple(w_folded.shape)
    assert x.stride(1) == 1 and x.stride(0) == cin and w_folded.dtype == x.dtype
    N = w_folded.shape[1]
    d = _up2_desc(x.dtype, batch, in_h, in_w, cin, N)
    if out is None:
        out = torch.empty((d.M, N), dtype=x.dtype, device=x.device)
    d.a0, d.w, d.bias, d.out, d.ldc = _ptr(x), _ptr(w_folded), _ptr(bias), _ptr(out), int(out.stride(0))
    # algorithmic work of the layer as the caller sees it (the unfolded conv), so TFLOP/s compare with the unfolded kernel's records
    _profiled(lambda: _lib.check(_lib.lib().tg_conv_up2(C.byref(d), _stream())), "conv_halo_kernel<up2,128x128>", d.M, N, 9 * cin, 2.0 * d.M * N * 9 * cin)
    return out


def _attn_desc(q, q_ld, q_bs, k0, k0_ld, k0_bs, vt0, vt0_ld, vt0_bs, len0, batch, heads, head_dim, n_q, scale, out, out_ld, out_bs):
    """AttnDesc of one unmasked softmax segment: what ``attention``, ``attention_wide`` and ``attention_relpos`` have in common"""
    d = AttnDesc()
    d.dtype = _dt(q)
    d.batch, d.heads, d.head_dim, d.n_q = int(batch), int(heads), int(head_dim), int(n_q)
    d.q, d.q_ld, d.q_bs = _ptr(q), int(q_ld), int(q_bs)
    d.k0, d.k0_ld, d.k0_bs = _ptr(k0), int(k0_ld), int(k0_bs)
    d.vt0, d.vt0_ld, d.vt0_bs = _ptr(vt0), int(vt0_ld), int(vt0_bs)
    d.len0 = int(len0)
    d.scale = float(scale)
    d.out, d.out_ld, d.out_bs = _ptr(out), int(out_ld), int(out_bs)
    return d


def attention(q, q_ld, q_bs, k0, k0_ld, k0_bs, vt0, vt0_ld, vt0_bs, len0, batch, heads, head_dim, n_q, scale,
              out, out_ld, out_bs, k1=None, k1_ld=0, k1_bs=0, vt1=None, vt1_ld=0, vt1_bs=0, len1=0, w1=0.0, causal=False, w1_dev=None,
              mask=None):
    """``w1_dev``: fp32 device tensor read by the kernel instead of the launch constant ``w1`` (graph-replayable IP scale): 1 element, or ``batch``
    elements = one weight per batch item (tg_attention_ps).
    ``mask``: additive score bias, fp32 [Bm, Hm, Qm, len0] with Bm in {1, batch}, Hm in {1, heads}, Qm in {1, n_q} (size-1 dims broadcast)."""
    _need_cuda(q)
    d = _attn_desc(q, q_ld, q_bs, k0, k0_ld, k0_bs, vt0, vt0_ld, vt0_bs, len0, batch, heads, head_dim, n_q, scale, out, out_ld, out_bs)
    d.k1, d.k1_ld, d.k1_bs = _ptr(k1), int(k1_ld), int(k1_bs)
    d.vt1, d.vt1_ld, d.vt1_bs = _ptr(vt1), int(vt1_ld), int(vt1_bs)
    d.len1 = int(len1)
    d.w1 = float(w1)
    d.causal = 1 if causal else 0
    n_w1 = 0
    if w1_dev is not None:
        if w1_dev.dtype != torch.float32 or not w1_dev.is_cuda:
            raise RuntimeError("attention: w1_dev must be an fp32 device tensor")
        n_w1 = _ip_scale_count(w1_dev, batch, "attention")
        d.w1_dev = w1_dev.data_ptr()
    if mask is not None:
        if mask.dtype != torch.float32 or not mask.is_cuda or mask.ndim != 4 or not mask.is_contiguous() or mask.shape[3] != len0:
            raise RuntimeError("attention: mask must be a contiguous fp32 device tensor [Bm, Hm, Qm, len0]")
        bm, hm, qm, _ = mask.shape
        if bm not in (1, batch) or hm not in (1, heads) or qm not in (1, n_q):
            raise RuntimeError(f"attention: mask shape {tuple(mask.shape)} does not broadcast to [{batch}, {heads}, {n_q}, {len0}]")
        d.mask = mask.data_ptr()
        d.mask_bs = hm * qm * len0 if bm > 1 else 0
        d.mask_hs = qm * len0 if hm > 1 else 0
        d.mask_qs = len0 if qm > 1 else 0
    launch = ((lambda: _lib.check(_lib.lib().tg_attention_ps(C.byref(d), n_w1, _stream()))) if n_w1 > 1 else
              (lambda: _lib.check(_lib.lib().tg_attention(C.byref(d), _stream()))))
    if _gemm_profile is None:
        launch()
        return out
    # profiling mode (bench.py roofline leg): HIP events around this launch; algorithmic flops = QK^T + PV of both segments, no padding
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    launch()
    e1.record()
    keys = int(len0) + int(len1)
    _gemm_profile.append(dict(kernel=f"attention_kernel<d{int(head_dim)},{'self' if int(len0) == int(n_q) else 'cross'}>", splits=1,
                              M=int(batch) * int(n_q), N=int(heads) * int(head_dim), K=keys,
                              flops=4.0 * batch * heads * n_q * keys * head_dim, events=(e0, e1), has_res=False,
                              n_out=int(heads) * int(head_dim), attention=True, batch=int(batch)))
    return out


def relpos_table_floats(batch, heads, grid):
    """fp32 elements of ONE of the two bias tables [batch, heads, grid^2, grid]."""
    return int(batch) * int(heads) * int(grid) ** 3


def relpos_tables(q, q_ld, q_bs, rel_pos_h, rel_pos_w, batch, heads, head_dim, grid, out=None):
    """``tg_relpos_tables``: SAM's decomposed relative-position bias as two fp32 tables ``(bh, bw)``, each [batch, heads, grid^2, grid], from the
    stored unscaled ``q`` (pitches as ``attention``) and the layer's ``rel_pos_h`` / ``rel_pos_w`` ([2 grid - 1, head_dim], the dtype of ``q``).
    ``out``: a caller pair ``(bh, bw)``; default: both halves of ``ops.workspace`` (valid until the next kernel that takes scratch from it)."""
    _need_cuda(q)
    _need_cuda(rel_pos_h)
    _need_cuda(rel_pos_w)
    want = (2 * int(grid) - 1, int(head_dim))
    for name, t in (("rel_pos_h", rel_pos_h), ("rel_pos_w", rel_pos_w)):
        if tuple(t.shape) != want or t.dtype != q.dtype or not t.is_contiguous():
            raise RuntimeError(f"relpos_tables: {name} must be a contiguous {q.dtype} tensor {want} (a table of another length would need "
                               f"interpolation, which is not done here), got {tuple(t.shape)} {t.dtype}")
    n = relpos_table_floats(batch, heads, grid)
    if out is None:
        n16 = (n + 3) // 4 * 4
        ws = workspace(2 * n16 * 4, q.device)
        bh, bw = ws[:n].view(batch, heads, grid * grid, grid), ws[n16:n16 + n].view(batch, heads, grid * grid, grid)
    else:
        bh, bw = out
        for t in (bh, bw):
            if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or t.numel() != n:
                raise RuntimeError(f"relpos_tables: out must be two contiguous fp32 device tensors of {n} elements")
    _lib.check(_lib.lib().tg_relpos_tables(_dt(q), int(batch), int(heads), int(head_dim), int(grid), _ptr(q), int(q_ld), int(q_bs),
                                           _ptr(rel_pos_h), _ptr(rel_pos_w), _ptr(bh), _ptr(bw), _stream()))
    return bh, bw


def attention_relpos(q, q_ld, q_bs, k0, k0_ld, k0_bs, vt0, vt0_ld, vt0_bs, batch, heads, head_dim, grid, scale, bh, bw, out, out_ld, out_bs):
    """``tg_attention_relpos``: one-segment flash self-attention over ``grid``^2 tokens with the separable score bias
    ``bh[b, h, i, j // grid] + bw[b, h, i, j % grid]`` (``relpos_tables``) — the argument list of ``attention`` with n_q = len0 = grid^2."""
    _need_cuda(q)
    n = relpos_table_floats(batch, heads, grid)
    for t in (bh, bw):
        _need_cuda(t)
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n:
            raise RuntimeError(f"attention_relpos: bh / bw must be contiguous fp32 device tensors of {n} elements ([batch, heads, grid^2, grid])")
    d = _attn_desc(q, q_ld, q_bs, k0, k0_ld, k0_bs, vt0, vt0_ld, vt0_bs, int(grid) ** 2, batch, heads, head_dim, int(grid) ** 2, scale, out, out_ld, out_bs)
    _lib.check(_lib.lib().tg_attention_relpos(C.byref(d), _ptr(bh), _ptr(bw), int(grid), _stream()))
    return out


def attention_swin(q, q_ld, q_bs, k, k_ld, k_bs, v, v_ld, v_bs, pad_q, pad_k, pad_v, table, batch, heads, H, W, shift, scale, out, out_ld, out_bs,
                   head_dim=32, window=7):
    """``tg_attention_swin``: Swin window attention on image-ordered tokens ``x[b, r * W + c, h * 32 + ch]`` (pitches in elements): pad to a multiple of
    7, roll by ``-shift``, 7 x 7 windows, the learned bias ``table`` [169, heads], the shift mask and their inverses are address arithmetic inside the
    kernel.  ``pad_q`` / ``pad_k`` / ``pad_v`` [heads * 32]: q / k / v of a padded token (the projection biases).  Writes the H * W real tokens of ``out``."""
    _need_cuda(q)
    hd = int(heads) * int(head_dim)
    for name, t in (("pad_q", pad_q), ("pad_k", pad_k), ("pad_v", pad_v)):
        _need_cuda(t)
        if t.dtype != q.dtype or t.numel() != hd or not t.is_contiguous():
            raise RuntimeError(f"attention_swin: {name} must be a contiguous {q.dtype} device tensor of {hd} elements, got {tuple(t.shape)} {t.dtype}")
    n, batch = int(H) * int(W), int(batch)
    for name, t, ld, bs in (("q", q, q_ld, q_bs), ("k", k, k_ld, k_bs), ("v", v, v_ld, v_bs), ("out", out, out_ld, out_bs)):
        _need_cuda(t)
        if t.dtype != q.dtype or t.device != q.device:
            raise RuntimeError(f"attention_swin: {name} must be a {q.dtype} tensor on {q.device}, got {t.dtype} on {t.device}")
        if t.stride(-1) != 1:
            raise RuntimeError(f"attention_swin: {name} must have unit stride along the channels")
        if int(ld) < hd or int(bs) < 0 or (name == "out" and batch > 1 and int(bs) < (n - 1) * int(ld) + hd):
            raise RuntimeError(f"attention_swin: {name} pitches (row {ld}, batch {bs}) do not hold {n} rows of {hd} channels per batch item without overlap")
        # the last element the kernel touches must lie inside the tensor's storage (the C entry point cannot know buffer sizes)
        need = (batch - 1) * int(bs) + (n - 1) * int(ld) + hd
        have = t.untyped_storage().nbytes() // t.element_size() - t.storage_offset()
        if n < 1 or batch < 1 or have < need:
            raise RuntimeError(f"attention_swin: {name} holds {have} elements from its first, {need} are addressed (batch {batch}, {H} x {W} tokens, "
                               f"row pitch {ld}, batch pitch {bs})")
    _need_cuda(table)
    if table.dtype != q.dtype or not table.is_contiguous() or tuple(table.shape) != ((2 * int(window) - 1) ** 2, int(heads)):
        raise RuntimeError(f"attention_swin: table must be a contiguous {q.dtype} device tensor [{(2 * int(window) - 1) ** 2}, {int(heads)}], "
                           f"got {tuple(table.shape)} {table.dtype}")
    _lib.check(_lib.lib().tg_attention_swin(_dt(q), int(batch), int(heads), int(head_dim), int(window), int(H), int(W), int(shift), float(scale),
                                            _ptr(q), int(q_ld), int(q_bs), _ptr(k), int(k_ld), int(k_bs), _ptr(v), int(v_ld), int(v_bs),
                                            _ptr(pad_q), _ptr(pad_k), _ptr(pad_v), _ptr(table), _ptr(out), int(out_ld), int(out_bs), _stream()))
    return out


def _held(t):
    """elements of ``t``'s storage from its first element on"""
    return t.untyped_storage().nbytes() // t.element_size() - t.storage_offset()


def msdeform_attn(value, v_ld, v_bs, shapes, offsets, off_ld, logits, log_ld, ref, batch, heads, n_q, out, out_ld, out_bs, value_mask=None,
                  head_dim=32, n_points=4):
    """``tg_msdeform_attn``: multi-scale deformable attention from the projected operands on (transformers' GroundingDinoMultiscaleDeformableAttention
    between its projections).  ``value`` [batch, Nv, heads * 32] (row pitch ``v_ld``, batch pitch ``v_bs``, elements), Nv = the tokens of the levels
    ``shapes`` = [(H_l, W_l), ...] concatenated; ``offsets`` rows [batch * n_q] of heads * L * 4 * 2 values (x, y in pixels of the level) and ``logits``
    rows of heads * L * 4, each with its row pitch (two column slices of one GEMM output); ``ref`` fp32 [batch, n_q, L, R], R = 2 (centres) or 4
    (boxes); ``value_mask`` uint8 [batch, Nv], 1 = padding token (samples as zeros).  Writes ``out`` [batch, n_q, heads * 32]."""
    _need_cuda(value)
    batch, heads, n_q = int(batch), int(heads), int(n_q)
    shapes = [(int(h), int(w)) for h, w in shapes]
    L = len(shapes)
    nv = sum(h * w for h, w in shapes)
    hd = heads * int(head_dim)
    if batch < 1 or heads < 1 or n_q < 1 or nv < 1 or any(h < 1 or w < 1 for h, w in shapes):
        raise RuntimeError(f"msdeform_attn: empty problem (batch {batch}, heads {heads}, n_q {n_q}, levels {shapes})")
    _f32_dev(ref, "msdeform_attn: ref")
    if ref.ndim != 4 or tuple(ref.shape[:3]) != (batch, n_q, L):
        raise RuntimeError(f"msdeform_attn: ref must be [{batch}, {n_q}, {L}, 2 or 4], got {tuple(ref.shape)}")
    R = int(ref.shape[3])
    for name, t, rows, ld, bs, cols in (("value", value, nv, v_ld, v_bs, hd), ("out", out, n_q, out_ld, out_bs, hd),
                                        ("offsets", offsets, batch * n_q, off_ld, None, heads * L * int(n_points) * 2),
                                        ("logits", logits, batch * n_q, log_ld, None, heads * L * int(n_points))):
        _need_cuda(t)
        if t.dtype != value.dtype or t.device != value.device:
            raise RuntimeError(f"msdeform_attn: {name} must be a {value.dtype} tensor on {value.device}, got {t.dtype} on {t.device}")
        if t.stride(-1) != 1:
            raise RuntimeError(f"msdeform_attn: {name} must have unit stride along the channels")
        if int(ld) < cols or (bs is not None and (int(bs) < 0 or (name == "out" and batch > 1 and int(bs) < (rows - 1) * int(ld) + cols))):
            raise RuntimeError(f"msdeform_attn: {name} pitches (row {ld}, batch {bs}) do not hold {rows} rows of {cols} channels without overlap")
        # the last element the kernel touches must lie inside the tensor's storage (the C entry point cannot know buffer sizes)
        need = ((batch - 1) * int(bs) if bs is not None else 0) + (rows - 1) * int(ld) + cols
        if _held(t) < need:
            raise RuntimeError(f"msdeform_attn: {name} holds {_held(t)} elements from its first, {need} are addressed ({rows} rows, row pitch {ld}, "
                               f"batch {batch}, batch pitch {bs})")
    if value_mask is not None:
        _need_cuda(value_mask)
        if value_mask.dtype != torch.uint8 or not value_mask.is_contiguous() or value_mask.numel() != batch * nv or value_mask.device != value.device:
            raise RuntimeError(f"msdeform_attn: value_mask must be a contiguous uint8 tensor [{batch}, {nv}] on {value.device}, "
                               f"got {tuple(value_mask.shape)} {value_mask.dtype}")
    sh = (C.c_int32 * (2 * L))(*[v for hw in shapes for v in hw])
    _lib.check(_lib.lib().tg_msdeform_attn(_dt(value), batch, heads, int(head_dim), L, int(n_points), n_q, R, sh, _ptr(value), int(v_ld), int(v_bs),
                                           _ptr(offsets), int(off_ld), _ptr(logits), int(log_ld), _ptr(ref), _ptr(value_mask), _ptr(out),
                                           int(out_ld), int(out_bs), _stream()))
    return out


def dino_contrastive(q, text, token_mask, max_text_len, logits=True, row_max=False):
    """``tg_dino_contrastive``: transformers' GroundingDinoContrastiveEmbedding.  ``q`` [batch, n, d] and ``text`` [batch, Lt, d] in the storage dtype, unit
    stride along d, any row / batch pitch that is a multiple of 8 (views of wider buffers are taken as they are); ``token_mask`` [batch, Lt] bool / uint8,
    1 = real token.  ``logits`` / ``row_max``: True allocates, a tensor is written, False / None leaves the output out; at least one.
    -> (logits fp32 [batch, n, max_text_len] or None, row_max fp32 [batch, n] or None).  The arguments are checked before the device is."""
    for name, t in (("q", q), ("text", text)):
        if not torch.is_tensor(t) or t.ndim != 3 or t.stride(2) != 1:
            raise RuntimeError(f"dino_contrastive: {name} must be a [batch, rows, d] tensor with unit stride along d")
    dt = _dt(q)
    B, n, d = (int(v) for v in q.shape)
    Lt, mtl = int(text.shape[1]), int(max_text_len)
    if text.dtype != q.dtype or text.device != q.device or text.shape[0] != B or text.shape[2] != d:
        raise RuntimeError(f"dino_contrastive: text {tuple(text.shape)} {text.dtype} does not match q {tuple(q.shape)} {q.dtype}")
    if B < 1 or n < 1:
        raise RuntimeError(f"dino_contrastive: empty problem (batch {B}, n {n})")
    if d not in (128, 256):
        raise RuntimeError(f"dino_contrastive: d = {d} unsupported (128 or 256)")
    if not 1 <= Lt <= mtl <= 256:
        raise RuntimeError(f"dino_contrastive: text_len {Lt} / max_text_len {mtl} unsupported (1 <= text_len <= max_text_len <= 256)")
    if tuple(token_mask.shape) != (B, Lt) or token_mask.dtype not in (torch.bool, torch.uint8) or token_mask.device != q.device:
        raise RuntimeError(f"dino_contrastive: token_mask must be a bool / uint8 tensor [{B}, {Lt}] on {q.device}, got {tuple(token_mask.shape)} "
                           f"{token_mask.dtype}")
    for name, t in (("q", q), ("text", text)):
        if t.stride(1) % 8 or t.stride(1) < d or (B > 1 and (t.stride(0) % 8 or t.stride(0) < 0)) or t.data_ptr() % 16:
            raise RuntimeError(f"dino_contrastive: {name} pitches (row {t.stride(1)}, batch {t.stride(0)}) must be multiples of 8 covering d, its base "
                               "16-byte aligned")
    if (logits is None or logits is False) and (row_max is None or row_max is False):
        raise RuntimeError("dino_contrastive: neither logits nor row_max asked for")
    outs = []
    for name, o, shape in (("logits", logits, (B, n, mtl)), ("row_max", row_max, (B, n))):
        if o is None or o is False:
            outs.append(None)
        elif o is True:
            outs.append(torch.empty(shape, dtype=torch.float32, device=q.device))
        else:
            if not torch.is_tensor(o) or o.dtype != torch.float32 or tuple(o.shape) != shape or not o.is_contiguous() or o.device != q.device:
                raise RuntimeError(f"dino_contrastive: {name} must be a contiguous fp32 tensor {shape} on {q.device}")
            outs.append(o)
    _need_cuda(q)
    mask = token_mask.to(torch.uint8).contiguous() if token_mask.dtype != torch.uint8 or not token_mask.is_contiguous() else token_mask
    _lib.check(_lib.lib().tg_dino_contrastive(dt, B, n, d, Lt, mtl, _ptr(q), int(q.stride(1)), int(q.stride(0)), _ptr(text), int(text.stride(1)),
                                              int(text.stride(0)), _ptr(mask), _ptr(outs[0]), _ptr(outs[1]), _stream()))
    return outs[0], outs[1]


def dino_box_update(h, w3, b3, prior, prior_is_box, rows_per_batch=None, valid_ratios=None, ref=None, ref_levels=False, pos_in=False):
    """``tg_dino_box_update``: ``h`` [rows, d] storage dtype (unit stride along d; the box MLP's second layer after ReLU), ``w3`` [4, d] storage dtype, ``b3``
    fp32 [4], ``prior`` fp32 [rows, 4] — logits (``prior_is_box`` False, +inf allowed) or boxes whose logit(eps = 1e-5) the kernel takes (True);
    ``valid_ratios`` fp32 [batch, L, 2] with rows = batch * ``rows_per_batch``.  ``ref_levels`` / ``pos_in``: True allocates, a tensor is written, False
    leaves it out.  -> (ref fp32 [rows, 4], ref_levels fp32 [rows, L, 4] or None, pos_in [rows, 2 d] storage dtype or None).  The arguments are checked
    before the device is."""
    if not torch.is_tensor(h) or h.ndim != 2 or h.stride(1) != 1:
        raise RuntimeError("dino_box_update: h must be a [rows, d] tensor with unit stride along d")
    dt = _dt(h)
    rows, d = int(h.shape[0]), int(h.shape[1])
    dev = h.device
    if rows < 1:
        raise RuntimeError("dino_box_update: empty problem (rows 0)")
    if d not in (128, 256):
        raise RuntimeError(f"dino_box_update: d = {d} unsupported (128 or 256)")
    if h.stride(0) < d:
        raise RuntimeError(f"dino_box_update: h row pitch {h.stride(0)} does not cover d = {d}")
    if w3.dtype != h.dtype or tuple(w3.shape) != (4, d) or not w3.is_contiguous() or w3.device != dev:
        raise RuntimeError(f"dino_box_update: w3 must be a contiguous {h.dtype} tensor [4, {d}] on {dev}, got {tuple(w3.shape)} {w3.dtype}")

    def f32(t, shape, what):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
            raise RuntimeError(f"dino_box_update: {what} must be a contiguous fp32 tensor {shape} on {dev}")
    f32(b3, (4,), "b3")
    f32(prior, (rows, 4), "prior")
    if prior.data_ptr() % 16:
        raise RuntimeError("dino_box_update: prior must be 16-byte aligned")
    want_levels, want_pos = ref_levels is not None and ref_levels is not False, pos_in is not None and pos_in is not False
    L = 0
    rpb = rows if rows_per_batch is None else int(rows_per_batch)
    if rpb < 1 or rows % rpb:
        raise RuntimeError(f"dino_box_update: rows = {rows} must be a multiple of rows_per_batch = {rpb}")
    if want_levels or want_pos:
        if valid_ratios is None:
            raise RuntimeError("dino_box_update: ref_levels / pos_in need valid_ratios")
        if not torch.is_tensor(valid_ratios) or valid_ratios.ndim != 3 or not 1 <= int(valid_ratios.shape[1]) <= 4:
            raise RuntimeError("dino_box_update: valid_ratios must be [batch, L, 2] with 1 <= L <= 4")
        L = int(valid_ratios.shape[1])
        f32(valid_ratios, (rows // rpb, L, 2), "valid_ratios")
    if ref is None:
        ref = torch.empty((rows, 4), dtype=torch.float32, device=dev)
    else:
        f32(ref, (rows, 4), "ref")
    if ref_levels is True:
        ref_levels = torch.empty((rows, L, 4), dtype=torch.float32, device=dev)
    elif want_levels:
        f32(ref_levels, (rows, L, 4), "ref_levels")
    else:
        ref_levels = None
    if pos_in is True:
        pos_in = torch.empty((rows, 2 * d), dtype=h.dtype, device=dev)
    elif want_pos:
        if not torch.is_tensor(pos_in) or pos_in.dtype != h.dtype or tuple(pos_in.shape) != (rows, 2 * d) or pos_in.stride(1) != 1 or \
                pos_in.stride(0) < 2 * d or pos_in.device != dev:
            raise RuntimeError(f"dino_box_update: pos_in must be a {h.dtype} tensor [{rows}, {2 * d}] on {dev} with unit stride along the channels")
    else:
        pos_in = None
    _need_cuda(h)
    _lib.check(_lib.lib().tg_dino_box_update(dt, rows, rpb, d, _ptr(h), int(h.stride(0)), _ptr(w3), _ptr(b3), _ptr(prior), 1 if prior_is_box else 0,
                                             _ptr(valid_ratios) if L else None, L, _ptr(ref), _ptr(ref_levels), _ptr(pos_in),
                                             int(pos_in.stride(0)) if pos_in is not None else 0, _stream()))
    return ref, ref_levels, pos_in


def _f32_dev(t, what, numel=None):
    _need_cuda(t)
    if t.dtype != torch.float32 or not t.is_contiguous() or (numel is not None and t.numel() != numel):
        raise RuntimeError(f"{what} must be a contiguous fp32 device tensor" + (f" of {numel} elements" if numel is not None else "") +
                           f", got {tuple(t.shape)} {t.dtype}")


def sam_posenc(coords, gauss, labels=None, table=None, dtype=torch.float32, out=None):
    """``tg_sam_posenc``: coords fp32 [n, 2] (x, y in units of the input size), gauss fp32 [2, F] -> [n, 2F] = [sin | cos](2 pi (2 c - 1) gauss) as ``dtype``
    (fp32, bf16 or fp16), all arithmetic in fp32.  ``labels`` int32 [n] + ``table`` fp32 [5, 2F] (point_embed[0..3], not_a_point_embed): label >= 0 adds its
    row, label -1 replaces the encoding by row 4."""
    _f32_dev(coords, "sam_posenc: coords")
    _f32_dev(gauss, "sam_posenc: gauss")
    if coords.ndim != 2 or coords.shape[1] != 2 or gauss.ndim != 2 or gauss.shape[0] != 2:
        raise RuntimeError(f"sam_posenc: coords [n, 2] and gauss [2, F] expected, got {tuple(coords.shape)} and {tuple(gauss.shape)}")
    n, F_ = int(coords.shape[0]), int(gauss.shape[1])
    if (labels is None) != (table is None):
        raise RuntimeError("sam_posenc: labels and table come together")
    if labels is not None:
        _need_cuda(labels)
        if labels.dtype != torch.int32 or not labels.is_contiguous() or labels.numel() != n:
            raise RuntimeError(f"sam_posenc: labels must be a contiguous int32 device tensor of {n} elements")
        _f32_dev(table, "sam_posenc: table", 5 * 2 * F_)
    code = 2 if dtype == torch.float32 else _lib.TG_BF16 if dtype == torch.bfloat16 else _lib.TG_F16 if dtype == torch.float16 else None
    if code is None:
        raise RuntimeError(f"sam_posenc: output dtype {dtype} unsupported (fp32, bf16, fp16)")
    if out is None:
        out = torch.empty((n, 2 * F_), dtype=dtype, device=coords.device)
    elif out.dtype != dtype or not out.is_cuda or not out.is_contiguous() or out.numel() != n * 2 * F_:
        raise RuntimeError(f"sam_posenc: out must be a contiguous {dtype} device tensor [{n}, {2 * F_}]")
    _lib.check(_lib.lib().tg_sam_posenc(code, _ptr(coords), n, _ptr(gauss), F_, _ptr(labels), _ptr(table), _ptr(out), _stream()))
    return out


def sam_mask_head(x, images, g, w1, w2, vec, hyper_in, eps=1e-6, out=None):
    """``tg_sam_mask_head``: image tokens x [images * g * g, 256] -> fp32 low-resolution logits [images, M, 4g, 4g] (upscale_conv1, LayerNorm, GELU,
    upscale_conv2, GELU, product with ``hyper_in`` [images, M, 32]) in one launch.  ``w1, w2, vec = weights_pack.pack_sam_upscale(...)``."""
    _need_cuda(x)
    for t in (w1, w2, hyper_in):
        _need_cuda(t)
        if t.dtype != x.dtype or not t.is_contiguous():
            raise RuntimeError(f"sam_mask_head: w1, w2 and hyper_in must be contiguous {x.dtype} device tensors")
    images, g = int(images), int(g)
    if x.ndim != 2 or tuple(x.shape) != (images * g * g, 256) or not x.is_contiguous():
        raise RuntimeError(f"sam_mask_head: x must be contiguous [{images * g * g}, 256], got {tuple(x.shape)}")
    if hyper_in.ndim != 3 or hyper_in.shape[0] != images or hyper_in.shape[2] != 32:
        raise RuntimeError(f"sam_mask_head: hyper_in must be [{images}, M, 32], got {tuple(hyper_in.shape)}")
    if w1.numel() != 4 * 64 * 256 or w2.numel() != 4 * 32 * 64:
        raise RuntimeError("sam_mask_head: w1 / w2 are not weights_pack.pack_sam_upscale's fragments")
    _f32_dev(vec, "sam_mask_head: vec", 224)
    M = int(hyper_in.shape[1])
    if out is None:
        out = torch.empty((images, M, 4 * g, 4 * g), dtype=torch.float32, device=x.device)
    else:
        _f32_dev(out, "sam_mask_head: out", images * M * 16 * g * g)
    _lib.check(_lib.lib().tg_sam_mask_head(_dt(x), _ptr(x), images, g, _ptr(w1), _ptr(w2), _ptr(vec), _ptr(hyper_in), M, float(eps), _ptr(out), _stream()))
    return out


def sam_mask_post(logits, padded_size, reshaped_size, original_size, target_size, threshold=0.0, out=None):
    """``tg_sam_mask_post``: fp32 logits [..., L, L] -> (uint8 mask [..., ht, wt], int32 areas [...]): post_process_masks (bilinear to ``padded_size``, crop to
    ``reshaped_size`` (hr, wr), bilinear to ``original_size`` (h0, w0), > threshold) and the reference's bilinear resize of the boolean mask to
    ``target_size`` (ht, wt), fused.  ``out``: a caller pair (mask, areas)."""
    _f32_dev(logits, "sam_mask_post: logits")
    if logits.ndim < 3 or logits.shape[-1] != logits.shape[-2]:
        raise RuntimeError(f"sam_mask_post: logits [..., L, L] expected, got {tuple(logits.shape)}")
    lead, L = tuple(logits.shape[:-2]), int(logits.shape[-1])
    planes = 1
    for s in lead:
        planes *= int(s)
    (hr, wr), (h0, w0), (ht, wt) = [tuple(int(v) for v in s) for s in (reshaped_size, original_size, target_size)]
    if out is None:
        mask = torch.empty(lead + (max(ht, 0), max(wt, 0)), dtype=torch.uint8, device=logits.device)
        areas = torch.empty(lead, dtype=torch.int32, device=logits.device)
    else:
        mask, areas = out
        if (mask.dtype != torch.uint8 or areas.dtype != torch.int32 or not mask.is_cuda or not areas.is_cuda or not mask.is_contiguous()
                or not areas.is_contiguous() or mask.numel() != planes * ht * wt or areas.numel() != planes):
            raise RuntimeError(f"sam_mask_post: out must be (uint8 [{planes}, {ht}, {wt}], int32 [{planes}]) contiguous device tensors")
    _lib.check(_lib.lib().tg_sam_mask_post(_ptr(logits), planes, L, int(padded_size), hr, wr, h0, w0, float(threshold), ht, wt, _ptr(mask), _ptr(areas),
                                           _stream()))
    return mask, areas


def attention_wide(q, q_ld, q_bs, k0, k0_ld, k0_bs, vt0, vt0_ld, vt0_bs, len0, batch, heads, head_dim, n_q, scale, out, out_ld, out_bs, key_splits=None,
                   key_mask=None):
    """``tg_attention_wide``: one-segment flash attention for head dims 256 / 512 (the VAE mid block), the argument list of ``attention`` without
    the second segment, mask, causal flag and device scalar.  Another head dim is an error (``attention`` takes multiples of 8 up to 160).
    ``key_splits``: None / 1 = the unsplit launch; 0 = the planner's choice (``tg_attention_wide_splits``), n >= 2 = n splits (clamped to the number of
    32-key tiles).  More than one effective split runs ``tg_attention_wide_split``: a partial launch and a combine launch, fp32 partials in the
    persistent ``workspace`` of the current slot (``tg_attention_wide_workspace_bytes``).
    ``key_mask``: uint8 [batch, len0], 1 = the key is masked for every query of its batch item (``tg_attention_wide_kmask``; a key-padding mask).  It
    also serves a key count that is no multiple of 8: pad ``len0`` (and the V^T pitch) to one and mask the tail.  A row whose keys are ALL masked
    is outside the contract and comes out as zeros."""
    _need_cuda(q)
    d = _attn_desc(q, q_ld, q_bs, k0, k0_ld, k0_bs, vt0, vt0_ld, vt0_bs, len0, batch, heads, head_dim, n_q, scale, out, out_ld, out_bs)
    if key_mask is not None:
        if (not isinstance(key_mask, torch.Tensor) or key_mask.dtype != torch.uint8 or key_mask.ndim != 2
                or tuple(key_mask.shape) != (int(batch), int(len0)) or not key_mask.is_contiguous()):
            raise RuntimeError(f"attention_wide: key_mask must be a contiguous uint8 tensor [{int(batch)}, {int(len0)}] (1 = masked), got "
                               f"{tuple(key_mask.shape) if isinstance(key_mask, torch.Tensor) else type(key_mask)} "
                               f"{getattr(key_mask, 'dtype', '')}")
        if not key_mask.is_cuda or key_mask.device != q.device:
            raise RuntimeError(f"attention_wide: key_mask must live on {q.device}")
    L = _lib.lib()
    S = 1
    if key_splits is not None and int(key_splits) != 1:
        if int(key_splits) < 0:
            raise RuntimeError(f"attention_wide: key_splits must be None, 0 (planner) or >= 1, got {key_splits}")
        S = L.tg_attention_wide_splits(C.byref(d), int(key_splits))
        if S < 0:
            _lib.check(S)                                                    # a refused descriptor: the code and message of the library
    if key_mask is not None:
        ws = workspace(int(L.tg_attention_wide_workspace_bytes(C.byref(d), S)), q.device) if S > 1 else None
        launch = lambda: _lib.check(L.tg_attention_wide_kmask(C.byref(d), key_mask.data_ptr(), int(len0), max(S, 1), _ptr(ws),   # noqa: E731
                                                              ws.numel() * 4 if ws is not None else 0, _stream()))
    elif S > 1:
        nbytes = int(L.tg_attention_wide_workspace_bytes(C.byref(d), S))
        ws = workspace(nbytes, q.device)
        launch = lambda: _lib.check(L.tg_attention_wide_split(C.byref(d), S, ws.data_ptr(), ws.numel() * 4, _stream()))   # noqa: E731
    else:
        launch = lambda: _lib.check(L.tg_attention_wide(C.byref(d), _stream()))                                            # noqa: E731
    if _gemm_profile is None:
        launch()
        return out
    # profiling mode (bench.py roofline leg), as ``attention``: algorithmic flops = QK^T + PV, no recomputed column half counted
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    launch()
    e1.record()
    rec = dict(splits=S, M=int(batch) * int(n_q), N=int(heads) * int(head_dim), K=int(len0), has_res=False,
               n_out=int(heads) * int(head_dim), attention=True, batch=int(batch))
    if S == 1:
        _gemm_profile.append(dict(rec, kernel=f"attention_wide_kernel<d{int(head_dim)}>", flops=4.0 * batch * heads * n_q * len0 * head_dim, events=(e0, e1)))
        return out
    # the C call issues the partial and the combine launch back to back, so the events around it time the PAIR: that time is on the partial's row (with
    # the algorithmic flops), the combine's row is the launch record with the (empty) interval after it
    e2 = torch.cuda.Event(enable_timing=True)
    e2.record()
    _gemm_profile.append(dict(rec, kernel=f"attention_wide_kernel<d{int(head_dim)},split{S}>", flops=4.0 * batch * heads * n_q * len0 * head_dim,
                              events=(e0, e1), includes_combine=True))
    _gemm_profile.append(dict(rec, kernel=f"attention_wide_combine_kernel<d{int(head_dim)}>", flops=0.0, events=(e1, e2), timed_with_partial=True))
    return out


def attn_probs(q, q_ld, q_bs, k, k_ld, k_bs, batch, b0, heads, head_dim, n_q, length, scale, tokens=None):
    """fp32 [batch-b0, heads, n_q, n_tokens] softmax probabilities (save_attn_to_dict side channel)."""
    nt = length if tokens is None else int(tokens.numel())
    out = torch.empty((batch - b0, heads, n_q, nt), dtype=torch.float32, device=q.device)
    _lib.check(_lib.lib().tg_attn_probs(_dt(q), batch, b0, heads, head_dim, n_q, _ptr(q), q_ld, q_bs, _ptr(k), k_ld, k_bs,
                                        length, float(scale), _ptr(tokens), nt, _ptr(out), _stream()))
    return out


def groupnorm(x0, batch, hw, groups, eps, gamma, beta, silu=False, x1=None, out=None):
    _need_cuda(x0)
    c0 = x0.shape[-1]
    c1 = x1.shape[-1] if x1 is not None else 0
    L = _lib.lib()
    if out is None:
        out = torch.empty((batch * hw, c0 + c1), dtype=x0.dtype, device=x0.device)
    scratch = workspace(L.tg_groupnorm_scratch_bytes(batch, hw, groups), x0.device)
    _lib.check(L.tg_groupnorm(_dt(x0), _ptr(x0), _ptr(x1), c0, c1, batch, hw, groups, float(eps), _ptr(gamma), _ptr(beta),
                              1 if silu else 0, _ptr(out), _ptr(scratch), _stream()))
    return out


def groupnorm_coef(x0, batch, hw, groups, eps, gamma, beta, x1=None):
    """GroupNorm statistics only -> fp32 [batch, 2, C]: a = rstd * gamma, d = beta - mean * a (``conv3x3(..., a_coef=)``)."""
    _need_cuda(x0)
    c0 = x0.shape[-1]
    c1 = x1.shape[-1] if x1 is not None else 0
    L = _lib.lib()
    coef = torch.empty((batch, 2, c0 + c1), dtype=torch.float32, device=x0.device)
    scratch = workspace(L.tg_groupnorm_scratch_bytes(batch, hw, groups), x0.device)
    _lib.check(L.tg_groupnorm_coef(_dt(x0), _ptr(x0), _ptr(x1), c0, c1, batch, hw, groups, float(eps), _ptr(gamma), _ptr(beta),
                                   _ptr(coef), _ptr(scratch), _stream()))
    return coef


def groupnorm_from_partials(gn, batch, hw, C_, eps, gamma, beta, x=None, silu=False, out=None):
    """GroupNorm whose partial sums a producer conv already wrote (``gemm(gn_out=...)``): ``x`` None -> the coefficients fp32 [batch, 2, C]
    (``groupnorm_coef``), else the normalised (+ SiLU) tensor (``groupnorm``); no statistics pass over the activation."""
    L = _lib.lib()
    part, nblk, groups = gn["partials"], int(gn["nblk"]), int(gn["groups"])
    if part.shape != (batch, nblk, groups, 2) or part.dtype != torch.float32 or not part.is_cuda:
        raise RuntimeError("groupnorm_from_partials: partials must be the fp32 [batch, nblk, groups, 2] tensor a producer conv wrote")
    dt = _dt(x) if x is not None else (0 if gamma.dtype == torch.bfloat16 else 1)
    if x is None:
        coef = torch.empty((batch, 2, C_), dtype=torch.float32, device=part.device)
        _lib.check(L.tg_groupnorm_from_partials(dt, None, int(C_), int(batch), int(hw), groups, float(eps), _ptr(gamma), _ptr(beta), 0, None,
                                                _ptr(coef), _ptr(part), nblk, _stream()))
        return coef
    _need_cuda(x)
    if out is None:
        out = torch.empty((batch * hw, C_), dtype=x.dtype, device=x.device)
    _lib.check(L.tg_groupnorm_from_partials(dt, _ptr(x), int(C_), int(batch), int(hw), groups, float(eps), _ptr(gamma), _ptr(beta), 1 if silu else 0,
                                            _ptr(out), None, _ptr(part), nblk, _stream()))
    return out


_slab_plans = {}


def conv3x3_takes_gn(dtype, batch, in_h, in_w, cin, c1, cout):
    """True when tg_gemm runs this stride-1 conv on the slab kernel (tg_gemm_plan kernel_kind 4), which can apply
    GroupNorm + SiLU to its input while staging it (``a_coef``)."""
    key = (dtype, batch, in_h, in_w, cin, c1, cout, os.environ.get("TG_GEMM_FLAGS"))
    hit = _slab_plans.get(key)
    if hit is None:
        L = _lib.lib()
        d = GemmDesc()
        d.dtype = 0 if dtype == torch.bfloat16 else 1
        d.mode = 1
        d.a0 = d.w = d.out = 16                      # plan only: pointers are not dereferenced, just non-NULL and aligned
        d.a1 = 16 if c1 else None
        d.c0, d.c1 = int(cin), int(c1)
        d.batch, d.in_h, d.in_w, d.out_h, d.out_w, d.stride, d.upsample = batch, in_h, in_w, in_h, in_w, 1, 0
        d.M, d.N, d.K = batch * in_h * in_w, int(cout), 9 * (cin + c1)
        d.ldc = int(cout)
        d.out_scale = 1.0
        kk = C.c_int32()
        hit = L.tg_gemm_plan(C.byref(d), None, None, None, C.byref(kk)) == 0 and kk.value == 4
        _slab_plans[key] = hit
    return hit


_ln_pp_plans = {}


def ln_qkv_takes_stats(dtype, M, C_, K, rows_per_batch):
    """True when tg_gemm runs the LayerNorm-folded q | k | v^T projection ([M, K] -> Q | K [M, 2 C] + V^T [M / rows, C, rows]) on the ping-pong tiles
    (tg_gemm_plan kernel_kind 7), which fold the norm from PRECOMPUTED row statistics: the caller runs ``layernorm_stats`` first.  Asked of the planner with
    the descriptor ``AttnProcessor`` launches (plan only, as ``conv3x3_takes_gn``)."""
    key = (dtype, M, C_, K, rows_per_batch, os.environ.get("TG_PP"))
    hit = _ln_pp_plans.get(key)
    if hit is None:
        d = GemmDesc()
        d.dtype = 0 if dtype == torch.bfloat16 else 1
        d.a0 = d.w = d.out = d.out_t = 16                   # plan only: pointers are not dereferenced, just non-NULL and aligned
        d.ln_u = d.ln_v = d.ln_rows = 16
        d.ln_eps = 1e-5
        d.c0 = d.K = int(K)
        d.M, d.N = int(M), 3 * int(C_)
        d.rows_per_batch, d.n_split, d.ldc, d.ldt = int(rows_per_batch), 2 * int(C_), 2 * int(C_), (int(rows_per_batch) + 7) // 8 * 8
        d.out_scale = 1.0
        kk = C.c_int32()
        hit = _lib.lib().tg_gemm_plan(C.byref(d), None, None, None, C.byref(kk)) == 0 and kk.value == 7
        _ln_pp_plans[key] = hit
    return hit


def layernorm(x, gamma, beta, eps=1e-5, out=None):
    _need_cuda(x)
    rows, Cc = x.shape
    if out is None:
        out = torch.empty((rows, Cc), dtype=x.dtype, device=x.device)
    _lib.check(_lib.lib().tg_layernorm(_dt(x), _ptr(x), rows, Cc, x.stride(0), float(eps), _ptr(gamma), _ptr(beta), _ptr(out),
                                       out.stride(0), _stream()))
    return out


def layernorm_add(x, res, gamma, beta, eps=1e-5, out=None):
    """``tg_layernorm_add``: LN(x + res) with the sum taken in fp32 from the two stored operands (a post-norm residual block without the rounding of
    the sum that a residual GEMM epilogue + ``layernorm`` has).  x, res [rows, C] (any row pitch, unit channel stride); gamma, beta [C]."""
    _need_cuda(x)
    rows, Cc = x.shape
    for name, t in (("res", res), ("gamma", gamma), ("beta", beta)):
        _need_cuda(t)
        if t.dtype != x.dtype or t.device != x.device:
            raise RuntimeError(f"layernorm_add: {name} must be a {x.dtype} tensor on {x.device}, got {t.dtype} on {t.device}")
    if tuple(res.shape) != (rows, Cc) or x.stride(1) != 1 or res.stride(1) != 1 or gamma.numel() != Cc or beta.numel() != Cc \
            or not gamma.is_contiguous() or not beta.is_contiguous():
        raise RuntimeError(f"layernorm_add: x and res must be [rows, C] with unit channel stride and gamma, beta contiguous [C]; got {tuple(x.shape)}, "
                           f"{tuple(res.shape)}, {tuple(gamma.shape)}, {tuple(beta.shape)}")
    if out is None:
        out = torch.empty((rows, Cc), dtype=x.dtype, device=x.device)
    elif out.dtype != x.dtype or out.device != x.device or tuple(out.shape) != (rows, Cc) or out.stride(1) != 1:
        raise RuntimeError(f"layernorm_add: out must be a {x.dtype} tensor [{rows}, {Cc}] on {x.device} with unit channel stride")
    _lib.check(_lib.lib().tg_layernorm_add(_dt(x), _ptr(x), x.stride(0), _ptr(res), res.stride(0), rows, Cc, float(eps), _ptr(gamma), _ptr(beta),
                                           _ptr(out), out.stride(0), _stream()))
    return out


def layernorm_stats(x, eps=1e-5):
    """fp32 [rows, 2] = (rstd, -rstd * mean) per row: the statistics half of ``layernorm`` (no normalised tensor), input of ``gemm(ln=...)``"""
    _need_cuda(x)
    rows, Cc = x.shape
    out = torch.empty((rows, 2), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().tg_layernorm_stats(_dt(x), _ptr(x), rows, Cc, x.stride(0), float(eps), _ptr(out), _stream()))
    return out


def geglu(x, out=None):
    rows, two_inner = x.shape
    inner = two_inner // 2
    if out is None:
        out = torch.empty((rows, inner), dtype=x.dtype, device=x.device)
    _lib.check(_lib.lib().tg_geglu(_dt(x), _ptr(x), rows, inner, _ptr(out), _stream()))
    return out


def act(x, kind, out=None):
    if out is None:
        out = torch.empty_like(x)
    _lib.check(_lib.lib().tg_act(_dt(x), _ptr(x), x.numel(), kind, _ptr(out), _stream()))
    return out


def add(a, b, out=None):
    if out is None:
        out = torch.empty_like(a)
    _lib.check(_lib.lib().tg_add(_dt(a), _ptr(a), _ptr(b), a.numel(), _ptr(out), _stream()))
    return out


def attention_bwd_supported(head_dim, n):
    """True when tg_attention_bwd (recompute-based self-attention reverse pass) takes the problem."""
    return head_dim % 8 == 0 and head_dim <= 64 and n % 8 == 0


def attention_bwd(q, k, v, dout, batch, n, heads, head_dim, scale):
    """Self-attention reverse pass without materialised probabilities: q, k, v, dout [batch * n, heads * head_dim] (contiguous rows) ->
    (dq, dk, dv) in the same layout.  Three launches of one kernel (+ three tg_transpose launches for the streamed K^T / Q^T / dO^T tiles)."""
    return _attention_bwd("tg_attention_bwd", q, k, v, dout, batch, n, heads, head_dim, scale)


def _attention_bwd(entry, q, k, v, dout, batch, n, heads, head_dim, scale):
    name = entry[3:]
    _need_cuda(q)
    inner = heads * head_dim
    for t in (q, k, v, dout):
        if t.shape != (batch * n, inner) or not t.is_contiguous() or t.dtype != q.dtype:
            raise RuntimeError(name + ": q, k, v, dout must be contiguous [batch * n, heads * head_dim] tensors of one dtype")
    L = _lib.lib()
    qt, kt, dot = transpose(q, batch, n, inner), transpose(k, batch, n, inner), transpose(dout, batch, n, inner)
    stats = torch.empty((batch, heads, n, 2), dtype=torch.float32, device=q.device)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
    d = _lib.AttnBwdDesc()
    d.dtype, d.batch, d.heads, d.head_dim, d.n = _dt(q), batch, heads, head_dim, n
    d.q, d.k, d.v, d.dout = _ptr(q), _ptr(k), _ptr(v), _ptr(dout)
    d.ld, d.bs = inner, n * inner
    d.qt, d.kt, d.doutt = _ptr(qt), _ptr(kt), _ptr(dot)
    d.t_ld, d.t_bs = n, inner * n
    d.stats = _ptr(stats)
    d.dq, d.dk, d.dv = _ptr(dq), _ptr(dk), _ptr(dv)
    d.scale = float(scale)
    _lib.check(getattr(L, entry)(C.byref(d), _stream()))
    return dq, dk, dv


def attention_bwd_cross(q, dout, k, v, batch, n_q, n_k, heads, head_dim, scale, ds_scale, extra=None):
    """dQ of one softmax segment of cross-attention (constant K / V): q, dout [batch * n_q, inner], k, v [batch * n_k, inner];
    ``extra`` fp32 [batch, heads, n_q, n_k] = d loss / d P or None.  Two launches (row statistics, dQ) for all (item, head) pairs."""
    return _attention_bwd_cross("tg_attention_bwd_cross", q, dout, k, v, batch, n_q, n_k, heads, head_dim, scale, ds_scale, extra)


def _attention_bwd_cross(entry, q, dout, k, v, batch, n_q, n_k, heads, head_dim, scale, ds_scale, extra):
    _need_cuda(q)
    inner = heads * head_dim
    lp = (n_k + 7) // 8 * 8
    kt = torch.zeros((batch, inner, lp), dtype=q.dtype, device=q.device)
    kt[:, :, :n_k] = k.reshape(batch, n_k, inner).transpose(1, 2)
    stats = torch.empty((batch, heads, n_q, 2), dtype=torch.float32, device=q.device)
    dq = torch.empty_like(q)
    d = _lib.AttnBwdCrossDesc()
    d.dtype, d.batch, d.heads, d.head_dim, d.n_q, d.n_k = _dt(q), batch, heads, head_dim, n_q, n_k
    d.q, d.dout, d.q_ld, d.q_bs = _ptr(q), _ptr(dout), inner, n_q * inner
    d.k, d.v, d.k_ld, d.k_bs = _ptr(k), _ptr(v), inner, n_k * inner
    d.kt, d.t_ld, d.t_bs = _ptr(kt), lp, inner * lp
    if extra is not None:
        if extra.dtype != torch.float32 or extra.shape != (batch, heads, n_q, n_k) or not extra.is_contiguous():
            raise RuntimeError(entry[3:] + ": extra must be a contiguous fp32 [batch, heads, n_q, n_k] tensor")
        d.extra, d.extra_ld = _ptr(extra), n_k
    d.stats, d.dq = _ptr(stats), _ptr(dq)
    d.scale, d.ds_scale = float(scale), float(ds_scale)
    _lib.check(getattr(_lib.lib(), entry)(C.byref(d), _stream()))
    return dq


def attention_bwd_wide_supported(head_dim, n):
    """True when tg_attention_bwd_wide (the recompute-based self-attention reverse pass for 64 < head_dim <= 160) takes the problem."""
    return head_dim % 8 == 0 and 64 < head_dim <= 160 and n % 8 == 0


def attention_bwd_wide(q, k, v, dout, batch, n, heads, head_dim, scale):
    """``attention_bwd`` for 64 < head_dim <= 160 (tg_attention_bwd_wide): same arguments, transposes and ``stats`` scratch."""
    return _attention_bwd("tg_attention_bwd_wide", q, k, v, dout, batch, n, heads, head_dim, scale)


def attention_bwd_cross_wide(q, dout, k, v, batch, n_q, n_k, heads, head_dim, scale, ds_scale, extra=None):
    """``attention_bwd_cross`` for 64 < head_dim <= 160 (tg_attention_bwd_cross_wide): same arguments, zero-padded K^T and ``stats`` scratch."""
    return _attention_bwd_cross("tg_attention_bwd_cross_wide", q, dout, k, v, batch, n_q, n_k, heads, head_dim, scale, ds_scale, extra)


def transpose(src, batch, rows, cols, out=None):
    """out[b, c, r] = src[b, r, c]"""
    if out is None:
        out = torch.empty((batch, cols, rows), dtype=src.dtype, device=src.device)
    _lib.check(_lib.lib().tg_transpose(_dt(src), _ptr(src), batch, rows, cols, _ptr(out), _stream()))
    return out


def conv1x1_nchw(x, weight, bias, in_scale=1.0):
    """fp32 NCHW thin 1x1 conv (VAE post_quant_conv): x [B, cin, h, w], weight [cout, cin] fp32"""
    _need_cuda(x)
    B, cin, h, w = x.shape
    cout = weight.shape[0]
    out = torch.empty((B, cout, h, w), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().tg_conv1x1_nchw(_ptr(x), B, cin, cout, h * w, _ptr(weight), _ptr(bias), float(in_scale), _ptr(out), _stream()))
    return out


def softmax_rows(x, scale=1.0, out=None):
    """row softmax of a 2-D [rows, cols] tensor (cols % 8 == 0); ``out`` may alias ``x``"""
    _need_cuda(x)
    rows, cols = x.shape
    if out is None:
        out = torch.empty_like(x)
    _lib.check(_lib.lib().tg_softmax_rows(_dt(x), _ptr(x), rows, cols, x.stride(0), float(scale), _ptr(out), out.stride(0), _stream()))
    return out


_SRC = {torch.bfloat16: 0, torch.float16: 1, torch.float32: 2}


def conv_in(sample, weight_packed, bias, cout, dtype, pair=False):
    """sample NCHW (bf16/f16/f32) -> token-major [B*h*w, cout] in ``dtype``.  ``pair``: the caller vouches that sample[:B/2] and sample[B/2:] hold the same
    values — the conv runs on the first half and both halves of the output are written (``tg_conv_in_dup``, or one ``dup_rows`` copy)."""
    _need_cuda(sample)
    B, cin, h, w = sample.shape
    out = torch.empty((B * h * w, cout), dtype=dtype, device=sample.device)
    if pair:
        L = _lib.lib()
        hb, rows = B // 2, (B // 2) * h * w
        if L.tg_conv_in_takes_dup(cin, cout) and out.data_ptr() % 16 == 0 and weight_packed.data_ptr() % 8 == 0:
            _lib.check(L.tg_conv_in_dup(_dt(out), _ptr(sample), _SRC[sample.dtype], hb, cin, h, w, _ptr(weight_packed), _ptr(bias), cout, _ptr(out),
                                        rows * cout, _stream()))
        else:
            _lib.check(L.tg_conv_in(_dt(out), _ptr(sample), _SRC[sample.dtype], hb, cin, h, w, _ptr(weight_packed), _ptr(bias), cout, _ptr(out), _stream()))
            dup_rows(out[:rows], out[rows:])
        return out
    _lib.check(_lib.lib().tg_conv_in(_dt(out), _ptr(sample), _SRC[sample.dtype], B, cin, h, w, _ptr(weight_packed), _ptr(bias),
                                     cout, _ptr(out), _stream()))
    return out


def conv_out_takes_gn(cin, h, w, cout):
    """True when conv_out runs on the matrix-core kernel, which can apply conv_norm_out + SiLU while it stages its window (``conv_out(..., coef=)``)."""
    return bool(_lib.lib().tg_conv_out_takes_coef(int(cin), int(h), int(w), int(cout)))


def conv_out(x, weight_packed, bias, batch, h, w, cout, out_dtype, coef=None, silu=True):
    """token-major [B*h*w, cin] -> NCHW [B, cout, h, w]; ``coef`` (groupnorm_coef of conv_norm_out): x is the raw block output, GroupNorm (+SiLU) applied
    inside the launch (only where conv_out_takes_gn)."""
    cin = x.shape[-1]
    out = torch.empty((batch, cout, h, w), dtype=out_dtype, device=x.device)
    if coef is not None:
        _lib.check(_lib.lib().tg_conv_out_gn(_dt(x), _ptr(x), _ptr(coef), 1 if silu else 0, batch, cin, h, w, _ptr(weight_packed), _ptr(bias), cout,
                                             _ptr(out), 1 if out_dtype == torch.float32 else 0, _stream()))
        return out
    _lib.check(_lib.lib().tg_conv_out(_dt(x), _ptr(x), batch, cin, h, w, _ptr(weight_packed), _ptr(bias), cout, _ptr(out),
                                      1 if out_dtype == torch.float32 else 0, _stream()))
    return out


def timestep_embedding(t_dev, rows, dim, flip_sin_to_cos, freq_shift, dtype, t_stride=0, index=None):
    out = torch.empty((rows, dim), dtype=dtype, device=t_dev.device)
    _lib.check(_lib.lib().tg_timestep_embedding(_dt(out), _ptr(t_dev), _ptr(index), t_stride, rows, dim, 1 if flip_sin_to_cos else 0,
                                                float(freq_shift), _ptr(out), dim, _stream()))
    return out


def _step_epilogue(entry, noise_pred, latents, guidance_scale, coef, step_idx, has_cfg, advance, frozen, frozen_mask, frozen_steps, history, model_in,
                   state=(), own=()):
    """What the three step epilogues share (csrc/tg_step.hip): the geometry read off ``latents`` and the pointer marshalling.  ``state``: the entry
    point's own leading arguments after ``latents``; ``own``: its own arguments after ``advance``."""
    n_img = latents.shape[0]
    chw = latents[0].numel()
    hw = latents.shape[-1] * latents.shape[-2]
    mask_per_img = 1 if (frozen_mask is not None and frozen_mask.numel() == n_img * hw and n_img > 1) else 0
    mi_dt = -1 if model_in is None else _SRC[model_in.dtype]
    _lib.check(getattr(_lib.lib(), entry)(_ptr(noise_pred), _ptr(latents), *state, n_img, chw, hw, 1 if has_cfg else 0, float(guidance_scale), _ptr(coef),
                                          _ptr(step_idx), 1 if advance else 0, *own, _ptr(frozen), _ptr(frozen_mask), mask_per_img, int(frozen_steps),
                                          _ptr(history), _ptr(model_in), mi_dt, _stream()))


def step_epilogue(noise_pred, latents, guidance_scale, coef, step_idx, *, has_cfg=True, advance=True, prediction_type=0, frozen=None,
                  frozen_mask=None, frozen_steps=0, history=None, model_in=None):
    _step_epilogue("tg_step_epilogue", noise_pred, latents, guidance_scale, coef, step_idx, has_cfg, advance, frozen, frozen_mask, frozen_steps, history,
                   model_in, own=(prediction_type,))


def step_epilogue_sigma(noise_pred, latents, guidance_scale, coef, step_idx, *, has_cfg=True, advance=True, noise=None, frozen=None,
                        frozen_mask=None, frozen_steps=0, history=None, model_in=None):
    """Euler / Euler-ancestral step (``tg_step_epilogue_sigma``): ``coef`` = the scheduler's ``coef_table`` on the device, ``noise`` =
    the pre-drawn ancestral noise table [n_steps, n_img, C, h, w] (storage dtype or fp32) or None"""
    _step_epilogue("tg_step_epilogue_sigma", noise_pred, latents, guidance_scale, coef, step_idx, has_cfg, advance, frozen, frozen_mask, frozen_steps,
                   history, model_in, own=(_ptr(noise), -1 if noise is None else _SRC[noise.dtype]))


def step_epilogue_dpm(noise_pred, latents, x0_prev, guidance_scale, coef, step_idx, *, has_cfg=True, advance=True, frozen=None,
                      frozen_mask=None, frozen_steps=0, history=None, model_in=None):
    """DPM-Solver++ multistep step (``tg_step_epilogue_dpm``): ``coef`` = ``DPMSolverMultistepScheduler.coef_table`` on the device
    (fp32 [n_steps, 8]), ``x0_prev`` = the fp32 state tensor shaped like ``latents`` (read when the row's C != 0, then overwritten)"""
    if x0_prev is None or x0_prev.dtype != torch.float32 or x0_prev.numel() != latents.numel() or not x0_prev.is_contiguous():
        raise ValueError("step_epilogue_dpm: x0_prev must be a contiguous fp32 tensor with the latents' element count")
    if coef.dtype != torch.float32 or coef.dim() != 2 or coef.shape[1] != 8 or not coef.is_contiguous():
        raise ValueError("step_epilogue_dpm: coef must be a contiguous fp32 [n_steps, 8] table")
    _step_epilogue("tg_step_epilogue_dpm", noise_pred, latents, guidance_scale, coef, step_idx, has_cfg, advance, frozen, frozen_mask, frozen_steps,
                   history, model_in, state=(_ptr(x0_prev),))


def pixel_unshuffle(x, factor):
    """NCHW [B, C, h, w] (bf16 / fp16) -> token-major [B * (h/f) * (w/f), C f^2] (``F.pixel_unshuffle`` then NHWC)"""
    _need_cuda(x)
    B, ch, h, w = x.shape
    x = x.contiguous()
    out = torch.empty((B * (h // factor) * (w // factor), ch * factor * factor), dtype=x.dtype, device=x.device)
    _lib.check(_lib.lib().tg_pixel_unshuffle(_dt(x), _ptr(x), B, ch, h, w, int(factor), _ptr(out), _stream()))
    return out


def relu(x, out=None):
    if out is None:
        out = torch.empty_like(x)
    _lib.check(_lib.lib().tg_relu(_dt(x), _ptr(x), x.numel(), _ptr(out), _stream()))
    return out


def avgpool2x2(x, batch, h, w):
    """AvgPool2d(2, 2, ceil_mode=True) of token-major [batch * h * w, C] -> [batch * ceil(h/2) * ceil(w/2), C]"""
    ch = x.shape[-1]
    out = torch.empty((batch * ((h + 1) // 2) * ((w + 1) // 2), ch), dtype=x.dtype, device=x.device)
    _lib.check(_lib.lib().tg_avgpool2x2(_dt(x), _ptr(x), batch, h, w, ch, _ptr(out), _stream()))
    return out


def scale_repeat(x, scale, copies, out=None):
    """``cat([x * scale] * copies)`` along the leading dimension (x contiguous)"""
    if out is None:
        out = torch.empty((copies * x.shape[0], *x.shape[1:]), dtype=x.dtype, device=x.device)
    _lib.check(_lib.lib().tg_scale_repeat(_dt(x), _ptr(x), x.numel(), float(scale), int(copies), _ptr(out), _stream()))
    return out


def image_from_u8(images, dtype, range_mode=1, copies=1, out=None):
    """uint8 RGB ``[B, H, W, 3]`` on the device -> NCHW ``[copies * B, 3, H, W]`` in ``dtype`` (bf16 / fp16 / fp32); copy r of image b is row ``r * B + b``
    (``cat([x] * copies)``).  ``range_mode`` 1: ``2 * (u / 255) - 1`` (VAE encoder input), 0: ``u / 255`` (ControlNet control image); fp32 arithmetic with
    an IEEE division, one rounding to ``dtype``: bit-equal to ``torch.from_numpy(a.astype(np.float32) / 255.0)`` [``* 2.0 - 1.0``] ``.permute(0, 3, 1, 2)
    .to(dtype)``."""
    _need_cuda(images)
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] != 3:
        raise ValueError(f"image_from_u8: uint8 [B, H, W, 3] expected, got {images.dtype} {tuple(images.shape)}")
    if dtype not in _SRC:
        raise RuntimeError(f"theatergen_amd: image_from_u8 writes bf16 / fp16 / fp32, not {dtype}")
    if int(copies) < 1:
        raise ValueError(f"image_from_u8: copies must be >= 1, got {copies}")
    B, H, W, _ = images.shape
    images = images.contiguous()
    shape = (int(copies) * B, 3, H, W)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=images.device)
    elif tuple(out.shape) != shape or out.dtype != dtype or not out.is_contiguous():
        raise ValueError(f"image_from_u8: out must be a contiguous {dtype} tensor of shape {shape}")
    _lib.check(_lib.lib().tg_image_from_u8(_ptr(images), B, H, W, int(range_mode), int(copies), _ptr(out), _SRC[dtype], _stream()))
    return out


def image_to_u8(images, out=None):
    """NCHW ``[B, 3, H, W]`` (bf16 / fp16 / fp32) in [-1, 1] -> uint8 RGB ``[B, H, W, 3]`` on the device: bit-equal to ``((x.float() / 2 + 0.5).clamp(0, 1)
    .permute(0, 2, 3, 1).numpy() * 255).round().astype("uint8")`` (ties to even; NaN, which has no value there, gives 0)."""
    _need_cuda(images)
    if images.dim() != 4 or images.shape[1] != 3 or images.dtype not in _SRC:
        raise ValueError(f"image_to_u8: bf16 / fp16 / fp32 [B, 3, H, W] expected, got {images.dtype} {tuple(images.shape)}")
    B, _, H, W = images.shape
    images = images.contiguous()
    if out is None:
        out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=images.device)
    elif tuple(out.shape) != (B, H, W, 3) or out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError(f"image_to_u8: out must be a contiguous uint8 tensor of shape {(B, H, W, 3)}")
    _lib.check(_lib.lib().tg_image_to_u8(_ptr(images), _SRC[images.dtype], B, H, W, _ptr(out), _stream()))
    return out


LINEART_DENSE, LINEART_BORDER, LINEART_PARITY = 0, 1, 2      # x_layout / res_layout of tg_lineart_instnorm


def lineart_instnorm(x, batch, h, w, c, *, layout=LINEART_DENSE, relu=False, res=None, res_layout=LINEART_DENSE, border=False, eps=1e-5, out=None):
    """``nn.InstanceNorm2d(c)`` (defaults) [+ ReLU] [+ res] of the h x w image held in ``x`` (see tg_lineart_instnorm for the three input layouts) ->
    token-major [batch * h * w, c], or with ``border`` the reflect-1 padded image [batch * (h + 2) * (w + 2), c] a pad-1 ``conv3x3`` then takes."""
    _need_cuda(x)
    L = _lib.lib()
    need = L.tg_lineart_instnorm_scratch_bytes(int(batch), int(h), int(w), int(c))
    if need < 0:
        raise RuntimeError(f"theatergen_amd: lineart_instnorm takes c in (64, 128, 256), got batch {batch}, {h} x {w} x {c}")
    rows_in = {LINEART_DENSE: h * w, LINEART_BORDER: (h + 2) * (w + 2), LINEART_PARITY: h * w}
    if x.numel() != batch * rows_in[layout] * c or not x.is_contiguous():
        raise ValueError(f"lineart_instnorm: x must be dense with {batch * rows_in[layout] * c} elements for layout {layout}, got {tuple(x.shape)}")
    if res is not None and (res.numel() != batch * rows_in[res_layout] * c or not res.is_contiguous() or res.dtype != x.dtype):
        raise ValueError(f"lineart_instnorm: res must be dense {x.dtype} with {batch * rows_in[res_layout] * c} elements, got {tuple(res.shape)}")
    rows = batch * ((h + 2) * (w + 2) if border else h * w)
    if out is None:
        out = torch.empty((rows, c), dtype=x.dtype, device=x.device)
    elif tuple(out.shape) != (rows, c) or out.dtype != x.dtype or not out.is_contiguous():
        raise ValueError(f"lineart_instnorm: out must be a contiguous {x.dtype} tensor of shape {(rows, c)}")
    scratch = workspace(need, x.device)
    _lib.check(L.tg_lineart_instnorm(_dt(x), _ptr(x), int(layout), int(batch), int(h), int(w), int(c), float(eps), 1 if relu else 0, _ptr(res),
                                     int(res_layout), _ptr(out), 1 if border else 0, _ptr(scratch), _stream()))
    return out


def lineart_conv7_in(image, w_packed, bias, out=None):
    """``ReflectionPad2d(3)`` + ``Conv2d(3, 64, 7)`` of the NCHW image [B, 3, H, W] (bf16 / fp16) -> token-major [B * H * W, 64]; ``w_packed`` =
    ``weights_pack.pack_conv7x7_fp32`` (fp32 [147, 64]), ``bias`` fp32 [64]."""
    _need_cuda(image)
    if image.dim() != 4 or image.shape[1] != 3:
        raise ValueError(f"lineart_conv7_in: [B, 3, H, W] expected, got {tuple(image.shape)}")
    if w_packed.dtype != torch.float32 or tuple(w_packed.shape) != (147, 64) or bias.dtype != torch.float32 or bias.numel() != 64:
        raise ValueError("lineart_conv7_in: w_packed must be fp32 [147, 64] and bias fp32 [64]")
    B, _, H, W = image.shape
    image = image.contiguous()
    if out is None:
        out = torch.empty((B * H * W, 64), dtype=image.dtype, device=image.device)
    _lib.check(_lib.lib().tg_lineart_conv7_in(_dt(image), _ptr(image), B, H, W, _ptr(w_packed.contiguous()), _ptr(bias.contiguous()), _ptr(out), _stream()))
    return out


def lineart_conv7_out(x, batch, h, w, w_packed, bias, want_sigmoid=False, out=None):
    """``ReflectionPad2d(3)`` + ``Conv2d(64, 1, 7)`` + sigmoid + the annotator's byte step over token-major x [batch * h * w, 64] -> uint8 RGB
    [batch, h, w, 3] holding ``255 - trunc(255 s)`` three times (and, with ``want_sigmoid``, s as fp32 [batch, h, w]).  ``w_packed`` =
    ``weights_pack.pack_conv7x7_to1_fp32`` (fp32 [49, 64]); ``bias`` a Python float."""
    _need_cuda(x)
    if x.numel() != batch * h * w * 64 or not x.is_contiguous():
        raise ValueError(f"lineart_conv7_out: x must be dense [{batch * h * w}, 64], got {tuple(x.shape)}")
    if w_packed.dtype != torch.float32 or tuple(w_packed.shape) != (49, 64) or not w_packed.is_contiguous():
        raise ValueError("lineart_conv7_out: w_packed must be contiguous fp32 [49, 64]")
    if out is None:
        out = torch.empty((batch, h, w, 3), dtype=torch.uint8, device=x.device)
    elif tuple(out.shape) != (batch, h, w, 3) or out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError(f"lineart_conv7_out: out must be a contiguous uint8 tensor of shape {(batch, h, w, 3)}")
    sig = torch.empty((batch, h, w), dtype=torch.float32, device=x.device) if want_sigmoid else None
    _lib.check(_lib.lib().tg_lineart_conv7_out(_dt(x), _ptr(x), int(batch), int(h), int(w), _ptr(w_packed), float(bias), _ptr(out), _ptr(sig), _stream()))
    return (out, sig) if want_sigmoid else out


resample_launches = {"fused": 0, "two_launch": 0}           # calls of image_resample_u8 by route (tests and timing scripts read it)


def image_resample_u8(images, plan_v, plan_h, lut, dtype, window=None, pad=None, out=None, u8_out=None, route=None):
    """uint8 RGB ``[B, hs, ws, 3]`` on the device -> ``pixel_values`` NCHW ``[B, 3, hp, wp]`` in ``dtype`` (bf16 / fp16 / fp32): Pillow's 8-bit resize
    (horizontal pass first, each pass rounded to uint8), ``lut[c][byte]`` (fp32 ``[3, 256]``, the processor's rescale + normalise), one rounding to
    ``dtype``, +0 outside the window.  ``plan_v`` / ``plan_h``: ``preprocess.device_plan(hs, rh, filter, device)`` / ``(ws, rw, ...)``.
    ``window`` = (oy, ox, oh, ow) inside the resized image (default: all of it); ``pad`` = (hp, wp) (default: the window, or ``out``'s shape).
    ``u8_out``: a uint8 ``[B, oh, ow, 3]`` tensor, or True to allocate one; returned as the second value.  ``route``: None lets the plan decide
    (``preprocess.resample_route``), "fused" / "two_launch" force one; both give the same bytes.  See tg_image_resample_u8 in include/theatergen_hip.h."""
    from . import preprocess
    _need_cuda(images)
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] != 3:
        raise ValueError(f"image_resample_u8: uint8 [B, H, W, 3] expected, got {images.dtype} {tuple(images.shape)}")
    if dtype not in _SRC:
        raise RuntimeError(f"theatergen_amd: image_resample_u8 writes bf16 / fp16 / fp32, not {dtype}")
    B, hs, ws, _ = (int(v) for v in images.shape)
    (pv, kv, fv, cv), (ph, kh, fh, ch) = plan_v, plan_h
    if (pv.in_size, ph.in_size) != (hs, ws):
        raise ValueError(f"image_resample_u8: plans for {(pv.in_size, ph.in_size)} sources, images are {(hs, ws)}")
    for t in (kv, fv, cv, kh, fh, ch, lut):
        if not t.is_cuda or t.device != images.device or not t.is_contiguous():
            raise ValueError("image_resample_u8: tables and lut must be contiguous tensors on the images' device")
    if lut.dtype != torch.float32 or tuple(lut.shape) != (3, 256) or any(t.dtype != torch.int32 for t in (kv, fv, cv, kh, fh, ch)):
        raise ValueError("image_resample_u8: lut fp32 [3, 256] and int32 tables expected")
    rh, rw = pv.out_size, ph.out_size
    oy, ox, oh, ow = (int(v) for v in (window if window is not None else (0, 0, rh, rw)))
    if oy < 0 or ox < 0 or oh < 1 or ow < 1 or oy + oh > rh or ox + ow > rw:
        raise ValueError(f"image_resample_u8: window {(oy, ox, oh, ow)} leaves the resized image {(rh, rw)}")
    if pad is None:
        pad = tuple(out.shape[-2:]) if out is not None else (oh, ow)
    hp, wp = int(pad[0]), int(pad[1])
    if hp < oh or wp < ow:
        raise ValueError(f"image_resample_u8: pad {(hp, wp)} smaller than the window {(oh, ow)}")
    images = images.contiguous()
    if out is None:
        out = torch.empty((B, 3, hp, wp), dtype=dtype, device=images.device)
    elif tuple(out.shape) != (B, 3, hp, wp) or out.dtype != dtype or not out.is_contiguous() or out.device != images.device:
        raise ValueError(f"image_resample_u8: out must be a contiguous {dtype} tensor of shape {(B, 3, hp, wp)} on the images' device")
    if u8_out is True:
        u8_out = torch.empty((B, oh, ow, 3), dtype=torch.uint8, device=images.device)
    elif u8_out is not None and (tuple(u8_out.shape) != (B, oh, ow, 3) or u8_out.dtype != torch.uint8 or not u8_out.is_contiguous()
                                 or u8_out.device != images.device):
        raise ValueError(f"image_resample_u8: u8_out must be a contiguous uint8 tensor of shape {(B, oh, ow, 3)} on the images' device")
    planned, rows = preprocess.resample_route(pv, oy, oh)
    if route is None:
        route = planned
    elif route not in ("fused", "two_launch") or (route == "fused" and planned != "fused"):
        raise ValueError(f"image_resample_u8: route {route!r} (the plan needs {rows} staged rows: {planned})")
    tmp = workspace(B * hs * ow * 3, images.device) if route == "two_launch" else None
    _lib.check(_lib.lib().tg_image_resample_u8(_ptr(images), B, hs, ws, _ptr(kv), _ptr(fv), _ptr(cv), int(kv.shape[1]), rh, _ptr(kh), _ptr(fh), _ptr(ch),
                                               int(kh.shape[1]), rw, oy, ox, oh, ow, _ptr(lut), _ptr(out), _SRC[dtype], hp, wp, _ptr(u8_out), rows,
                                               _ptr(tmp), _stream()))
    resample_launches[route] += 1
    return out if u8_out is None else (out, u8_out)


def cv_area_u8(images, size, dtype, out=None, u8_out=None):
    """``cv2.resize(image, (wd, hd), interpolation=cv2.INTER_AREA)`` of uint8 RGB ``[B, hs, ws, 3]`` on the device (``size`` = (hd, wd), neither axis
    growing), then ``byte / 255`` as NCHW ``[B, 3, hd, wd]`` in ``dtype`` (bf16 / fp16 / fp32): bit-equal to ``image_from_u8(resized, dtype,
    range_mode=0)``, in one launch.  ``u8_out``: a uint8 ``[B, hd, wd, 3]`` tensor, or True to allocate one: the resized bytes, returned as the second
    value.  The arithmetic is OpenCV's portable C++ path as tg_cv_area_u8 in include/theatergen_hip.h restates it (not run against a cv2 build)."""
    from . import cv_resize
    _need_cuda(images)
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] != 3:
        raise ValueError(f"cv_area_u8: uint8 [B, H, W, 3] expected, got {images.dtype} {tuple(images.shape)}")
    if dtype not in _SRC:
        raise RuntimeError(f"theatergen_amd: cv_area_u8 writes bf16 / fp16 / fp32, not {dtype}")
    B, hs, ws, _ = (int(v) for v in images.shape)
    hd, wd = int(size[0]), int(size[1])
    if hd > hs or wd > ws or hd < 1 or wd < 1:
        raise NotImplementedError(f"cv_area_u8: {(hs, ws)} -> {(hd, wd)}: INTER_AREA is built for shrinking or equal axes only")
    images = images.contiguous()
    if out is None:
        out = torch.empty((B, 3, hd, wd), dtype=dtype, device=images.device)
    elif tuple(out.shape) != (B, 3, hd, wd) or out.dtype != dtype or not out.is_contiguous() or out.device != images.device:
        raise ValueError(f"cv_area_u8: out must be a contiguous {dtype} tensor of shape {(B, 3, hd, wd)} on the images' device")
    if u8_out is True:
        u8_out = torch.empty((B, hd, wd, 3), dtype=torch.uint8, device=images.device)
    elif u8_out is not None and (tuple(u8_out.shape) != (B, hd, wd, 3) or u8_out.dtype != torch.uint8 or not u8_out.is_contiguous()
                                 or u8_out.device != images.device):
        raise ValueError(f"cv_area_u8: u8_out must be a contiguous uint8 tensor of shape {(B, hd, wd, 3)} on the images' device")
    if cv_resize.area_is_integer(hs, hd) and cv_resize.area_is_integer(ws, wd):
        tables, rows = (None, None, None, 0, None, None, None, 0), 0
    else:
        (pv, fv, cv, av), (ph, fh, ch, ah) = cv_resize.device_area_plan(hs, hd, images.device), cv_resize.device_area_plan(ws, wd, images.device)
        rows = cv_resize.area_stage_rows(pv)
        if rows > _lib.CV_AREA_STAGE_ROWS:
            raise NotImplementedError(f"cv_area_u8: {hs} -> {hd} rows: a tile's vertical entries span {rows} source rows; the kernel stages "
                                      f"{_lib.CV_AREA_STAGE_ROWS}")
        tables = (_ptr(fv), _ptr(cv), _ptr(av), int(av.shape[1]), _ptr(fh), _ptr(ch), _ptr(ah), int(ah.shape[1]))
    _lib.check(_lib.lib().tg_cv_area_u8(_ptr(images), B, hs, ws, hd, wd, *tables, rows, _ptr(out), _SRC[dtype], _ptr(u8_out), _stream()))
    return out if u8_out is None else (out, u8_out)


def cv_linear_u8(images, size, invert=False, dtype=None, u8_out=True, out=None):
    """``cv2.resize(map, (wd, hd), interpolation=cv2.INTER_LINEAR)`` (no antialiasing, either direction) of a uint8 ``[B, hs, ws, 3]`` map whose three
    channels are equal (``lineart_conv7_out``'s; channel 0 is read), ``size`` = (hd, wd).  ``invert``: the map holds ``255 - t``; the kernel resizes ``t``
    and stores ``255 - result`` (the annotator's order: the fixed-point rounding does not commute with the inversion).  Outputs: ``u8_out`` (True to
    allocate, a tensor, or None / False) uint8 ``[B, hd, wd, 3]``; with ``dtype`` (or ``out``) also ``byte / 255`` as NCHW ``[B, 3, hd, wd]`` in bf16 /
    fp16 / fp32, the control image.  Returns the uint8 tensor, the float tensor, or ``(uint8, float)`` when both are asked for.  See tg_cv_linear_u8."""
    from . import cv_resize
    _need_cuda(images)
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] != 3:
        raise ValueError(f"cv_linear_u8: uint8 [B, H, W, 3] expected, got {images.dtype} {tuple(images.shape)}")
    B, hs, ws, _ = (int(v) for v in images.shape)
    hd, wd = int(size[0]), int(size[1])
    if out is not None:
        dtype = out.dtype
    if dtype is not None and dtype not in _SRC:
        raise RuntimeError(f"theatergen_amd: cv_linear_u8 writes bf16 / fp16 / fp32, not {dtype}")
    images = images.contiguous()
    if u8_out is True:
        u8_out = torch.empty((B, hd, wd, 3), dtype=torch.uint8, device=images.device)
    elif u8_out is False:
        u8_out = None
    elif u8_out is not None and (tuple(u8_out.shape) != (B, hd, wd, 3) or u8_out.dtype != torch.uint8 or not u8_out.is_contiguous()
                                 or u8_out.device != images.device):
        raise ValueError(f"cv_linear_u8: u8_out must be a contiguous uint8 tensor of shape {(B, hd, wd, 3)} on the images' device")
    if dtype is not None and out is None:
        out = torch.empty((B, 3, hd, wd), dtype=dtype, device=images.device)
    elif out is not None and (tuple(out.shape) != (B, 3, hd, wd) or not out.is_contiguous() or out.device != images.device):
        raise ValueError(f"cv_linear_u8: out must be a contiguous tensor of shape {(B, 3, hd, wd)} on the images' device")
    if u8_out is None and out is None:
        raise ValueError("cv_linear_u8: no output asked for (u8_out, dtype / out, or both)")
    (_, tv), (_, th) = cv_resize.device_linear_plan(hs, hd, images.device), cv_resize.device_linear_plan(ws, wd, images.device)
    _lib.check(_lib.lib().tg_cv_linear_u8(_ptr(images), B, hs, ws, hd, wd, _ptr(tv), _ptr(th), 1 if invert else 0, _ptr(u8_out), _ptr(out),
                                          _SRC[dtype] if dtype is not None else 0, _stream()))
    if u8_out is None:
        return out
    return u8_out if out is None else (u8_out, out)


def blend_latents(bg, fg, mask, ratio, sigma=1.0, storage_dtype=None):
    """fp32 in / out; ``storage_dtype`` torch.float16 / torch.bfloat16: reproduce the half-precision roundings of the
    reference expression (its latents are ``unet.dtype`` tensors)"""
    out = torch.empty_like(bg)
    hw = bg.shape[-1] * bg.shape[-2]
    sd = {None: -1, torch.float32: -1, torch.bfloat16: _lib.TG_BF16, torch.float16: _lib.TG_F16}[storage_dtype]
    _lib.check(_lib.lib().tg_blend_latents(_ptr(bg), _ptr(fg), _ptr(mask), bg.numel() // hw, hw, float(ratio), float(sigma),
                                           sd, _ptr(out), _stream()))
    return out


def gaussian_sample(moments, noise, scale=1.0):
    """moments fp32 [B, 2C, h, w] -> scale * (mean + std * noise) fp32 [B, C, h, w]; ``noise`` None = the mode"""
    B, C2, h, w = moments.shape
    out = torch.empty((B, C2 // 2, h, w), dtype=torch.float32, device=moments.device)
    _lib.check(_lib.lib().tg_gaussian_sample(_ptr(moments), _ptr(noise), B, C2 // 2, h * w, float(scale), _ptr(out), _stream()))
    return out


def add_noise(x0, noise, ca, cb):
    """out[s] = ca[s] * x0 + cb[s] * noise for a table of `steps` coefficients (fp32)"""
    steps = ca.numel()
    out = torch.empty((steps, *x0.shape), dtype=torch.float32, device=x0.device)
    _lib.check(_lib.lib().tg_add_noise(_ptr(x0), _ptr(noise), _ptr(ca), _ptr(cb), steps, x0.numel(), _ptr(out), _stream()))
    return out


def shift(src, dx, dy):
    h, w = src.shape[-2:]
    out = torch.empty_like(src)
    _lib.check(_lib.lib().tg_shift(_ptr(src), src.numel() // (h * w), h, w, int(dx), int(dy), _ptr(out), _stream()))
    return out


def masked_compose_(dst, src, mask):
    hw = dst.shape[-1] * dst.shape[-2]
    _lib.check(_lib.lib().tg_masked_compose(_ptr(dst), _ptr(src), _ptr(mask), dst.numel() // hw, hw, _stream()))
    return dst


def guidance_topk(attn, token, mask, k_fg, k_bg, fg_w, bg_w, scale, out, grad=None):
    for t in (attn, mask, out, grad):
        if t is not None:
            _need_cuda(t)
    heads, hw, n_tok = attn.shape
    _lib.check(_lib.lib().tg_guidance_topk(_ptr(attn), heads, hw, n_tok, int(token), _ptr(mask), int(k_fg), int(k_bg),
                                           float(fg_w), float(bg_w), float(scale), _ptr(out), _ptr(grad), _stream()))


def guidance_ref(attn, token, ref, mask, eps, scale, out, grad=None):
    """attn fp32 [heads, hw, tokens]; ref fp32 [heads, hw] contiguous"""
    for t in (attn, ref, mask, out, grad):
        if t is not None:
            _need_cuda(t)
    heads, hw, n_tok = attn.shape
    if ref.dtype != torch.float32 or ref.numel() != heads * hw or not ref.is_contiguous():
        raise RuntimeError("guidance_ref: ref must be a contiguous fp32 [heads, hw] column")
    _lib.check(_lib.lib().tg_guidance_ref(_ptr(attn), heads, hw, n_tok, int(token), _ptr(ref), _ptr(mask), float(eps),
                                          float(scale), _ptr(out), _ptr(grad), _stream()))


def guidance_ratio(attn, token, mask, scale, out, grad=None):
    for t in (attn, mask, out, grad):
        if t is not None:
            _need_cuda(t)
    heads, hw, n_tok = attn.shape
    _lib.check(_lib.lib().tg_guidance_ratio(_ptr(attn), heads, hw, n_tok, int(token), _ptr(mask), float(scale), _ptr(out),
                                            _ptr(grad), _stream()))


# ---- input-gradient kernels (latent_backward_guidance) ------------------------------------------------------------------
def groupnorm_bwd(x, dy, batch, hw, groups, eps, gamma, beta, silu=False):
    _need_cuda(x)
    dx = torch.empty_like(x)
    L = _lib.lib()
    scratch = workspace(L.tg_groupnorm_bwd_scratch_bytes(int(batch), int(hw), int(groups)), x.device)
    _lib.check(L.tg_groupnorm_bwd(_dt(x), _ptr(x), _ptr(dy), int(batch), int(hw), x.shape[-1], int(groups), float(eps), _ptr(gamma),
                                  _ptr(beta), 1 if silu else 0, _ptr(dx), _ptr(scratch), _stream()))
    return dx


def layernorm_bwd(x, dy, gamma, eps=1e-5):
    _need_cuda(x)
    rows, Cc = x.shape
    dx = torch.empty_like(x)
    _lib.check(_lib.lib().tg_layernorm_bwd(_dt(x), _ptr(x), _ptr(dy), rows, Cc, float(eps), _ptr(gamma), _ptr(dx), _stream()))
    return dx


def geglu_bwd(h, dg):
    rows, two_inner = h.shape
    dh = torch.empty_like(h)
    _lib.check(_lib.lib().tg_geglu_bwd(_dt(h), _ptr(h), _ptr(dg), rows, two_inner // 2, _ptr(dh), _stream()))
    return dh


def softmax_bwd_rows(probs, dprobs, length, scale, ld_out, extra=None, want_probs=False):
    """probs fp32 or storage dtype [rows, >= length] (row pitch probs.stride(0)), dprobs storage dtype [rows, >= length];
    -> dS [rows, ld_out] (and P in the storage dtype, same shape, when ``want_probs``)"""
    rows = probs.shape[0]
    if probs.dtype != torch.float32 and probs.dtype != dprobs.dtype:
        raise RuntimeError("softmax_bwd_rows: probs must be fp32 or the storage dtype")
    ds = torch.empty((rows, ld_out), dtype=dprobs.dtype, device=dprobs.device)
    pout = torch.empty_like(ds) if want_probs else None
    _lib.check(_lib.lib().tg_softmax_bwd_rows(_dt(dprobs), _ptr(probs), 1 if probs.dtype == torch.float32 else 0, probs.stride(0),
                                              _ptr(dprobs), dprobs.stride(0), _ptr(extra),
                                              extra.stride(0) if extra is not None else 0, rows, int(length), float(scale), _ptr(ds),
                                              _ptr(pout), int(ld_out), _stream()))
    return (ds, pout) if want_probs else ds


def sumpool2x2(du, batch, h, w):
    """du token-major [batch * 2h * 2w, C] -> [batch * h * w, C]"""
    Cc = du.shape[-1]
    out = torch.empty((batch * h * w, Cc), dtype=du.dtype, device=du.device)
    _lib.check(_lib.lib().tg_sumpool2x2(_dt(du), _ptr(du), int(batch), int(h), int(w), Cc, _ptr(out), _stream()))
    return out


def capturing_now():
    """True while the current stream is being captured into a hipGraph"""
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


class GuidanceBatch:
    """Collects the terms of one ``compute_ca_lossv3`` call (one per attention map x object x token position) and evaluates
    them with ONE ``tg_guidance_plan_run`` launch pair (+ an in-order fold) instead of one dependent launch each.

    Round 3: the device-side item table holds SLOT indices, not pointers; the call's tensors (maps, gradients, masks, reference
    columns) are passed as kernel arguments.  The table therefore only depends on (kinds, shapes, token positions, top-k sizes,
    weights, which tensor goes with which) and is cached on the device, keyed by exactly that — a steady-state call makes NO host ->
    device copy (the round-2 path built and uploaded a pointer table per call: most of its 1.3 ms at BASELINE configs[3]) and can
    be captured in a hipGraph.

    Terms whose gradient columns would collide (same grad tensor and token in one call: two objects sharing a token position, or a
    reference-attention term next to the box term of the same key and token) are deferred to a following launch, so the
    order of additions into the loss is LAUNCH-MAJOR, item order within each launch — fixed and deterministic for a given
    call, identical to the per-term launches whenever no column collides (the shipped flow), one fp32 re-association otherwise."""
    KIND_TOPK, KIND_RATIO, KIND_REF = 0, 1, 2
    _tables = {}            # (device index, item signature) -> (device table tensor, n_items, max_hw_topk, max_heads)
    _TABLES_MAX = 128
    _pinned = {}            # entries a stream CAPTURE has read: a captured hipGraph bakes the table's device address, so they are never
                            # evicted (a 64-byte row per term; ADVICE r3: the FIFO above recycled tables under still-cached graphs)

    def __init__(self, device):
        self.device = device
        self.items = []

    def add(self, kind, attn, token, mask, scale, grad=None, ref=None, k_fg=0, k_bg=0, fg_w=0.0, bg_w=0.0, eps=0.0):
        heads, hw, n_tok = attn.shape
        for t in (attn, grad, mask, ref):             # raw device pointers go to the kernel: a host tensor would fault the GPU
            if t is not None:
                _need_cuda(t)
                if t.dtype != torch.float32 or not t.is_contiguous():
                    raise RuntimeError("guidance: attention maps, gradients, masks and reference columns must be contiguous fp32")
        if not (0 <= int(token) < n_tok):
            raise RuntimeError(f"guidance: token position {token} outside the {n_tok} text tokens")
        if kind == self.KIND_TOPK and not (1 <= k_fg <= hw and 1 <= k_bg <= hw):
            raise RuntimeError("guidance: top-k size out of range")
        if mask.numel() != hw or (ref is not None and ref.numel() != heads * hw) or (grad is not None and grad.numel() != attn.numel()):
            raise RuntimeError("guidance: mask / reference / gradient shape does not match the attention map")
        self.items.append(dict(kind=int(kind), attn=attn, grad=grad, mask=mask, ref=ref, heads=int(heads), hw=int(hw), n_tok=int(n_tok),
                               token=int(token), k_fg=int(k_fg), k_bg=int(k_bg), fg_w=float(fg_w), bg_w=float(bg_w), scale=float(scale),
                               eps=float(eps)))

    def _launch(self, now, loss):
        slots, index = [], {}

        def slot(t):
            if t is None:
                return -1
            key = t.data_ptr()
            if key not in index:
                index[key] = len(slots)
                slots.append(t)
            return index[key]
        rows = []
        for it in now:
            rows.append((slot(it["attn"]), slot(it["grad"]), slot(it["mask"]), slot(it["ref"]), it["heads"], it["hw"], it["n_tok"], it["token"],
                         it["kind"], it["k_fg"], it["k_bg"], it["fg_w"], it["bg_w"], it["scale"], it["eps"]))
        if len(slots) > _lib.GUIDANCE_MAX_SLOTS:
            half = len(now) // 2                      # more distinct tensors than argument slots: two launches (item order is kept)
            self._launch(now[:half], loss)
            self._launch(now[half:], loss)
            return
        key = (self.device.index, tuple(rows))
        capturing = capturing_now()
        hit = GuidanceBatch._pinned.get(key) or GuidanceBatch._tables.get(key)
        if hit is None:
            if capturing:
                raise RuntimeError("guidance: this term layout has no device table yet and a stream capture is in progress (the upload "
                                   "cannot be captured): run the same call once eagerly before capturing it")
            arr = (_lib.GuidancePItem * len(rows))()
            for a, r in zip(arr, rows):
                (a.attn_slot, a.grad_slot, a.mask_slot, a.ref_slot, a.heads, a.hw, a.n_tok, a.token, a.kind, a.k_fg, a.k_bg,
                 a.fg_w, a.bg_w, a.scale, a.eps) = r
            table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.device)     # once per signature
            hit = (table, len(rows), max([r[5] for r in rows if r[8] == self.KIND_TOPK] + [0]), max(r[4] for r in rows))
            if len(GuidanceBatch._tables) >= GuidanceBatch._TABLES_MAX:
                GuidanceBatch._tables.pop(next(iter(GuidanceBatch._tables)))
            GuidanceBatch._tables[key] = hit
        if capturing:
            GuidanceBatch._pinned[key] = hit
        table, n, max_hw, max_heads = hit
        ptrs = (C.c_void_p * len(slots))(*[t.data_ptr() for t in slots])
        head_terms = torch.empty(n * max_heads, dtype=torch.float32, device=self.device)
        _lib.check(_lib.lib().tg_guidance_plan_run(table.data_ptr(), n, max_hw, max_heads, ptrs, len(slots), head_terms.data_ptr(), _ptr(loss),
                                                   _stream()))

    def flush(self, loss):
        """loss: fp32 device tensor [1], accumulated in place (launch-major, item order within a launch)"""
        items, self.items = self.items, []
        while items:
            seen, now, later = set(), [], []
            for it in items:
                col = (it["grad"].data_ptr(), it["token"]) if it["grad"] is not None else None
                if col is not None and col in seen:
                    later.append(it)              # keeps item order within each launch; collisions go to the next one
                else:
                    if col is not None:
                        seen.add(col)
                    now.append(it)
            self._launch(now, loss)
            items = later
        # eager launches pin nothing beyond the last launch: every tensor is used on the current stream only, and the caching allocator
        # hands a freed block back to that same stream (stream-ordered reuse).  Under a stream capture the item table is pinned above,
        # the box masks by guidance._box_mask, and the per-call tensors (maps, gradients, head terms) live in the graph's private pool.
        return loss
