"""Launch-by-launch checks of ``ops.gemm`` / ``ops.attention`` against their C-ABI contracts (tests/gemm_contract.py), for GPU tests
that run whole production plans (test_launch_replay_gpu.py) or hand-made edge descriptors (test_gemm_edges_gpu.py).

``LaunchChecker.install(monkeypatch)`` replaces ``ops.gemm`` and ``ops.attention`` (every caller looks them up as module attributes) with
wrappers that, on EVERY launch (synchronising before and after it):
  * check that each operand's read region lies inside its tensor's storage, that a0 / a1 / w are 16-byte aligned, and that no written
    element of out / out_t is read by the same launch (the one exception: ``res`` IS ``out``, same pointer and pitch: the in-place
    residual GEMMs of the reverse pass);
  * snapshot the storages of out / out_t and check afterwards that every element outside the written region kept its bits;
and on the FIRST launch of each distinct key (kernel plan, sizes, conv geometry, optional fields, epilogue path, in-place residual):
  * compare the output with the fp64 reference (``gemm_contract.check``: l2_tol / rel_tol of test_kernels_gpu.py, attention at its 1.5x);
    ``ln_rows`` against the fp64 row statistics; ``gn_out`` partial sums against those of the kernel's own output (rtol 2e-5);
  * replay the call with out / out_t / gn partials in fresh NaN-filled buffers and the K-split workspace in a slot of its own filled with
    NaN: the replay must reproduce the production output bit for bit (determinism, every element written, nothing read from stale memory).
Other ops entry points are only counted (``unwrapped``).
"""
import collections
import contextlib
import json
import os

import torch

from tests import gemm_contract as gc
from tests import parity_metrics as pm

REPLAY_SLOT = 61
UNWRAPPED = {
    "row chains": ("rc_linear", "rc_xattn", "rc_ff", "rc_front", "rc_kv_pack"),
    "xq_attn": ("xq_attn", "xq_kv_pack"),
    "skinny": ("skinny_gemm",),
    "GroupNorm / LayerNorm": ("groupnorm", "groupnorm_coef", "groupnorm_from_partials", "layernorm", "layernorm_stats"),
    "conv_in / conv_out": ("conv_in", "conv_out", "conv1x1_nchw"),
    "elementwise": ("act", "add", "geglu", "transpose", "softmax_rows", "timestep_embedding", "gaussian_sample"),
    "guidance": ("guidance_topk", "guidance_ratio", "guidance_ref"),
    "attention backward": ("attention_bwd", "attention_bwd_cross", "groupnorm_bwd", "layernorm_bwd", "geglu_bwd", "softmax_bwd_rows",
                           "sumpool2x2", "attn_probs"),
}


def l2_tol(dtype):
    return 3.0e-3 if dtype == torch.bfloat16 else 4.0e-4


def rel_tol(dtype):
    return 1.0e-2 if dtype == torch.bfloat16 else 2.5e-3


def _al16(t):
    return t is None or t.data_ptr() % 16 == 0


def epi_lds(a):
    """Python statement of tg_gemm.hip::epi_lds_of: the LDS-transposed epilogue (and the ping-pong tiles) need these"""
    N, out = int(a["N"]), a["out"]
    ns = int(a.get("n_split") or 0)
    return (N % 8 == 0 and out.stride(0) % 8 == 0 and all(_al16(a.get(k)) for k in ("out", "bias", "bvec", "res"))
            and (a.get("bvec") is None or a["bvec"].stride(0) % 8 == 0) and (a.get("res") is None or a["res"].stride(0) % 8 == 0)
            and (ns == 0 or ns % 64 == 0))


def _bytes(t):
    """uint8 tensor over t's whole storage"""
    st = t.untyped_storage()
    b = torch.empty(0, dtype=torch.uint8, device=t.device)
    b.set_(st, 0, (st.nbytes(),), (1,))
    return b


def _sptr(t):
    return t.untyped_storage().data_ptr()


@contextlib.contextmanager
def _nan_empty():
    """torch.empty hands out NaN-filled floating tensors (the gn partials ops.gemm allocates itself)"""
    real = torch.empty

    def empty(*args, **kw):
        t = real(*args, **kw)
        if t.is_floating_point():
            t.fill_(float("nan"))
        return t
    torch.empty = empty
    try:
        yield
    finally:
        torch.empty = real


class LaunchChecker:
    def __init__(self, label=""):
        from theatergen_amd import ops
        self.ops = ops
        self.label = label
        self.orig_gemm, self.orig_attention = ops.gemm, ops.attention
        self.counts = collections.Counter()              # key -> launches
        self.metrics = {}                                # key -> metrics of its checked launch
        self.families = collections.Counter()
        self.kinds = {}                                  # key -> kernel kind label
        self.unwrapped = collections.Counter()
        self.launches = 0

    # ---- installation ----------------------------------------------------------------------------------------------------------------
    def install(self, monkeypatch):
        monkeypatch.setattr(self.ops, "gemm", self.gemm)
        monkeypatch.setattr(self.ops, "attention", self.attention)
        for fam, names in UNWRAPPED.items():
            for n in names:
                if hasattr(self.ops, n):
                    monkeypatch.setattr(self.ops, n, self._counted(fam, getattr(self.ops, n)))
        if hasattr(self.ops, "GuidanceBatch"):
            orig_flush = self.ops.GuidanceBatch.flush
            checker = self

            def flush(gb, loss):
                checker.unwrapped["guidance"] += 1
                return orig_flush(gb, loss)
            monkeypatch.setattr(self.ops.GuidanceBatch, "flush", flush)
        return self

    def _counted(self, fam, fn):
        def wrapped(*args, **kw):
            self.unwrapped[fam] += 1
            return fn(*args, **kw)
        return wrapped

    # ---- shared pieces ---------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _check_reads(reads, what):
        for r in reads:
            rng = r.byte_range()
            if rng is None:
                continue
            nbytes = r.t.untyped_storage().nbytes()
            assert 0 <= rng[0] and rng[1] <= nbytes, f"{what}: operand {r.name} reads bytes [{rng[0]}, {rng[1]}) of a {nbytes}-byte storage"

    @staticmethod
    def _write_masks(writes):
        masks = {}
        for w in writes:
            sp = _sptr(w.t)
            if sp not in masks:
                masks[sp] = (w.t, torch.zeros(w.t.untyped_storage().nbytes(), dtype=torch.bool, device=w.t.device))
            w.byte_view(masks[sp][1]).fill_(True)
        return masks

    @staticmethod
    def _check_overlap(masks, reads, what, allowed=()):
        for r in reads:
            if r.name in allowed or _sptr(r.t) not in masks:
                continue
            hit = bool(r.byte_view(masks[_sptr(r.t)][1]).any())
            assert not hit, f"{what}: operand {r.name} overlaps the region this launch writes"

    @staticmethod
    def _snapshot(masks):
        return {sp: _bytes(t).clone() for sp, (t, _) in masks.items()}

    @staticmethod
    def _check_outside(masks, snaps, what):
        for sp, (t, m) in masks.items():
            now = _bytes(t)
            changed = (now != snaps[sp]) & ~m
            n = int(changed.sum())
            assert n == 0, f"{what}: {n} bytes outside the written region of {tuple(t.shape)} changed (first at byte " \
                           f"{int(changed.nonzero()[0])})"

    @staticmethod
    def _fresh(writes, snaps, keep):
        """NaN-filled replacement storages for the written tensors (same byte offset, so the same alignment); ``keep``: storages whose
        pre-launch bytes are copied in instead (res IS out)"""
        new, views = {}, {}
        for w in writes:
            sp = _sptr(w.t)
            if sp not in new:
                nb = w.t.untyped_storage().nbytes()
                buf = torch.empty(nb // w.t.element_size(), dtype=w.t.dtype, device=w.t.device)
                if sp in keep:
                    _bytes(buf).copy_(snaps[sp])
                else:
                    buf.fill_(float("nan"))
                new[sp] = buf
            views[w.name] = new[sp].as_strided(w.t.shape, w.t.stride(), w.t.storage_offset())
        return views

    def _record_key(self, key, kind, fams):
        self.counts[key] += 1
        self.launches += 1
        new = self.counts[key] == 1
        if new:
            self.kinds[key] = kind
            for f in fams:
                self.families[f] += 1
        return new

    # ---- GEMM ------------------------------------------------------------------------------------------------------------------------
    def gemm_key(self, a, plan):
        tm, tn, sp, kk = plan
        opt = tuple(k for k in ("a1", "bias", "bvec", "res", "a_coef", "ln", "gn_out", "out_t") if a.get(k) is not None)
        opt += tuple(f"{k}={a[k]}" for k in ("act", "geglu", "a_silu", "n_split", "a_rows_per_batch", "lda", "ldw", "pad_mode") if a.get(k))
        if a.get("ln") is not None and len(a["ln"]) > 3 and a["ln"][3] is not None:
            opt += ("ln_rows",)
        if float(a.get("out_scale", 1.0)) != 1.0:
            opt += ("out_scale",)
        conv = tuple(int(v) for v in a["conv"]) if a.get("conv") is not None else None
        res_is_out = a.get("res") is not None and a["res"].data_ptr() == a["out"].data_ptr() and a["res"].stride(0) == a["out"].stride(0)
        return (str(a["a0"].dtype).replace("torch.", ""), f"plan={tm}x{tn}/s{sp}/k{kk}", f"MNK={a['M']}x{a['N']}x{a['K']}", f"mode={a.get('mode', 0)}",
                f"conv={conv}", "+".join(opt), f"epi_lds={epi_lds(a)}", f"res_is_out={res_is_out}"), res_is_out

    @staticmethod
    def gemm_families(a, plan, res_is_out):
        tm, tn, sp, kk = plan
        f = [f"kind{kk}"]
        if kk == 4 and sp > 1:
            ow = int(a["conv"][4])
            f.append("slab_split_whole_row" if ow in (16, 32, 64) else "slab_split_patch")
        if kk == 4:
            ow = int(a["conv"][4])
            f.append("slab_whole_row" if ow in (16, 32, 64) else "slab_patch")
        if kk == 7:
            f.append(f"pp{tn}")
        if a.get("gn_out") is not None:
            f.append("gn_out_asked")
        if a.get("ln") is not None:
            f.append("ln_fold_rows" if len(a["ln"]) > 3 and a["ln"][3] is not None else "ln_fold")
        for k in ("a_coef", "a1", "bvec"):
            if a.get(k) is not None:
                f.append({"a1": "two_source"}.get(k, k))
        for k in ("geglu", "pad_mode"):
            if a.get(k):
                f.append(k)
        if int(a.get("n_split") or 0) > 0:
            f.append("n_split")
        if int(a.get("a_rows_per_batch") or 0) > 0:
            f.append("batched_a")
        if int(a.get("lda") or 0) > 0 or int(a.get("ldw") or 0) > 0:
            f.append("padded_pitch")
        if a.get("conv") is not None and int(a["conv"][5]) == 2:
            f.append("stride2")
        if a.get("conv") is not None and int(a["conv"][6]):
            f.append("upsample")
        if res_is_out:
            f.append("res_is_out")
        if not epi_lds(a):
            f.append("epi_fallback")
        return f

    def gemm(self, *args, **kwargs):
        a = gc.gemm_args(args, kwargs, self.orig_gemm)
        if a["plan_only"]:
            return self.orig_gemm(**a)
        M, N, K, mode, c0, c1, n_split, geglu, n_main, rpb = gc._geometry(a)
        if a["out"] is None:
            a["out"] = torch.empty((M, n_main), dtype=a["a0"].dtype, device=a["a0"].device)
        plan = self.orig_gemm(**dict(a, plan_only=True))
        key, res_is_out = self.gemm_key(a, plan)
        what = f"{self.label} gemm {key}"
        torch.cuda.synchronize()
        reads, writes = gc.read_extents(a), gc.written_region(a)
        self._check_reads(reads, what)
        for r in writes:
            self._check_reads([r], what)
        for n in ("a0", "a1", "w"):
            assert _al16(a.get(n)), f"{what}: {n} is not 16-byte aligned"
        masks = self._write_masks(writes)
        self._check_overlap(masks, reads, what, allowed=("res",) if res_is_out else ())
        snaps = self._snapshot(masks)
        new = self._record_key(key, f"kind{plan[3]}", self.gemm_families(a, plan, res_is_out))
        ref = None
        if new:
            ref = gc.gemm_reference(**a)                      # before the launch: an in-place residual is overwritten by it
        out = self.orig_gemm(**a)
        torch.cuda.synchronize()
        assert out.data_ptr() == a["out"].data_ptr()
        self._check_outside(masks, snaps, what)
        if new:
            self._check_gemm(a, key, what, ref, writes, snaps, res_is_out, plan)
        return out

    def _check_gemm(self, a, key, what, ref, writes, snaps, res_is_out, plan):
        dtype = a["a0"].dtype
        views = {w.name: w.view() for w in writes}
        m = gc.check(views["out"], ref[0], f"launch {what}", l2_tol(dtype), rel_tol(dtype), record=False)
        if ref[1] is not None:
            mt = gc.check(views["out_t"], ref[1], f"launch {what} (out_t)", l2_tol(dtype), rel_tol(dtype), record=False)
            m = {k: max(m[k], mt[k]) if isinstance(m[k], float) else m[k] and mt[k] for k in m}
        ln = a.get("ln")
        if ln is not None and len(ln) > 3 and ln[3] is not None:
            mean, rstd = gc.ln_row_stats(a)
            st = ln[3].double()
            assert torch.allclose(st[:, 0], rstd, rtol=1e-4, atol=0), f"{what}: ln_rows rstd"
            err = (st[:, 1] + rstd * mean).abs() / torch.maximum((rstd * mean).abs(), rstd)
            assert float(err.max()) <= 1e-4, f"{what}: ln_rows -rstd * mean off by {float(err.max()):.2e}"
        gn = a.get("gn_out")
        if gn is not None and "partials" in gn:
            batch, hw = int(a["conv"][0]), int(a["conv"][3]) * int(a["conv"][4])
            want = gc.gn_partials_reference(views["out"], int(gn["groups"]), batch, hw)
            got = gn["partials"].double()
            assert torch.allclose(got, want, rtol=2e-5, atol=2e-3), f"{what}: gn partials off by {(got - want).abs().max().item():.3e}"
            self.families["gn_out_written"] += 1
        # replay on fresh NaN-filled outputs and a NaN-filled workspace of its own
        fresh = self._fresh(writes, snaps, keep={_sptr(a["out"])} if res_is_out else set())
        b = dict(a, out=fresh["out"])
        if "out_t" in fresh:
            b["out_t"] = fresh["out_t"]
        if res_is_out:
            b["res"] = fresh["out"]
        if gn is not None:
            b["gn_out"] = {"groups": gn["groups"]}
        tm, tn, sp, kk = plan
        M, N = int(a["M"]), int(a["N"])
        with self.ops.workspace_slot(REPLAY_SLOT):
            if sp > 1:
                ws = self.ops.workspace(-(-M // tm) * -(-N // tn) * sp * tm * tn * 4, a["a0"].device)
                ws.fill_(float("nan"))
            with _nan_empty():
                self.orig_gemm(**b)
        torch.cuda.synchronize()
        for w in writes:
            got, want = fresh[w.name], views[w.name]
            rv = gc.Region(w.name, got, 0, w.sizes, w.strides).view()
            same = torch.equal(rv.view(torch.int16), want.view(torch.int16)) and not bool(torch.isnan(rv).any())
            assert same, f"{what}: the replay on NaN-filled {w.name} / workspace differs from the production launch"
        if gn is not None and "partials" in gn:
            assert torch.equal(b["gn_out"]["partials"], gn["partials"]), f"{what}: gn partials of the replay differ"
        self.metrics[key] = m

    # ---- attention -------------------------------------------------------------------------------------------------------------------
    def attention(self, *args, **kwargs):
        a = gc.attention_args(args, kwargs, self.orig_attention)
        mask = a.get("mask")
        key = (str(a["q"].dtype).replace("torch.", ""), f"B={a['batch']}", f"H={a['heads']}", f"D={a['head_dim']}", f"nq={a['n_q']}",
               f"len0={a['len0']}", f"len1={a['len1']}", f"causal={bool(a.get('causal'))}", f"mask={None if mask is None else tuple(mask.shape)}",
               f"w1_dev={a.get('w1_dev') is not None}")
        what = f"{self.label} attention {key}"
        fams = ["attention"]
        if int(a["len0"]) == int(a["n_q"]) and int(a["n_q"]) >= 4096:
            fams.append("attn_self_n>=4096")
        if int(a["len1"]) > 0:
            fams.append("attn_two_segments")
        if mask is not None:
            fams.append("attn_mask")
        if a.get("causal"):
            fams.append("attn_causal")
        torch.cuda.synchronize()
        reads, writes = gc.attention_read_extents(a), gc.attention_written_region(a)
        self._check_reads(reads + writes, what)
        masks = self._write_masks(writes)
        self._check_overlap(masks, reads, what)
        snaps = self._snapshot(masks)
        new = self._record_key(key, "attention", fams)
        out = self.orig_attention(**a)
        torch.cuda.synchronize()
        self._check_outside(masks, snaps, what)
        if new:
            dtype = a["q"].dtype
            ref = gc.attention_reference(**a)
            got = writes[0].view()
            m = gc.check(got, ref, f"launch {what}", 1.5 * l2_tol(dtype), 1.5 * rel_tol(dtype), record=False)
            fresh = self._fresh(writes, snaps, keep=set())
            self.orig_attention(**dict(a, out=fresh["out"]))
            torch.cuda.synchronize()
            rv = gc.Region("out", fresh["out"], 0, writes[0].sizes, writes[0].strides).view()
            same = torch.equal(rv.view(torch.int16), got.view(torch.int16)) and not bool(torch.isnan(rv).any())
            assert same, f"{what}: the replay on a NaN-filled output differs from the production launch"
            self.metrics[key] = m
        return out

    # ---- report ----------------------------------------------------------------------------------------------------------------------
    def report(self):
        """record every checked key (with its occurrences) in parity_metrics.jsonl; -> summary dict"""
        worst = {}
        near = []
        for key, m in self.metrics.items():
            kind = self.kinds[key]
            dtype = torch.bfloat16 if key[0] == "bfloat16" else torch.float16
            f = 1.5 if kind == "attention" else 1.0
            pm.record(f"launch replay {self.label}: {' '.join(key)}", m, occurrences=self.counts[key], kind=kind,
                      l2_tol=f * l2_tol(dtype), max_tol=f * rel_tol(dtype))
            w = worst.setdefault(kind, {"rel_l2": 0.0, "max_rel": 0.0, "tile_rel_l2": 0.0})
            for k in w:
                w[k] = max(w[k], m[k])
            if m["rel_l2"] > 0.5 * f * l2_tol(dtype) or m["max_rel"] > 0.5 * f * rel_tol(dtype) or m["tile_rel_l2"] > f * l2_tol(dtype):
                near.append({"key": " ".join(key), **{k: m[k] for k in ("rel_l2", "max_rel", "tile_rel_l2")}})
        s = {"plan": self.label, "launches": self.launches, "distinct_keys": len(self.counts), "checked_keys": len(self.metrics),
             "families": dict(self.families), "worst_per_kind": worst, "within_2x_of_tolerance": near, "unwrapped": dict(self.unwrapped)}
        try:
            d = os.path.dirname(pm._LOG)                     # next to parity_metrics.jsonl
            os.makedirs(d, exist_ok=True)
            with open(os.path.join(d, "launch_replay_summary.jsonl"), "a") as fh:
                fh.write(json.dumps(s) + "\n")
        except OSError:
            pass
        print(json.dumps(s, indent=1))
        return s
