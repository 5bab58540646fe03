"""tests/golden/gemm_routes.npz: what the tg_gemm planner answers for 12,586 descriptors under 18 settings of its dev knobs.

    THEATERGEN_HIP_LIB=<library of the commit to pin> python tests/golden/make_gemm_routes.py

The stored file was recorded with the library of the commit BEFORE the planner moved into csrc/tg_gemm_route.hip (91294af; that library lacks
``tg_gemm_kernel_name``, so it loads with THEATERGEN_HIP_ABI_COMPAT=308).  tests/test_gemm_route_cpu.py replays the enumeration below against the
current library.  Host logic only: pointers are fake aligned integers, nothing is launched.  Regenerate only when a planner change is intended, and say
so in that change.
"""
import ctypes as C
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PATH = os.path.join(ROOT, "tests", "golden", "gemm_routes.npz")
KNOBS = ("TG_GEMM_FLAGS", "TG_PP", "TG_T160", "TG_T64_MAX", "TG_T3_MAX", "TG_T7_MAXK", "TG_T7_FIT", "TG_SLAB_PP")
ENVS = [{}] + [{"TG_GEMM_FLAGS": v} for v in ("8", "128", "1024", "2048", "4096")] + [{"TG_PP": v} for v in ("0", "1", "7")] + \
    [{"TG_T160": v} for v in ("0", "3")] + [{"TG_T64_MAX": "0"}, {"TG_T3_MAX": "0"}, {"TG_T7_MAXK": "0"}, {"TG_T7_FIT": "1"}] + \
    [{"TG_SLAB_PP": v} for v in ("0", "1", "2")]
# per row: (rc, tile_m, tile_n, splits, kernel_kind, workspace_bytes, gn_partial_blocks); the plan columns are 0 where rc != 0
COLUMNS = (("rc", np.int8), ("tile_m", np.int16), ("tile_n", np.int16), ("splits", np.int8), ("kernel_kind", np.int8),
           ("workspace_bytes", np.int64), ("gn_partial_blocks", np.int16))


def _base(_lib):
    d = _lib.GemmDesc()
    d.dtype = 0
    d.a0 = d.w = d.out = 16
    d.out_scale = 1.0
    return d


def gemm_descs(_lib):
    """mode 0: shapes x epilogue / operand variants, then every force_tile on five problems"""
    Ms = [64, 128, 300, 512, 1024, 2048, 4096, 4608, 8192, 16384, 65536]
    Ns = [64, 128, 320, 640, 960, 1280, 1920, 2560, 3840, 5120, 10240]
    Ks = [64, 320, 640, 1280, 2560, 5120]
    variants = ["plain", "geglu", "act", "ln", "ln_rows", "ln_rows_geglu", "nsplit", "ln_rows_nsplit", "res8", "a1", "split2", "pitch"]
    for M, N, K, v in itertools.product(Ms, Ns, Ks, variants):
        d = _base(_lib)
        d.mode, d.c0, d.M, d.N, d.K, d.ldc = 0, K, M, N, K, N
        if "geglu" in v:
            d.geglu, d.ldc = 1, N // 2
        if v == "act":
            d.act = 1
        if v.startswith("ln"):
            d.ln_u, d.ln_v, d.ln_eps = 64, 64, 1e-5
        if "rows" in v:
            d.ln_rows = 64
        if "nsplit" in v:                        # q | k | v^T: the last third leaves transposed
            if N % 3:
                continue
            d.n_split, d.out_t, d.rows_per_batch = 2 * N // 3, 16, (M // 2 if M % 2 == 0 else M)
            d.ldt, d.ldc = d.rows_per_batch, d.n_split
        if v == "res8":                          # 8-byte aligned residual: no LDS-transposed epilogue, no ping-pong tiles
            d.res, d.ldres = 8, N
        if v == "a1":
            d.a1, d.c0, d.c1 = 16, K // 2, K // 2
        if v == "split2":
            d.force_split_k = 2
        if v == "pitch":
            d.lda = d.ldw = K + 64
        yield d
    for ft in range(1, 27):
        for M, N, K, g in [(512, 512, 640, 0), (512, 320, 640, 0), (4096, 1280, 1280, 0), (16384, 2560, 320, 1), (300, 512, 640, 0)]:
            d = _base(_lib)
            d.mode, d.c0, d.M, d.N, d.K, d.ldc, d.geglu, d.force_tile = 0, K, M, N, K, (N // 2 if g else N), g, ft
            yield d


def conv_descs(_lib):
    """mode 1: batch x side x channels x variants"""
    variants = ["plain", "c1", "s2", "up", "coef", "gn", "ft11", "ft12", "ft11s3", "split2"]
    for b, hw, cin, cout, v in itertools.product([1, 2, 4, 16], [8, 12, 16, 24, 32, 40, 48, 64, 96, 128], [320, 640, 1280], [128, 320, 640, 1280], variants):
        d = _base(_lib)
        d.mode, d.c0 = 1, cin
        st, up = (2 if v == "s2" else 1), (1 if v == "up" else 0)
        if v == "c1":
            d.a1, d.c1 = 16, cin
        oh = 2 * hw if up else (hw + 2 - 3) // st + 1
        d.batch, d.in_h, d.in_w, d.out_h, d.out_w, d.stride, d.upsample = b, hw, hw, oh, oh, st, up
        d.M, d.N, d.K, d.ldc = b * oh * oh, cout, 9 * (cin + d.c1), cout
        if v == "coef":
            d.a_coef = 16
        if v == "gn":
            d.out_gn_groups = 32
        if v in ("ft11", "ft11s3"):
            d.force_tile = 11
        if v == "ft12":
            d.force_tile = 12
        if v == "ft11s3":
            d.force_split_k = 3
        if v == "split2":
            d.force_split_k = 2
        yield d


def sweep(_lib, setenv):
    """-> {column: array [len(ENVS), descriptors]}; ``setenv(dict)`` installs one knob setting (every knob absent from it unset)"""
    h = _lib.lib()
    descs = list(itertools.chain(gemm_descs(_lib), conv_descs(_lib)))
    rows = np.zeros((len(ENVS), len(descs), len(COLUMNS)), dtype=np.int64)
    tm, tn, sp, kk = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    for e, env in enumerate(ENVS):
        setenv(env)
        for i, d in enumerate(descs):
            rc = h.tg_gemm_plan(C.byref(d), C.byref(tm), C.byref(tn), C.byref(sp), C.byref(kk))
            plan = (tm.value, tn.value, sp.value, kk.value) if rc == 0 else (0, 0, 0, 0)
            rows[e, i] = (rc,) + plan + (h.tg_gemm_workspace_bytes(C.byref(d)), h.tg_gemm_gn_partial_blocks(C.byref(d)))
    return {name: rows[:, :, c] for c, (name, _) in enumerate(COLUMNS)}


def _setenv(env):
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from theatergen_amd import _lib
    got = sweep(_lib, _setenv)
    out = {}
    for name, dt in COLUMNS:
        out[name] = got[name].astype(dt)
        assert np.array_equal(out[name], got[name]), name
    np.savez_compressed(PATH, envs=np.array([json.dumps(e, sort_keys=True) for e in ENVS]), **out)
    kinds = sorted(set(zip(out["rc"].ravel().tolist(), out["tile_m"].ravel().tolist(), out["tile_n"].ravel().tolist(), out["kernel_kind"].ravel().tolist())))
    print(f"{out['rc'].size} rows ({out['rc'].shape[1]} descriptors x {len(ENVS)} knob settings), {int((out['rc'] != 0).sum())} refusals, "
          f"{len(kinds)} (rc, tile, kind) outcomes, {os.path.getsize(PATH)} bytes from {_lib.LIB_PATH}")
