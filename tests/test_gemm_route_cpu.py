"""CPU: the tg_gemm planner (csrc/tg_gemm_route.hip) is host logic, so what it decides is pinned without a GPU.

  * every row of tests/golden/gemm_routes.npz — (rc, tile, splits, kernel_kind, workspace bytes, GroupNorm-partial blocks) for 12,586 descriptors under 18
    settings of the dev knobs, recorded with the library of the commit before the planner became one route — is reproduced;
  * ``ops.ln_qkv_takes_stats`` (does attn1's LayerNorm-folded q | k | v^T projection need a ``layernorm_stats`` launch first?) answers as the Python
    mirror of the planner it replaced did on the q | k | v^T shapes of the six launch-replay plans.
"""
import json
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_route_table_matches_the_recorded_planner(monkeypatch):
    from tests.golden import make_gemm_routes as gen
    from theatergen_amd import _lib
    gold = np.load(os.path.join(ROOT, "tests", "golden", "gemm_routes.npz"))
    assert gold["envs"].tolist() == [json.dumps(e, sort_keys=True) for e in gen.ENVS]

    def setenv(env):
        for k in gen.KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    got = gen.sweep(_lib, setenv)
    assert gold["rc"].shape == (18, 12586)
    for name, _ in gen.COLUMNS:
        want = gold[name].astype(np.int64)
        assert want.shape == got[name].shape, name
        bad = np.argwhere(want != got[name])
        assert bad.size == 0, f"{name}: {len(bad)} rows differ, first (knob setting, descriptor) = {bad[0].tolist()}: " \
                              f"{gen.ENVS[bad[0][0]]} recorded {want[tuple(bad[0])]} got {got[name][tuple(bad[0])]}"
    # the enumeration reaches every kernel family, every tile shape and the refusals
    ok = gold["rc"] == 0
    assert set(gold["kernel_kind"][ok].tolist()) == {0, 1, 2, 3, 4, 6, 7} and int((~ok).sum()) == 7110
    assert {(64, 64), (128, 64), (64, 128), (128, 128), (128, 160), (256, 256), (256, 160), (128, 320)} <= set(zip(gold["tile_m"][ok].tolist(), gold["tile_n"][ok].tolist()))


# what TG_GEMM_FLAGS once meant besides the planner's five bits: stagger (1), priority hints (2, 32768), the big tile's epilogue (4), the tile-major work
# order (8192) and the two-wave slab kernel's timing switches (1 << 16 .. 1 << 18).  Nothing reads them any more.
_RETIRED_FLAGS = 1 | 2 | 4 | 8192 | 32768 | 1 << 16 | 1 << 17 | 1 << 18


def test_retired_flag_bits_change_no_route(monkeypatch):
    """The retired bits alone plan as no variable at all, and OR-ed onto each of the five router values they plan as that value does."""
    from tests.golden import make_gemm_routes as gen
    from theatergen_amd import _lib
    gold = np.load(os.path.join(ROOT, "tests", "golden", "gemm_routes.npz"))
    rows = [0] + [i for i, e in enumerate(gen.ENVS) if set(e) == {"TG_GEMM_FLAGS"}]
    assert [gen.ENVS[i] for i in rows] == [{}] + [{"TG_GEMM_FLAGS": v} for v in ("8", "128", "1024", "2048", "4096")]
    assert gold["envs"][rows].tolist() == [json.dumps(gen.ENVS[i], sort_keys=True) for i in rows]
    envs = [{"TG_GEMM_FLAGS": str(_RETIRED_FLAGS | int(gen.ENVS[i].get("TG_GEMM_FLAGS", "0")))} for i in rows]
    assert envs[0] == {"TG_GEMM_FLAGS": str(_RETIRED_FLAGS)}

    def setenv(env):
        for k in gen.KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    monkeypatch.setattr(gen, "ENVS", envs)                 # sweep() walks the module's list
    got = gen.sweep(_lib, setenv)
    for name, _ in gen.COLUMNS:
        want = gold[name][rows].astype(np.int64)
        assert want.shape == got[name].shape == (6, 12586), name
        bad = np.argwhere(want != got[name])
        assert bad.size == 0, f"{name}: {len(bad)} rows differ, first (knob setting, descriptor) = {bad[0].tolist()}: " \
                              f"{envs[bad[0][0]]} recorded {want[tuple(bad[0])]} got {got[name][tuple(bad[0])]}"


# (side, channels) -> the batch sizes at which the planner's mirror in unet.py (``_pp_takes_ln``, removed with this table's commit) asked for the statistics
# launch, over batch {1, 2, 4, 8, 16, 32} x side {8 .. 128} x C {320, 640, 1280}: 72 of 162 shapes; the parent's planner put exactly those on kind 7
_LN_STATS = {(8, 1280): [32], (12, 640): [32], (12, 1280): [16, 32], (16, 640): [16, 32], (16, 1280): [8, 16, 32], (24, 640): [8, 16, 32],
             (24, 1280): [4, 8, 16, 32], (32, 640): [4, 8, 16, 32], (32, 1280): [2, 4, 8, 16, 32], (48, 640): [2, 4, 8, 16, 32],
             (48, 1280): [1, 2, 4, 8, 16, 32], (64, 640): [1, 2, 4, 8, 16, 32], (64, 1280): [1, 2, 4, 8, 16, 32], (96, 640): [1, 2, 4, 8, 16, 32],
             (96, 1280): [1, 2, 4, 8, 16, 32], (128, 640): [1, 2, 4, 8, 16, 32], (128, 1280): [1, 2, 4, 8, 16, 32]}


def test_layernorm_statistics_decision_is_the_planners(monkeypatch):
    from theatergen_amd import ops
    for k in ("TG_PP", "TG_GEMM_FLAGS"):
        monkeypatch.delenv(k, raising=False)
    n = 0
    for b in (1, 2, 4, 8, 16, 32):
        for side in (8, 12, 16, 24, 32, 48, 64, 96, 128):
            for ch in (320, 640, 1280):
                want = b in _LN_STATS.get((side, ch), [])
                for dtype in (torch.bfloat16, torch.float16):
                    assert ops.ln_qkv_takes_stats(dtype, b * side * side, ch, ch, side * side) == want, (b, side, ch)
                n += want
    assert n == 72
    # the knob is part of the answer (and of the cache key): without TG_PP bit 2 no LayerNorm-folded launch goes to the ping-pong tiles
    monkeypatch.setenv("TG_PP", "11")
    assert not ops.ln_qkv_takes_stats(torch.bfloat16, 16 * 32 * 32, 640, 640, 32 * 32)
    monkeypatch.setenv("TG_PP", "7")                       # no 256 x 160 tiles: N = 1920 leaves, N = 3840 (256-wide tiles) stays
    assert not ops.ln_qkv_takes_stats(torch.bfloat16, 16 * 32 * 32, 640, 640, 32 * 32)
    assert ops.ln_qkv_takes_stats(torch.bfloat16, 16 * 16 * 16, 1280, 1280, 16 * 16)
    monkeypatch.delenv("TG_PP")
    assert ops.ln_qkv_takes_stats(torch.bfloat16, 16 * 32 * 32, 640, 640, 32 * 32)
