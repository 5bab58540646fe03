"""CPU (no GPU): the head-dim-64 instance of the fused to_q + cross-attention launch (tg_xq_attn on 128 x 128 tiles, TG_XQ_D64) at the
layers that need no device — fragment-blob sizes, the argument checks of the C entry (they return before any launch) and the processors'
eligibility rule."""
import ctypes as C
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TG_ERR_ARG, TG_ERR_UNSUPPORTED = -1, -3


def _lib():
    from theatergen_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib


def test_kv_bytes_by_head_dim():
    h = _lib().lib()
    assert h.tg_xq_kv_bytes(2, 640, 64) == 2 * 5 * 60 * 1024
    assert h.tg_xq_kv_bytes(1, 1280, 64) == 10 * 60 * 1024
    assert h.tg_xq_kv_bytes(1, 320, 64) == -1                  # 2.5 tiles of 128 columns
    assert h.tg_xq_kv_bytes(1, 640, 80) == 4 * 82 * 1024       # the 160-column instances keep their sizes
    assert h.tg_xq_kv_bytes(1, 1280, 160) == 8 * 75 * 1024
    assert h.tg_xq_kv_bytes(1, 640, 40) == -1
    assert h.tg_xq_kv_bytes(1, 640, 160) == 4 * 75 * 1024
    assert h.tg_xq_kv_bytes(1, 384, 80) == -1                  # 80 / 160 still need whole 160-column tiles
    assert h.tg_xq_kv_bytes(0, 640, 64) == -1


def _desc(lib, C_, head_dim, M=256, rows_per_batch=128, text_len=77, ip_tokens=4):
    """every pointer is a fake 16-byte aligned address: the checks under test return before anything is read"""
    d = lib.XqAttnDesc()
    d.dtype = 0
    d.x, d.wq, d.ln_u, d.ln_v, d.kv, d.out = 1 << 12, 2 << 12, 3 << 12, 4 << 12, 5 << 12, 6 << 12
    d.ldx, d.ldc, d.ln_eps = C_, C_, 1e-5
    d.M, d.C, d.head_dim, d.rows_per_batch, d.text_len, d.ip_tokens = M, C_, head_dim, rows_per_batch, text_len, ip_tokens
    return d


def test_xq_attn_argument_checks_return_before_any_launch():
    lib = _lib()
    h = lib.lib()
    # head dim 64: a width that is no whole number of 128-column tiles, a batch item that is no whole number of 128-token tiles, too many keys
    assert h.tg_xq_attn(C.byref(_desc(lib, 320, 64)), None) == TG_ERR_UNSUPPORTED
    assert b"128" in h.tg_last_error()
    assert h.tg_xq_attn(C.byref(_desc(lib, 640, 64, M=128, rows_per_batch=64)), None) == TG_ERR_ARG
    assert b"rows_per_batch" in h.tg_last_error()
    assert h.tg_xq_attn(C.byref(_desc(lib, 640, 64, M=192, rows_per_batch=192)), None) == TG_ERR_ARG
    assert h.tg_xq_attn(C.byref(_desc(lib, 640, 64, text_len=97)), None) == TG_ERR_ARG
    assert h.tg_xq_attn(C.byref(_desc(lib, 640, 64, ip_tokens=17)), None) == TG_ERR_ARG
    # what was refused before stays refused with the same code
    assert h.tg_xq_attn(C.byref(_desc(lib, 320, 40)), None) == TG_ERR_UNSUPPORTED
    assert b"head_dim 40" in h.tg_last_error()
    assert h.tg_xq_attn(C.byref(_desc(lib, 640, 128)), None) == TG_ERR_UNSUPPORTED
    assert h.tg_xq_attn(C.byref(_desc(lib, 400, 80)), None) == TG_ERR_ARG        # C % 160 != 0
    assert h.tg_xq_attn(C.byref(_desc(lib, 800, 160)), None) == TG_ERR_ARG       # C % 64 != 0
    assert b"320" in h.tg_last_error()


def test_kv_pack_argument_checks():
    lib = _lib()
    h = lib.lib()
    p = 1 << 12
    assert h.tg_xq_kv_pack(0, 1, 320, 64, p, p, 80, 77, None, None, 0, 0, p, None) == TG_ERR_ARG
    assert h.tg_xq_kv_pack(0, 1, 640, 40, p, p, 80, 77, None, None, 0, 0, p, None) == TG_ERR_ARG
    assert h.tg_xq_kv_pack(0, 1, 640, 64, p, p, 80, 97, None, None, 0, 0, p, None) == TG_ERR_ARG


def _attn(C_, heads, d=64):
    """what ``xq_eligible`` reads of an Attention: to_q's weight (inner x C) and the head count"""
    return types.SimpleNamespace(heads=heads, to_q=types.SimpleNamespace(weight=torch.empty(heads * d, C_, device="meta")), scale=d ** -0.5)


def _eligible(AP, C_, heads, B, N, d=64, L=77, T=4, dtype=torch.bfloat16, **kw):
    x = torch.empty(B * N, C_, dtype=dtype, device="meta")
    return AP.xq_eligible(_attn(C_, heads, d), x, B, N, L, T, kw)


def test_eligibility_of_head_dim_64(monkeypatch):
    from theatergen_amd import attention_processor as AP
    assert AP.attn_dims(_attn(640, 10)) == (640, 10, 64)
    monkeypatch.setattr(AP, "XQ_ENABLED", True)
    monkeypatch.setattr(AP, "XQ_D64_ENABLED", False)
    monkeypatch.setattr(AP, "XQ_D64_MIN_ROWS", 128)
    assert not _eligible(AP, 640, 10, 2, 1024)                            # opt-in: nothing changes without the flag
    monkeypatch.setattr(AP, "XQ_D64_ENABLED", True)
    assert _eligible(AP, 640, 10, 2, 1024)
    assert _eligible(AP, 640, 10, 2, 1024, dtype=torch.float16)
    assert _eligible(AP, 1280, 20, 2, 256, T=16, L=96)
    assert _eligible(AP, 640, 10, 2, 1024, T=0)
    assert not _eligible(AP, 640, 10, 2, 576)                             # 24 x 24: no whole number of 128-token tiles
    assert not _eligible(AP, 320, 5, 2, 1024)                             # 2.5 tile columns
    assert not _eligible(AP, 640, 10, 2, 1024, save_attn_to_dict={})
    assert not _eligible(AP, 640, 10, 2, 1024, attention_mask=torch.empty(1, device="meta"))
    assert not _eligible(AP, 640, 10, 2, 1024, return_attntion_probs=True)
    assert not _eligible(AP, 640, 10, 2, 1024, dtype=torch.float32)
    assert not _eligible(AP, 640, 10, 2, 1024, L=97)
    assert not _eligible(AP, 640, 10, 2, 1024, T=17)
    monkeypatch.setattr(AP, "XQ_D64_MIN_ROWS", 4096)
    assert not _eligible(AP, 640, 10, 2, 1024)                            # 2048 rows < the threshold
    assert _eligible(AP, 640, 10, 4, 1024)
    monkeypatch.setattr(AP, "XQ_D64_MIN_ROWS", 128)
    monkeypatch.setattr(AP, "XQ_ENABLED", False)                          # TG_XQ=0 switches every fused launch off
    assert not _eligible(AP, 640, 10, 2, 1024)


def test_eligibility_of_head_dims_80_160_does_not_depend_on_the_new_flag(monkeypatch):
    from theatergen_amd import attention_processor as AP
    monkeypatch.setattr(AP, "XQ_ENABLED", True)
    monkeypatch.setattr(AP, "XQ_MIN_ROWS", 4096)
    monkeypatch.setattr(AP, "XQ_D64_MIN_ROWS", 128)
    cases = [(640, 8, 4, 1024, 80, True), (640, 8, 2, 1024, 80, False), (1280, 8, 16, 256, 160, True), (640, 8, 4, 1000, 80, False),
             (320, 8, 16, 4096, 40, False), (480, 6, 16, 1024, 80, False)]
    for flag in (False, True):
        monkeypatch.setattr(AP, "XQ_D64_ENABLED", flag)
        for C_, heads, B, N, d, want in cases:
            assert _eligible(AP, C_, heads, B, N, d=d) == want, (flag, C_, heads, B, N, d)


def test_abi_version_is_unchanged():
    lib = _lib()
    header = open(os.path.join(ROOT, "include", "theatergen_hip.h")).read()
    assert int(re.search(r"#define TG_ABI_VERSION (\d+)", header).group(1)) == 308
    assert lib.ABI_VERSION == 308
    assert lib.lib().tg_version() == 308
