"""CPU: ``tg_layernorm_add`` is declared, bound and exported, and refuses bad arguments on the host."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_binding_and_symbol_agree():
    from theatergen_amd import _lib
    header = open(os.path.join(ROOT, "include", "theatergen_hip.h")).read()
    m = re.search(r"^int tg_layernorm_add\s*\(([^;]*)\);", header, flags=re.M | re.S)
    assert m, "tg_layernorm_add is not declared"
    kinds = {"int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float}
    want = [C.c_void_p if "*" in p else kinds[p.split()[0]] for p in (q.strip() for q in m.group(1).replace("\n", " ").split(","))]
    res, args = _lib.SIGNATURES["tg_layernorm_add"]
    assert res is C.c_int32 and args == want
    h = _lib.lib()

    # host validation, fake pointers (never read)
    def call(dtype=0, x=64, ldx=128, r=64, ldr=128, rows=4, Cc=128, g=64, b=64, out=64, ldo=128):
        return h.tg_layernorm_add(dtype, x, ldx, r, ldr, rows, Cc, 1e-5, g, b, out, ldo, None)
    for kw, code in ((dict(dtype=2), -1), (dict(x=0), -1), (dict(r=0), -1), (dict(g=0), -1), (dict(rows=0), -1), (dict(Cc=100, ldx=104, ldr=104, ldo=104), -1),
                     (dict(Cc=1288, ldx=1288, ldr=1288, ldo=1288), -3), (dict(ldx=120), -1), (dict(ldr=132), -1), (dict(out=72), -1)):
        assert call(**kw) == code, kw
        assert b"tg_layernorm_add" in h.tg_last_error()


def test_wrapper_refusals_without_a_device():
    from theatergen_amd import ops
    x = torch.zeros(4, 128, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.layernorm_add(x, x, x[0], x[0])
