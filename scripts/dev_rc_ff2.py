"""dev: tg_rc_ff on its two kernels — rc_ff_kernel (one wave per SIMD) and rc_ff2_kernel (two waves per SIMD, 16 tokens per wave) — in isolation.

    python scripts/dev_rc_ff2.py                  the gate: 65536 x 320, inner 1280, proj_out tail, rotating operands, HIP events, both kernels
                                                  interleaved on one box; parity of both against fp32
    python scripts/dev_rc_ff2.py --parent-table   rel-L2 against fp64 of BOTH kernels on the operands of tests/test_rc_ff2_gpu.py (the one-wave
                                                  column is that test's PARENT table)

Prints one JSON line per row; ``--out FILE`` also writes the rows to FILE (profiles/rc_ff2_gate.json holds a gate run)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
import torch.nn.functional as F

from theatergen_amd import ops, rowchain
from theatergen_amd.weights_pack import rc_pack_tiles
from dev_rc_linear import timeit

dev = "cuda"


def gate(M=65536, inner=1280, dtype=torch.bfloat16, rounds=3, rot=6):
    torch.manual_seed(0)
    C = 320
    hs = [(torch.randn(M, C, device=dev) * 1.2 + 0.2).to(dtype) for _ in range(rot)]
    x0s = [torch.randn(M, C, device=dev).to(dtype) for _ in range(rot)]
    outs = [torch.empty(M, C, device=dev, dtype=dtype) for _ in range(rot)]
    w1 = (torch.randn(2 * inner, C, device=dev) / C ** 0.5).to(dtype); b1 = (0.2 * torch.randn(2 * inner, device=dev)).to(dtype)
    w2 = (torch.randn(C, inner, device=dev) / inner ** 0.5).to(dtype); b2 = (0.1 * torch.randn(C, device=dev)).to(dtype)
    wp = (torch.randn(C, C, device=dev) / C ** 0.5).to(dtype); bp = (0.1 * torch.randn(C, device=dev)).to(dtype)
    gamma = (1 + 0.2 * torch.randn(C, device=dev)).to(dtype); beta = (0.1 * torch.randn(C, device=dev)).to(dtype)
    x = F.layer_norm(hs[0].float(), (C,), gamma.float(), beta.float(), 1e-5)
    pr = x @ w1.float().T + b1.float()
    h3 = (pr[:, :inner] * F.gelu(pr[:, inner:])) @ w2.float().T + b2.float() + hs[0].float()
    ref = h3 @ wp.float().T + bp.float() + x0s[0].float()
    del x, pr, h3
    arms = {"one_wave": (rowchain.pack_ff(w1, b1, gamma, beta, w2, b2), rc_pack_tiles(wp, bp.float()), False),
            "two_wave": (rowchain.pack_ff2(w1, b1, gamma, beta, w2, b2), rowchain.pack_po2(wp, bp.float()), True)}
    row = {"M": M, "inner": inner, "dtype": str(dtype), "rotating_operands": rot}
    for name, ((s1, s2, bb2), wpo, two) in arms.items():
        got = ops.rc_ff(hs[0], s1, s2, bb2, inner, 1e-5, wpo=wpo, res0=x0s[0], two_wave=two)
        torch.cuda.synchronize()
        row[name] = {"rel_l2_vs_fp32": ((got.float() - ref).norm() / ref.norm()).item(), "us": []}
    for _ in range(rounds):
        for name, ((s1, s2, bb2), wpo, two) in arms.items():
            t = timeit(lambda i: ops.rc_ff(hs[i % rot], s1, s2, bb2, inner, 1e-5, wpo=wpo, res0=x0s[i % rot], out=outs[i % rot], two_wave=two), n=20)
            row[name]["us"].append(round(t, 1))
    for name in arms:
        v = sorted(row[name]["us"])
        row[name]["median_us"] = v[len(v) // 2]
    row["two_over_one"] = round(row["two_wave"]["median_us"] / row["one_wave"]["median_us"], 4)
    print(json.dumps(row), flush=True)
    return row


def parent_table():
    sys.path.insert(0, os.path.join(ROOT))
    from tests import test_rc_ff2_gpu as t
    table = {}
    for case in t.CASES:
        for dname in t.DTYPES:
            o = t.operands(case, dname)
            one = t.rel_l2(t.launch(o, case, two_wave=False)[0], o["ref"])
            two = t.rel_l2(t.launch(o, case, two_wave=True)[0], o["ref"])
            table[f"{case}/{dname}"] = {"one_wave": one, "two_wave": two}
            print(f'    ("{case}", "{dname}"): {one:.4e},    # two-wave kernel: {two:.4e}', flush=True)
    return table


if __name__ == "__main__":
    res = parent_table() if "--parent-table" in sys.argv else [gate(), gate(dtype=torch.float16, rounds=1)]
    if "--out" in sys.argv:
        path = os.path.abspath(sys.argv[sys.argv.index("--out") + 1])
        os.makedirs(os.path.dirname(path), exist_ok=True)
        json.dump(res, open(path, "w"), indent=1)
