"""dev: tg_rc_ff (rc_ff2_kernel: two waves per SIMD, 16 tokens per wave) in isolation.

    python scripts/dev_rc_ff2.py                  65536 x 320, inner 1280, proj_out tail, rotating operands, HIP events; parity against fp32

Prints one JSON line per row; ``--out FILE`` also writes the rows to FILE (profiles/rc_ff2_gate.json holds a run from the time the one-wave
kernel was timed beside this one)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
import torch.nn.functional as F

from theatergen_amd import ops, rowchain
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
    s1, s2, bb2 = rowchain.pack_ff2(w1, b1, gamma, beta, w2, b2)
    wpo = rowchain.pack_po2(wp, bp.float())
    got = ops.rc_ff(hs[0], s1, s2, bb2, inner, 1e-5, wpo=wpo, res0=x0s[0])
    torch.cuda.synchronize()
    row = {"M": M, "inner": inner, "dtype": str(dtype), "rotating_operands": rot, "rel_l2_vs_fp32": ((got.float() - ref).norm() / ref.norm()).item()}
    row["us"] = [round(timeit(lambda i: ops.rc_ff(hs[i % rot], s1, s2, bb2, inner, 1e-5, wpo=wpo, res0=x0s[i % rot], out=outs[i % rot]), n=20), 1)
                 for _ in range(rounds)]
    row["median_us"] = sorted(row["us"])[len(row["us"]) // 2]
    print(json.dumps(row), flush=True)
    return row


if __name__ == "__main__":
    res = [gate(), gate(dtype=torch.float16, rounds=1)]
    if "--out" in sys.argv:
        path = os.path.abspath(sys.argv[sys.argv.index("--out") + 1])
        os.makedirs(os.path.dirname(path), exist_ok=True)
        json.dump(res, open(path, "w"), indent=1)
