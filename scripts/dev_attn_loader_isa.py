#!/usr/bin/env python
"""dev helper (not part of the product): the key loop of `attention_kernel` in tg_attention.hip, basic block by basic block.

    python scripts/dev_attn_loader_isa.py [path of tg_attention.hip] [substring of the mangled kernel symbol, default the d40 bf16 FOLD instance]

Compiles the file to gfx950 assembly as scripts/dev_isa_loops.py does and prints, for every basic block between the header of the segment-0 tile loop
and its back edge: vector ALU instructions (and among them v_exp_f32, 64-bit multiplies, 64-bit adds, 64-bit moves), MFMAs, LDS-DMA requests, LDS reads,
`s_getpc` (the address of a constant page taken inside the loop) and where the block branches.  The blocks with `global_load_lds` are the loader; which of
them a full tile runs through is read from the branches (profiles/attn_loader_findings.md has the reading for the d40 / d64 / d80 / d160 instances).
A path other than the default source (a checkout of another commit) compares two versions."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    src = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "theatergen_amd", "csrc", "tg_attention.hip")
    filt = sys.argv[2] if len(sys.argv) > 2 else "IDF16bLi48ELi64ELb1ELb1ELb0E"
    out = os.path.join(tempfile.mkdtemp(prefix="isa_"), "k.s")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "theatergen_amd", "csrc"), "-S", "--cuda-device-only", src, "-o", out]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    lines = open(out).read().split("\n")
    for s in [i for i, l in enumerate(lines) if re.match(r"^_Z\w+:", l)]:
        name = lines[s].split(":")[0]
        if "attention_kernel" not in name or filt not in name:
            continue
        e = next(j for j in range(s, len(lines)) if "s_endpgm" in lines[j])
        body = lines[s:e]
        # basic blocks with the loop the compiler's comments put them in (a loop's blocks need not be contiguous, nor start at its header: the PV half
        # of the tile loop is laid out above the header in some instances)
        blocks, cur = [], None
        for l in body:
            t = l.split(";")[0].strip()
            m = re.match(r"^(\.LBB\d+_\d+):", l) or re.match(r"^; %bb\.(\d+):", l)
            if m:
                own = re.search(r"=>\s*This (?:Inner )?Loop Header: Depth=(\d)", l)
                par = re.search(r"Parent Loop (BB\d+_\d+)", l)
                inl = re.search(r"in Loop: Header=(BB\d+_\d+)", l)
                cur = {"name": m.group(1), "ins": [], "header_depth": int(own.group(1)) if own else 0, "parent": par.group(1) if par else None,
                       "loop": inl.group(1) if inl else (m.group(1).lstrip(".L") if own else None)}
                blocks.append(cur)
                continue
            if cur is not None and "Loop Header" in l and "=>" in l:             # the header comment of an inner loop sits on the line after its label
                cur["header_depth"], cur["loop"] = int(re.search(r"Depth=(\d)", l).group(1)), cur["name"].lstrip(".L")
                continue
            if t and cur is not None and not t.startswith("."):
                cur["ins"].append(t)
        for hb in [b for b in blocks if b["header_depth"] == 1]:
            hdr = hb["loop"]
            inner = {b["loop"] for b in blocks if b["parent"] == hdr}
            loop = [b for b in blocks if b["loop"] == hdr or b["loop"] in inner]
            if any(i.startswith("v_mfma") for b in loop for i in b["ins"]):
                break
        else:
            raise SystemExit(name + ": no tile loop found")
        print(f"{name}\n  tile loop {hdr}: {len(loop)} blocks, {sum(len(b['ins']) for b in loop)} instructions")
        blocks = loop
        tot = {}
        for b in blocks:
            ins = b["ins"]
            op = [i.split()[0] for i in ins]
            c = {"valu": sum(1 for o in op if o.startswith("v_") and not o.startswith("v_mfma")),
                 "exp": sum(1 for o in op if o.startswith("v_exp")), "mul64": sum(1 for o in op if o.startswith("v_mad_u64") or o.startswith("v_mad_i64")),
                 "add64": sum(1 for o in op if o.startswith("v_lshl_add_u64")), "mov64": sum(1 for o in op if o.startswith("v_mov_b64")),
                 "mfma": sum(1 for o in op if o.startswith("v_mfma")), "dma": sum(1 for o in op if o.startswith("global_load_lds")),
                 "ds_read": sum(1 for o in op if o.startswith("ds_read")), "getpc": sum(1 for o in op if o.startswith("s_getpc"))}
            br = [i.split()[-1] for i in ins if i.startswith("s_cbranch") or i.startswith("s_branch")]
            print(f"  {b['name']:>10s} " + " ".join(f"{k} {v:3d}" for k, v in c.items()) + f"  -> {' '.join(br)}")
            for k, v in c.items():
                tot[k] = tot.get(k, 0) + v
        print("  all blocks " + " ".join(f"{k} {v:3d}" for k, v in tot.items()))


if __name__ == "__main__":
    main()
