#!/usr/bin/env python
"""dev helper (not part of the product): did a source change move a kernel's code?  Per-kernel diff of the gfx950 assembly of one .hip file in two trees.

    python scripts/dev_isa_diff.py <tree A> <tree B> tg_attention.hip [substring of the kernel symbol]

A tree is a checkout of this repository (e.g. `git worktree add ../parent HEAD~1`).  Both sides are compiled with the flags of theatergen_amd/build.py
(FLAGS plus the file's EXTRA_FLAGS; this checkout's, for both), device pass only, to assembly (-S --cuda-device-only).  Comments, `.file`, `.ident` and
the `__hip_cuid_*` symbol are stripped, data symbols (the constant pages) are renamed after their CONTENT so that a renamed page still matches, and the
function number inside local labels is dropped.  Then, per kernel symbol (code and kernel descriptor): `identical`, or the number of differing lines.
Exit status 1 if some kernel differs, 2 if a kernel exists on one side only.  It is a diff and nothing else."""
import difflib
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from theatergen_amd.build import EXTRA_FLAGS, FLAGS, _hipcc, _pretty  # noqa: E402


def assembly(tree, name, workdir, tag):
    src = os.path.join(tree, "theatergen_amd", "csrc", name)
    out = os.path.join(workdir, tag + ".s")
    subprocess.run([_hipcc()] + FLAGS + EXTRA_FLAGS.get(name, []) + ["-S", "--cuda-device-only", src, "-o", out], check=True, stderr=subprocess.DEVNULL)
    lines = []
    for l in open(out).read().split("\n"):
        l = l.split(";")[0].rstrip()
        if l.strip() and not re.match(r"\s*\.(file|ident)\b", l) and "__hip_cuid_" not in l:
            lines.append(l)
    return lines


def rename_data(lines):
    """every `@object` symbol -> data_<hash of its definition without the name>[_n]"""
    names = [m.group(1) for l in lines for m in [re.match(r"\s*\.type\s+(\S+),@object", l)] if m]
    new, seen = {}, {}
    for n in names:
        i = next((k for k, l in enumerate(lines) if l.startswith(n + ":")), None)
        if i is None:                                 # zero-initialised: `.comm name,size,align`
            body = [l.split(",", 1)[1] for l in lines if re.match(r"\s*\.comm\s+" + re.escape(n) + ",", l)]
        else:
            j = next(k for k in range(i, len(lines)) if re.match(r"\s*\.size\s+" + re.escape(n) + ",", lines[k]))
            body = lines[i + 1:j] + [lines[j].split(",")[-1]]
        h = hashlib.sha256("\n".join(body).encode()).hexdigest()[:12]
        seen[h] = seen.get(h, 0) + 1
        new[n] = f"data_{h}" + (f"_{seen[h]}" if seen[h] > 1 else "")
    if not new:
        return lines
    pat = re.compile("|".join(sorted((re.escape(n) for n in new), key=len, reverse=True)))
    return [pat.sub(lambda m: new[m.group(0)], l) for l in lines]


def kernels(lines):
    """{kernel symbol: its code (label .. .Lfunc_end) + its .amdhsa_kernel block}"""
    lines = [re.sub(r"\.L(BB|func_end|func_begin)\d+", r".L\1", l) for l in lines]
    out = {}
    for i, l in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)
        if not m:
            continue
        sym = m.group(1)
        e = next(k for k in range(i, len(lines)) if ".end_amdhsa_kernel" in lines[k])
        s = lines.index(sym + ":")
        f = next(k for k in range(s, len(lines)) if lines[k].startswith(".Lfunc_end"))
        out[sym] = lines[s:f] + lines[i:e + 1]
    return out


def main():
    if len(sys.argv) < 4:
        sys.exit(__doc__)
    tree_a, tree_b, name = sys.argv[1:4]
    filt = sys.argv[4] if len(sys.argv) > 4 else ""
    with tempfile.TemporaryDirectory(prefix="isa_diff_") as td:
        a, b = (kernels(rename_data(assembly(t, name, td, tag))) for t, tag in ((tree_a, "a"), (tree_b, "b")))
    status = 0
    for sym in sorted(set(a) | set(b), key=_pretty):
        if filt not in sym and filt not in _pretty(sym):
            continue
        if sym not in a or sym not in b:
            print(f"{_pretty(sym):70s} only in {'A' if sym in a else 'B'}")
            status = 2
        elif a[sym] == b[sym]:
            print(f"{_pretty(sym):70s} identical ({len(a[sym])} lines)")
        else:
            ops = difflib.SequenceMatcher(None, a[sym], b[sym], autojunk=False).get_opcodes()
            n = sum(max(i2 - i1, j2 - j1) for op, i1, i2, j1, j2 in ops if op != "equal")
            print(f"{_pretty(sym):70s} {n} differing lines of {len(a[sym])} / {len(b[sym])}")
            status = max(status, 1)
    sys.exit(status)


if __name__ == "__main__":
    main()
