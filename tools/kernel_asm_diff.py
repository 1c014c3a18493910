#!/usr/bin/env python3
"""Compares the kernels of two device listings (hipcc --cuda-device-only -S of
pt_kernels.hip or pt_kernels_env.hip, build.py's flags) function by function:
which bodies are instruction-identical, which differ, which exist on one side
only, with each kernel's VGPR / SGPR / LDS / scratch figures from the metadata.

Labels are compared without their function numbers and comments are dropped.
render_kernel instantiations are matched by their template arguments, a
trailing `false` of the longer list ignored (a new defaulted parameter).
--kernarg OLD,NEW treats the kernel-argument segment's old and new size as the
same number (an appended KParams field moves the hidden arguments behind it).

Usage: python tools/kernel_asm_diff.py parent.s new.s [--kernarg 704,720]
"""
from __future__ import annotations

import argparse
import re
import shutil
import subprocess
from collections import Counter


def functions(path, kernarg):
    out, name, body = {}, None, []
    for ln in open(path):
        m = re.match(r"^(_Z\w+):", ln)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if ln.startswith(".Lfunc_end"):
            out[name], name = body, None
            continue
        ln = re.sub(r"\.L(BB|tmp|func_begin|JTI)\d+_", r".L\1_", ln).split(";")[0].rstrip()
        ln = re.sub(r"_ZZ?N3ptk13render_kernelI(Lb[01]E)+", "KERNEL", ln)
        if kernarg:  # the hidden arguments' offsets and the segment's size
            old, new = kernarg
            ln = "" if "amdhsa_kernarg_size" in ln else ln.replace(hex(new - 256), hex(old - 256))
        if ln:
            body.append(ln)
    return out


def metadata(path):
    txt = open(path).read()
    res = {}
    for blk in re.split(r"\n  - \.", txt[txt.find("amdhsa.kernels"):]):
        n = re.search(r"\.name:\s+(\S+)", blk)
        if n:
            g = lambda k: (re.search(r"\.%s:\s+(\d+)" % k, blk) or [None, "?"])[1]
            res[n.group(1)] = "vgpr %s sgpr %s lds %s scratch %s" % (g("vgpr_count"), g("sgpr_count"),
                                                                     g("group_segment_fixed_size"),
                                                                     g("private_segment_fixed_size"))
    return res


def demangle(names):
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not filt:
        return {n: n for n in names}
    out = subprocess.run([filt] + list(names), capture_output=True, text=True).stdout.splitlines()
    return dict(zip(names, out))


def key(d):
    m = re.search(r"render_kernel<([^>]*)>", d)
    if m:
        a = m.group(1).split(", ")
        while len(a) > 7 and a[-1] == "false":
            a.pop()
        d = d.replace(m.group(1), ", ".join(a))
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--kernarg", default=None, help="OLD,NEW kernel-argument segment sizes to treat as equal")
    args = ap.parse_args()
    kernarg = tuple(int(v) for v in args.kernarg.split(",")) if args.kernarg else None
    a, b = functions(args.parent, kernarg), functions(args.new, kernarg)
    ma, mb = metadata(args.parent), metadata(args.new)
    da, db = demangle(list(a)), demangle(list(b))
    ka, kb = {key(da[n]): n for n in a}, {key(db[n]): n for n in b}
    same = 0
    for d in sorted(set(ka) | set(kb)):
        if d in ka and d in kb:
            x, y = a[ka[d]], b[kb[d]]
            if x == y:
                same += 1
                continue
            ops = lambda body: Counter(l.split()[0] for l in body if l.startswith("\t") and not l.startswith("\t."))
            how = "the same lines in another order" if sorted(x) == sorted(y) else \
                "the same opcode counts" if ops(x) == ops(y) else "other instructions"
            print(f"DIFFERENT ({len(x)} / {len(y)} lines, {how}): {d}\n    {ma.get(ka[d])} | {mb.get(kb[d])}")
        else:
            side, n, m = ("parent", ka.get(d), ma) if d in ka else ("new", kb.get(d), mb)
            print(f"only in {side}: {d}\n    {m.get(n)}")
    print(f"{same} kernels identical")


if __name__ == "__main__":
    main()
