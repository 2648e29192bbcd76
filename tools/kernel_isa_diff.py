"""Did a change to csrc sources change their gfx950 code?  Compiles the named files (default: svr, regress,
kpredict, baseline and gbr.hip, the estimators) of two csrc directories under build.py's flags and compares
every kernel.

    python tools/kernel_isa_diff.py PARENT_CSRC [CSRC] [--files conv.hip lower.hip]
                                    (CSRC default: the tree's csrc; PARENT_CSRC inside a checkout, e.g. a
                                     `git worktree add` of the parent)

Per kernel: instruction text identical / mnemonic sequence identical / the compiler's register, scratch, LDS and
occupancy figures equal.  A kernel whose mnemonics differ is printed with its instruction-count difference,
whether the two sequences are the same multiset (a reordering only), the diff of the two sequences and whether
its float64 arithmetic (v_*_f64, v_mfma_f64*, v_exp*, v_rcp*, v_div*) still runs in the same order.
Exit status 1 when a kernel's mnemonics or figures differ.
"""
import argparse
import collections
import difflib
import os
import re
import subprocess
import sys

import stem_codegen as S

FILES = ["svr.hip", "regress.hip", "kpredict.hip", "baseline.hip", "gbr.hip"]
FIGURES = ["TotalNumSgprs", "NumVgprs", "NumAgprs", "TotalNumVgprs", "ScratchSize", "LDSByteSize", "Occupancy"]
F64 = re.compile(r"v_\w+_f64|v_mfma_f64|v_exp|v_rcp|v_div")


def kernels(src):
    asm = S.assembly(src)
    entry = set(re.findall(r"^\s*\.amdhsa_kernel (\w+)", asm, re.M))
    return {k: v for k, v in S.kernels(asm, r"\w+").items() if k in entry}


def figures(meta):
    return {k: int(re.search(r"; " + k + r":\s*(\d+)", meta).group(1)) for k in FIGURES}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("tree", nargs="?", default=os.path.join(S.PKG, "csrc"))
    ap.add_argument("--files", nargs="+", default=FILES)
    args = ap.parse_args()
    parent, tree = args.parent, args.tree
    bad = 0
    for f in args.files:
        a, b = kernels(os.path.join(parent, f)), kernels(os.path.join(tree, f))
        print(f"{f}: {len(a)} kernels in the parent, {len(b)} in the tree")
        bad += set(a) != set(b)
        for name in sorted(set(a) & set(b)):
            (ia, ma), (ib, mb) = a[name], b[name]
            oa, ob = [ln.split()[0] for ln in ia], [ln.split()[0] for ln in ib]
            fa, fb = figures(ma), figures(mb)
            short = subprocess.run(["c++filt", "-p", name], capture_output=True, text=True).stdout.strip() or name
            print(f"  {short:44s} {len(ib):5d} instructions   text {'identical' if ia == ib else 'DIFFERS  '}   mnemonics "
                  f"{'identical' if oa == ob else 'DIFFER   '}   figures {'equal' if fa == fb else 'DIFFER'}  "
                  + " ".join(f"{k} {v}" for k, v in fb.items()))
            if fa != fb:
                print("    parent figures: " + " ".join(f"{k} {v}" for k, v in fa.items()))
            if oa != ob:
                same = [o for o in oa if F64.match(o)] == [o for o in ob if F64.match(o)]
                print(f"    {len(ob) - len(oa):+d} instructions, "
                      f"{'a reordering only (same multiset)' if collections.Counter(oa) == collections.Counter(ob) else 'NOT the same multiset'}")
                print(f"    float64 arithmetic mnemonics in {'unchanged' if same else 'CHANGED'} order; mnemonic diff:")
                for ln in difflib.unified_diff(oa, ob, "parent", "tree", lineterm="", n=2):
                    print("      " + ln)
            bad += oa != ob or fa != fb
    print("every kernel: mnemonic sequence identical, figures equal" if not bad else f"{bad} kernels or files differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
