#!/usr/bin/env python3
"""Development aid: did a refactor change the compiled kernels?  Compares two gfx950 assemblies of one translation unit (no GPU).

For every kernel of the unit it says whether the instruction stream is identical; where it is not it prints both sides' VGPRs, SGPRs,
scratch, LDS, occupancy and instruction count, and what kind of difference it is: the streams agree once the offsets of
kernel-argument loads (s_load_* ... s[a:b], 0x..) are blanked - a changed argument layout and nothing else -, or they hold the same
instructions (opcode for opcode) in another order or other registers, or other instructions.  Kernels are matched by name without
the parameter list, so a parameter's new TYPE does not hide a kernel.

usage: isa_kernel_diff.py PARENT.s BRANCH.s          (both made with isa_waits.compile_asm)
       isa_kernel_diff.py --compile UNIT.hip OUT.s   (compile the working tree's unit)
"""
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_step_path as sp  # noqa: E402
import isa_waits  # noqa: E402

INFO = ("TotalNumSgprs", "TotalNumVgprs", "ScratchSize", "LDSByteSize", "Occupancy")


def kernels(text):
    """symbol -> (instructions, resources) for every kernel (.amdhsa_kernel) of an assembly."""
    lines = text.splitlines()
    names = set(m.group(1) for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)", text, re.M))
    out = {}
    i = 0
    while i < len(lines):
        m = re.match(r"^(\S+):\s*(;.*)?$", lines[i])
        if not (m and m.group(1) in names):
            i += 1
            continue
        sym, body, j = m.group(1), [], i + 1
        while not lines[j].startswith(".Lfunc_end"):
            ln = lines[j].split(";")[0].rstrip()
            if ln.strip() and not ln.lstrip().startswith(".") or re.match(r"^\.LBB", ln):
                body.append(ln.strip())
            j += 1
        res = {}
        for ln in lines[j:j + 80]:
            r = re.match(r"^; (\w+): (\d+)", ln)
            if r and r.group(1) in INFO:
                res[r.group(1)] = int(r.group(2))
        res["instructions"] = sum(1 for b in body if not b.startswith(".LBB"))
        out[sym] = ([re.sub(r"\.LBB\d+_", ".LBB_", x) for x in body], res)
        i = j
    return by_name(out)


def by_name(ks):
    """Keyed by the demangled name without the parameter list: an argument's TYPE may change its mangled name and nothing else."""
    syms = sorted(ks)
    dem = subprocess.run(["c++filt"] + syms, capture_output=True, text=True).stdout.splitlines()
    out = {}
    for sym, d in zip(syms, dem):
        depth, cut = 0, len(d)
        for i in range(len(d) - 1, -1, -1):
            depth += d[i] == ")"
            depth -= d[i] == "("
            if depth == 0:
                cut = i
                break
        name = d[:cut].replace("(anonymous namespace)::", "")
        assert name not in out, name
        out[name] = ks[sym]
    return out


def classes(body):
    c = dict.fromkeys(sp.CLASSES, 0)
    for x in body:
        if not x.startswith(".LBB"):
            c[sp.classify(x)] += 1
    return c


def blank_kernarg(body):
    return [re.sub(r"^(s_load_\w+ \S+ s\[\d+:\d+\]), 0x[0-9a-f]+", r"\1, KARG", b) for b in body]


def main():
    if sys.argv[1] == "--compile":
        isa_waits.compile_asm(sys.argv[2], sys.argv[3])
        return
    a, b = kernels(open(sys.argv[1]).read()), kernels(open(sys.argv[2]).read())
    same = [k for k in a if k in b and a[k][0] == b[k][0]]
    print("kernels: %d parent, %d branch; identical instruction streams: %d" % (len(a), len(b), len(same)))
    for k in sorted(set(a) ^ set(b)):
        print("  only in %s: %s" % ("parent" if k in a else "branch", k))
    for k in sorted(k for k in a if k in b and k not in same):
        ra, rb = a[k][1], b[k][1]
        only_args = blank_kernarg(a[k][0]) == blank_kernarg(b[k][0])
        ops = lambda body: sorted(x.split()[0] for x in body if not x.startswith(".LBB"))
        same_ops = ops(a[k][0]) == ops(b[k][0])
        worse = [f for f in INFO + ("instructions",) if (rb[f] != ra[f] if f in ("ScratchSize", "LDSByteSize", "Occupancy") else rb[f] > ra[f])]
        print("  DIFFERS %s" % k)
        print("    parent: " + ", ".join("%s %d" % (f, ra[f]) for f in INFO + ("instructions",)))
        print("    branch: " + ", ".join("%s %d" % (f, rb[f]) for f in INFO + ("instructions",)))
        ca, cb = classes(a[k][0]), classes(b[k][0])
        print("    by class (branch - parent): " + ", ".join("%s %+d" % (c, cb[c] - ca[c]) for c in ca if cb[c] != ca[c]) if ca != cb else "    by class: equal")
        print("    -> %s; %s" % ("kernel-argument offsets only" if only_args else ("the same instructions in another order / other registers" if same_ops else "other instructions"),
                                ("OVER the parent in " + ", ".join(worse)) if worse else "nothing over the parent"))


if __name__ == "__main__":
    main()
