#!/usr/bin/env python3
"""Development aid: the waits of k_run's batch loop, read off the compiled code.

Compiles one translation unit to gfx950 assembly with the product flags (simfire_amd/build.py: FLAGS minus -shared, plus
-S --cuda-device-only), finds the batch loop of one k_run instantiation - the innermost loop around the first `wave_shr:1` DPP, which
starts a batch's work - and prints every s_waitcnt in it with the memory instructions issued since the wait before.  A wait that
names vmcnt between the four row loads of the prefetch and that DPP means the wave sits out the round trip of its NEXT batch's rows in
front of the current batch's work (NOTEBOOK.md 5.13); tests/test_batch_prefetch_isa_cpu.py asserts there is none.

usage: isa_waits.py [--unit simfire_hip_run2.hip] [--kernel "1,0,1,0,2"] [--asm FILE]      (--asm: read this assembly, do not compile)
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEM = re.compile(r"^\s*(global_|flat_|scratch_|buffer_|ds_|s_load_|s_buffer_load_)")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
DPP_START = "wave_shr:1"
ROW_LOAD = "global_load_dwordx4"


def compile_asm(unit, out):
    """hipcc -S of simfire_amd/csrc/<unit> with the product flags; returns the assembly's path (`out`)."""
    sys.path.insert(0, ROOT)
    from simfire_amd import build as B
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = [f for f in B.FLAGS if f != "-shared"] + ["-S", "--cuda-device-only"]
    subprocess.run([hipcc] + flags + ["-o", out, os.path.join(B.CSRC, unit)], check=True, stderr=subprocess.DEVNULL)
    return out


def mangled(args):
    """'1,0,1,0,2' -> the part of the symbol that names k_run<1, 0, 1, 0, 2>."""
    return "5k_runI" + "".join("Li%sE" % (("n%d" % -v) if v < 0 else str(v)) for v in (int(x) for x in args.split(","))) + "E"


def kernel_lines(asm_text, args):
    """The instructions of one k_run instantiation, label lines included, comments-only lines dropped."""
    key = mangled(args)
    lines = asm_text.splitlines()
    start = next((i for i, ln in enumerate(lines) if key in ln and re.match(r"^_Z\S+:", ln)), None)
    if start is None:
        raise LookupError("no k_run<%s> in this assembly" % args)
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return [ln for ln in lines[start + 1:end] if ln.strip() and not ln.lstrip().startswith(";")]


def instr(ln):
    return ln.split(";")[0].strip()


def find_prefetch(body):
    """(index of the last of the four consecutive row loads in front of the first batch-start DPP, index of that DPP)."""
    dpp = next(i for i, ln in enumerate(body) if DPP_START in ln)
    i = dpp
    while i >= 3:
        if all(ROW_LOAD in body[i - k] for k in range(4)):
            return i, dpp
        i -= 1
    raise LookupError("no group of four %s in front of the first %s" % (ROW_LOAD, DPP_START))


def vm_waits_on_skip_path(body, load, dpp):
    """The s_waitcnt that name vmcnt on the way from the last row load to the DPP on which every s_cbranch_execz is taken: the path of a
    wave without an edge lane and without a boundary row."""
    labels = {m.group(1): i for i, ln in enumerate(body) for m in [LABEL.match(ln)] if m}
    waits, i, steps = [], load + 1, 0
    while i != dpp:
        steps += 1
        if steps > 10000 or i >= len(body):
            raise RuntimeError("the path from the prefetch does not reach the batch's first DPP")
        op = instr(body[i])
        if op.startswith("s_waitcnt") and "vmcnt" in op:
            waits.append((i, op))
        m = re.match(r"(s_cbranch_execz|s_branch)\s+(\.LBB\d+_\d+)", op)
        i = labels[m.group(2)] if m else i + 1
    return waits


def vm_waits_between(body, load, dpp):
    """Every s_waitcnt that names vmcnt between the last row load and the DPP, on any path (the blocks lie between them in the text)."""
    return [(i, instr(body[i])) for i in range(load + 1, dpp) if instr(body[i]).startswith("s_waitcnt") and "vmcnt" in instr(body[i])]


def loop_range(body, dpp):
    """[first, last) of the innermost loop around body[dpp], by the compiler's `in Loop: Header=` block comments."""
    hdr = None
    for i in range(dpp, -1, -1):
        m = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", body[i]) if LABEL.match(body[i]) else None
        if m:
            hdr = m.group(1)
            break
    first = next(i for i, ln in enumerate(body) if ln.startswith(".L%s:" % hdr))
    marked = [i for i, ln in enumerate(body) if LABEL.match(ln) and ("Header=%s " % hdr) in ln]
    last = next((i for i in range(marked[-1] + 1, len(body)) if LABEL.match(body[i])), len(body))
    return first, last, hdr


def report(body, args, out=sys.stdout):
    load, dpp = find_prefetch(body)
    first, last, hdr = loop_range(body, dpp)
    p = lambda *a: print(*a, file=out)
    p("# k_run<%s>: batch loop = loop with header %s, instructions %d .. %d of the kernel (labels counted)" % (args.replace(",", ", "), hdr, first, last))
    p("# row loads of the prefetch end at %d, the batch's first DPP (%s) is at %d" % (load, DPP_START, dpp))
    skip, every = vm_waits_on_skip_path(body, load, dpp), vm_waits_between(body, load, dpp)
    p("# vmcnt waits between them: %d on the path that takes every s_cbranch_execz, %d on any path" % (len(skip), len(every)))
    p("# index | wait | memory instructions issued since the wait before (x count)")
    pending = []
    for i in range(first, last):
        op = instr(body[i])
        if i == load - 3:
            p("%6d | -- prefetch: the next batch's four rows are requested here" % i)
        if i == dpp:
            p("%6d | -- the batch's work starts (first %s)" % (i, DPP_START))
        if MEM.match(op):
            pending.append(op.split()[0])
        elif op.startswith("s_waitcnt"):
            seen = []
            for m_ in pending:
                if seen and seen[-1][0] == m_:
                    seen[-1][1] += 1
                else:
                    seen.append([m_, 1])
            p("%6d | %-32s | %s" % (i, op, " ".join(n if c == 1 else "%s x%d" % (n, c) for n, c in seen) or "-"))
            pending = []


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--unit", default="simfire_hip_run2.hip")
    ap.add_argument("--kernel", default="1,0,1,0,2", help="template arguments of k_run: MAXD,ATT,DIAG,MIT,TEAM")
    ap.add_argument("--asm", default=None)
    a = ap.parse_args()
    if a.asm:
        text = open(a.asm).read()
    else:
        with tempfile.TemporaryDirectory() as d:
            text = open(compile_asm(a.unit, os.path.join(d, "unit.s"))).read()
    report(kernel_lines(text, a.kernel), a.kernel)


if __name__ == "__main__":
    main()
