#!/usr/bin/env python3
"""Development aid: what a step of k_run costs in instructions, read off the compiled code (no GPU).

For one k_run instantiation of one translation unit (compiled to gfx950 assembly with the product flags, like isa_waits.py) it prints
  - the kernel's registers: VGPRs, spilled SGPRs / VGPRs, scratch, waves per SIMD;
  - static instruction counts by class - VALU, SALU, LDS, vector memory, scalar memory, lane reads / writes (v_readlane / v_writelane:
    the reloads and stores of spilled SGPRs), waits, branches - of the BATCH loop (the innermost loop around a batch's first DPP, the
    walk's loop included) and of the STEP loop outside it (interest, list, barriers, cursor, team boundary, fold; cut and join code too:
    static counts say what the step path carries, not what a step executes);
  - the register moves and vmcnt waits at the head of the batch loop, in front of the prefetch: the "this batch's rows = the rows
    requested during the batch before" copy of the loops that are not unrolled by two (NOTEBOOK.md 5.13, 5.18).

usage: isa_step_path.py [--unit simfire_hip_run2.hip] [--kernel "1,0,1,0,2"] [--asm FILE] [--label TEXT]
"""
import argparse
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_waits as iw  # noqa: E402

BLOCK = re.compile(r"^(?:\.L(BB\d+_\d+):|; %bb\.\d+:)")
IN_LOOP = re.compile(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)")
PARENT = re.compile(r"Parent Loop (BB\d+_\d+) Depth=(\d+)")
IS_HEADER = re.compile(r"This (?:Inner )?Loop Header: Depth=(\d+)")
CLASSES = ("VALU", "SALU", "LDS", "VMEM", "SMEM", "lane", "wait", "branch", "other")


def kernel_text(asm_text, args):
    """(raw lines of one k_run instantiation, comments kept; its symbol)."""
    key = iw.mangled(args)
    lines = asm_text.splitlines()
    start = next((i for i, ln in enumerate(lines) if key in ln and re.match(r"^_Z\S+:", ln)), None)
    if start is None:
        raise LookupError("no k_run<%s> in this assembly" % args)
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines[start + 1:end], lines[start].split(":")[0]


def resources(asm_text, symbol):
    """VGPRs, spills, scratch and waves per SIMD of one kernel: the compiler's `; Kernel info` comments and the code object's metadata."""
    lines = asm_text.splitlines()
    out = {}
    at = next(i for i, ln in enumerate(lines) if ln.startswith(symbol + ":"))
    for ln in lines[at:]:
        m = re.match(r"^; (NumVgprs|ScratchSize|Occupancy): (\d+)", ln)
        if m:
            out[m.group(1)] = int(m.group(2))
            if m.group(1) == "Occupancy":
                break
    name = next(i for i, ln in enumerate(lines) if re.match(r"^\s+\.name:\s+%s\s*$" % re.escape(symbol), ln))
    lo = next(i for i in range(name, -1, -1) if lines[i].startswith("  - ."))       # (the kernel's entry of the metadata: fields sorted by name)
    hi = next((i for i in range(name + 1, len(lines)) if lines[i].startswith("  - .") or not lines[i].startswith(" ")), len(lines))
    for ln in lines[lo:hi]:
        m = re.match(r"^\s+\.(sgpr_spill_count|vgpr_spill_count|vgpr_count|private_segment_fixed_size):\s+(\d+)", ln)
        if m:
            out[m.group(1)] = int(m.group(2))
    return out


def blocks(raw):
    """The kernel's basic blocks in text order: (innermost loop header or None, is-a-header name or None, parents, instructions)."""
    out, cur = [], None
    for ln in raw:
        if BLOCK.match(ln):
            cur = {"label": BLOCK.match(ln).group(1), "notes": [ln], "ins": []}
            out.append(cur)
        elif cur is None:
            continue
        elif ln.lstrip().startswith(";"):
            if not cur["ins"]:
                cur["notes"].append(ln)
        elif ln.strip() and not ln.lstrip().startswith("."):
            cur["ins"].append(iw.instr(ln))
    for b in out:
        notes = " ".join(b["notes"])
        b["parents"] = [m.group(1) for m in PARENT.finditer(notes)]
        b["header"] = b["label"] if IS_HEADER.search(notes) else None
        m = IN_LOOP.search(notes)
        b["inner"] = b["header"] or (m.group(1) if m else None)
    parents = {b["header"]: b["parents"] for b in out if b["header"]}
    for b in out:
        b["chain"] = (parents.get(b["inner"], []) + [b["inner"]]) if b["inner"] else []
    return out


def classify(op):
    name = op.split()[0]
    if name in ("v_readlane_b32", "v_writelane_b32"):
        return "lane"
    if name.startswith("s_waitcnt"):
        return "wait"
    if name.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc", "s_barrier")):
        return "branch"
    if name.startswith(("s_load", "s_buffer_load", "s_memtime", "s_memrealtime")):
        return "SMEM"
    if name.startswith("ds_"):
        return "LDS"
    if name.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "VMEM"
    if name.startswith("v_"):
        return "VALU"
    if name.startswith("s_"):
        return "SALU"
    return "other"


def count(bs):
    c = dict.fromkeys(CLASSES, 0)
    for b in bs:
        for op in b["ins"]:
            c[classify(op)] += 1
    c["all"] = sum(c[k] for k in CLASSES)
    return c


def header_moves(body):
    """The instructions between the batch loop's header and the first row load of the prefetch that are register moves or waits that
    name vmcnt: (v_mov_b64, v_mov_b32, vmcnt waits, the longest run of consecutive moves)."""
    load, dpp = iw.find_prefetch(body)
    first, _, hdr = iw.loop_range(body, dpp)
    n64 = n32 = nw = run = best = 0
    for i in range(first, load - 3):
        op = iw.instr(body[i])
        if op.startswith(("v_mov_b64", "v_mov_b32")) and re.match(r"v_mov_b(64|32)(_e32)? v(\d+|\[\d+:\d+\]), v", op):
            n64 += op.startswith("v_mov_b64")
            n32 += op.startswith("v_mov_b32")
            run += 1
            best = max(best, run)
        elif not iw.LABEL.match(body[i]):
            run = 0
        if op.startswith("s_waitcnt") and "vmcnt" in op:
            nw += 1
    return {"v_mov_b64": n64, "v_mov_b32": n32, "vmcnt_waits": nw, "longest_run": best, "header": hdr, "span": load - 3 - first}


def analyse(asm_text, args):
    raw, symbol = kernel_text(asm_text, args)
    body = iw.kernel_lines(asm_text, args)
    res = resources(asm_text, symbol)
    hm = header_moves(body)
    bs = blocks(raw)
    batch_hdr = hm["header"]
    chain = next(b["chain"] for b in bs if b["header"] == batch_hdr)
    # the loops around the batch loop, outermost first: (assignments, TEAM = 2 only,) steps, chunks of the list, batches
    step_hdr = chain[-3] if len(chain) >= 3 else chain[0]
    in_batch = [b for b in bs if batch_hdr in b["chain"]]
    in_step = [b for b in bs if step_hdr in b["chain"] and batch_hdr not in b["chain"]]
    entry = [b for b in bs if not b["chain"]]
    return {"resources": res, "header_moves": hm, "batch_loop": count(in_batch), "step_outside": count(in_step), "outside_loops": count(entry),
            "batch_header": batch_hdr, "step_header": step_hdr}


def report(asm_text, args, label="", out=sys.stdout):
    a = analyse(asm_text, args)
    r, hm = a["resources"], a["header_moves"]
    p = lambda *x: print(*x, file=out)
    p("# k_run<%s>%s" % (args.replace(",", ", "), ("  [%s]" % label) if label else ""))
    p("registers: %d VGPRs, %d spilled SGPRs, %d spilled VGPRs, scratch %d B per lane, %d waves per SIMD" %
      (r.get("NumVgprs", r.get("vgpr_count", -1)), r.get("sgpr_spill_count", -1), r.get("vgpr_spill_count", -1),
       r.get("ScratchSize", r.get("private_segment_fixed_size", -1)), r.get("Occupancy", -1)))
    p("loops: steps %s, batches %s" % (a["step_header"], a["batch_header"]))
    p("%-28s | %5s | %s" % ("static instructions", "all", " | ".join("%5s" % k for k in CLASSES)))
    for name, key in (("batch loop (with the walk)", "batch_loop"), ("step loop outside it", "step_outside"), ("outside the step loop", "outside_loops")):
        c = a[key]
        p("%-28s | %5d | %s" % (name, c["all"], " | ".join("%5d" % c[k] for k in CLASSES)))
    p("head of the batch loop, %d instructions in front of the prefetch: %d v_mov_b64 + %d v_mov_b32 (longest run %d), %d waits that name vmcnt" %
      (hm["span"], hm["v_mov_b64"], hm["v_mov_b32"], hm["longest_run"], hm["vmcnt_waits"]))
    return a


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--unit", default="simfire_hip_run2.hip")
    ap.add_argument("--kernel", default="1,0,1,0,2", help="template arguments of k_run: MAXD,ATT,DIAG,MIT,TEAM")
    ap.add_argument("--asm", default=None)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    if a.asm:
        text = open(a.asm).read()
    else:
        with tempfile.TemporaryDirectory() as d:
            text = open(iw.compile_asm(a.unit, os.path.join(d, "unit.s"))).read()
    report(text, a.kernel, a.label)


if __name__ == "__main__":
    main()
