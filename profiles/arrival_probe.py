"""Probe: what recording arrival times costs (sf_enable_arrival, simfire_amd/csrc/sf_arrival_kernels.h).

C3 (256 x 1024^2), the two windows of bench.py - 20 updates after 5 and 1000 after 20 - each 7 times from a reset; GPU milliseconds
of the timed call by HIP events on the handle's stream (``step_timed``), median [min, max] per update:

  (a) the library of the commit before this feature (built aside; SIMFIRE_HIP_PARENT names it, default
      profiles/_variants/libsimfire_hip_parent.so; the line is left out where it does not exist),
  (b) this library, recording off,
  (c) recording on, the sparse pass (the bitmap walk),
  (d) recording on, the dense pass forced (``set_arrival_dense``),

and for (c) / (d) the GPU time of one pass alone behind each window (``time_arrival_pass``: one more pass over the state as the
window left it).  Every variant runs in a child process of its own: a process loads one build of the library.

  python profiles/arrival_probe.py            # -> profiles/arrival_timing.txt
  python profiles/arrival_probe.py --quick    # 8 x 256^2, nothing written"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "profiles", "arrival_timing.txt")
PARENT = os.environ.get("SIMFIRE_HIP_PARENT") or os.path.join(ROOT, "profiles", "_variants", "libsimfire_hip_parent.so")
REPS = 7
WINDOWS = ((5, 20), (20, 1000))           # (warm-up updates, timed updates)
NEW = ("sf_enable_arrival", "sf_get_arrival", "sf_arrival_device", "sf_set_arrival_dense", "sf_get_arrival_passes", "sf_time_arrival_pass")


def child(variant, size, E):
    from simfire_amd import _lib, workloads
    if variant == "a":                     # the parent's library does not export the new entry points
        for name in NEW:
            _lib.SIGNATURES.pop(name, None)
    from simfire_amd.engine import FireEngine
    w = workloads.c3(size, E)
    eng = FireEngine(**w.engine_kwargs())
    eng.set_layers(*w.layers())
    if variant in "cd":
        eng.reset(w.init_xy)
        eng.enable_arrival(True)
        eng.set_arrival_dense(variant == "d")
    res = {}
    for warm, n in WINDOWS:
        ms, pass_ms, kinds = [], [], set()
        for rep in range(REPS + 1):
            eng.reset(w.init_xy)
            eng.step(warm)
            eng.sync()
            ms.append(eng.step_timed(n) / n * 1e3)
            kinds.add(eng.last_launch_kind())
            if variant in "cd":
                pass_ms.append(eng.time_arrival_pass() * 1e3)
        res["%d after %d" % (n, warm)] = dict(us_per_update=ms[1:], pass_us=pass_ms[1:], kinds=sorted(kinds),
                                              passes=eng.arrival_passes() if variant in "cd" else None,
                                              recorded=int(sum((eng.arrival(e) >= 0).sum() for e in range(min(E, 8)))) if variant in "cd" else None)
    print("RESULT " + json.dumps(res))


def med(v):
    return "%8.2f [%.2f, %.2f]" % (statistics.median(v), min(v), max(v))


def main():
    quick = "--quick" in sys.argv
    size, E = (256, 8) if quick else (1024, 256)
    if "--variant" in sys.argv:
        return child(sys.argv[sys.argv.index("--variant") + 1], size, E)
    names = {"a": "the parent commit's library", "b": "this library, recording off", "c": "recording on, sparse pass",
             "d": "recording on, dense pass forced"}
    got = {}
    for v in "abcd":
        env = dict(os.environ)
        if v == "a":
            if not os.path.exists(PARENT):
                continue
            env["SIMFIRE_HIP_LIB"] = PARENT
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--variant", v] + (["--quick"] if quick else []), env=env,
                             capture_output=True, text=True, timeout=900)
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
        if out.returncode or not line:
            print(out.stdout[-2000:], out.stderr[-2000:])
            raise SystemExit(f"variant {v} failed ({out.returncode})")
        got[v] = json.loads(line[0][7:])
    text = (f"Arrival recording on one MI355X: C3's shape, {E} x {size}^2.  GPU microseconds per update of the timed call (HIP events), median [min, max]\n"
            f"of {REPS} repetitions from a reset after one warm-up repetition; for (c) / (d) also one pass alone behind the window.\n\n")
    for key in ("%d after %d" % (n, warm) for warm, n in WINDOWS):
        text += f"  {key}:\n"
        for v, r in got.items():
            r = r[key]
            text += f"    ({v}) {names[v]:34s} {med(r['us_per_update'])} us / update   launch kinds {r['kinds']}"
            if r["pass_us"]:
                text += f"   one pass {med(r['pass_us'])} us   passes sparse / dense {r['passes']}   cells recorded in the first 8 environments {r['recorded']}"
            text += "\n"
        if "a" in got and "b" in got:
            a, b = got["a"][key]["us_per_update"], got["b"][key]["us_per_update"]
            text += f"    (b) against (a): the repetitions {'overlap' if max(min(a), min(b)) <= min(max(a), max(b)) else 'DO NOT overlap'}\n"
        text += "\n"
    print(text)
    if not quick:
        with open(OUT, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
