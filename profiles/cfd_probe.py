"""Probe: CFD wind training (sf_cfd_step, simfire_amd/csrc/sf_cfd_kernels.h) - GPU ms per training iteration (iterate_wind_step +
fvect.step = two Fluid.step()s), kernel time from HIP events (sf_cfd_step_timed), median of 7 timed calls after a warm-up call.

  python profiles/cfd_probe.py                      # every shape -> profiles/cfd_wind_timing.txt
  python profiles/cfd_probe.py --quick              # one small shape, for a rocprofv3 --kernel-trace --stats run
  python profiles/cfd_probe.py --rocprof DIR        # append the kernel's registers / scratch from that run's CSVs

Clocks per wavefront step of the Gauss-Seidel pass are derived from result_accuracy 4 against 1 at 225^2: the 3 extra passes of
each of the 3 lin_solves of a Fluid.step (2 steps per iteration) cost (t4 - t1) / 18 per pass (its set_bnd included), and one pass is
2 (N - 2) - 1 wavefront steps (one strip), at the clock the probe reports."""
import csv
import ctypes as C
import glob
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from simfire_amd import _lib  # noqa: E402
from simfire_amd.wind import _Solver  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "cfd_wind_timing.txt")
SHAPES = [(225, 1, 1), (225, 256, 1), (1024, 1, 1), (1024, 64, 1), (225, 1, 4)]


def ms_per_iteration(n, envs, itr, iters):
    s = _Solver(n, envs, itr, 1.0, 1e-7, 5.3, 0)
    rng = np.random.default_rng(n + envs)
    for e in range(envs):
        s.set_terrain(e, (rng.random((n, n)) < 0.2).astype(np.uint8))
    ms = C.c_float()
    _lib.check(s._lib.sf_cfd_step_timed(s._h, 2 * iters, 2, C.byref(ms)), s._lib)     # warm-up
    ts = []
    for _ in range(7):
        _lib.check(s._lib.sf_cfd_step_timed(s._h, 2 * iters, 2, C.byref(ms)), s._lib)
        ts.append(ms.value / iters)
    s.close()
    return statistics.median(ts), min(ts), max(ts)


def clock_mhz():
    return 2400.0       # MI355X peak engine clock (the clocks per step are an upper bound if the engine ran slower)


def rocprof_lines(d):
    out = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                if "k_cfd" in row.get("Kernel_Name", ""):
                    keep = {k: v for k, v in row.items() if any(t in k for t in ("VGPR", "SGPR", "Scratch", "LDS", "Workgroup_Size"))}
                    out.append("k_cfd kernel trace: " + ", ".join(f"{k}={v}" for k, v in sorted(keep.items())))
                    break
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                if "k_cfd" in row.get("Name", ""):
                    out.append("k_cfd kernel stats: " + ", ".join(f"{k}={row[k]}" for k in ("Calls", "TotalDurationNs", "AverageNs") if k in row))
    return out


def main():
    if "--rocprof" in sys.argv:
        lines = rocprof_lines(sys.argv[sys.argv.index("--rocprof") + 1])
        with open(OUT, "a") as f:
            f.write("\n".join(["", "rocprofv3 --kernel-trace --stats (profiles/cfd_probe.py --quick):"] + lines) + "\n")
        print("\n".join(lines))
        return
    if "--quick" in sys.argv:
        print("225^2 x1 itr1: %.3f ms / iteration" % ms_per_iteration(225, 1, 1, 4)[0])
        return
    lines = ["CFD wind training on one MI355X: GPU ms per training iteration (2 Fluid.step()s), median [min, max] of 7 calls",
             "of sf_cfd_step_timed(2T, 2) after a warm-up call; 20 % random terrain mask, north inflow, viscosity 1e-7, dt 1.", ""]
    res = {}
    for n, envs, itr in SHAPES:
        iters = 40 if n <= 256 else 4
        med, lo, hi = ms_per_iteration(n, envs, itr, iters)
        res[(n, envs, itr)] = med
        lines.append(f"N={n:5d}  E={envs:4d}  result_accuracy={itr}  T={iters:3d}:  {med:9.3f} ms/iteration  [{lo:.3f}, {hi:.3f}]")
        print(lines[-1], flush=True)
    mhz = clock_mhz()
    n = 225
    per_pass = (res[(225, 1, 4)] - res[(225, 1, 1)]) / 18.0
    steps = 2 * (n - 2) - 1
    lines += ["",
              f"E=256 / E=1 at 225^2: {res[(225, 256, 1)] / res[(225, 1, 1)]:.2f}x;  E=64 / E=1 at 1024^2: "
              f"{res[(1024, 64, 1)] / res[(1024, 1, 1)]:.2f}x",
              f"Gauss-Seidel pass at 225^2 (with its set_bnd): {per_pass * 1e3:.1f} us = {steps} wavefront steps -> "
              f"{per_pass * 1e-3 * mhz * 1e6 / steps:.0f} clocks per step at {mhz:.0f} MHz",
              "  dependent chain of one step: one neighbour hop (ds_bpermute shuffle, or the LDS ring between waves) + 4 f64 adds,",
              "  a multiply, an add and a multiply (+ the mask select)"]
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
