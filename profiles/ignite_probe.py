"""Probe: what an ignition during an episode costs (sf_ignite_device, simfire_amd/csrc/sf_ignite_kernels.h).

C3's shape (256 x 1024^2, shared terrain) after a 100-update rollout, in both cell layouts - the blocked plane current (after a
resident launch) and the row-major planes current (after per-step launches) - for n = 1, 256, 65 536 rows spread over all
environments, with arrival recording off and on:

  (a) ``sf_ignite_device``: wall time of the call with its wait (host clock around the call and a ``sync``), and the GPU time of its
      one scatter launch (HIP events on the handle's stream, ``sf_time_ignites``) - with recording on the wall time holds the arrival
      pass behind the launch, the events do not;
  (b) the yardstick, ``sf_apply_mitigation_device`` with the same number of rows on the same handle (wall time; it has no events of
      its own).  With ``SIMFIRE_HIP_LIB`` naming another build of the library - the parent commit's - ``--yardstick`` measures (b)
      alone on that build: the nearest operation that exists without this change.

and what the first stepping call behind an ignition pays (a recounted result row, a lost window placement): one 20-update call
behind an ignition of 256 rows against the same call without one, each from the same 100-update state.

Median [min, max] of 7 repetitions after one warm-up; every repetition ignites cells that are still UNBURNED.

  python profiles/ignite_probe.py                 # -> profiles/ignite_timing.txt
  python profiles/ignite_probe.py --quick         # 16 x 256^2, nothing written
  python profiles/ignite_probe.py --yardstick     # (b) alone, printed (for the parent's library)"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from simfire_amd import workloads  # noqa: E402
from simfire_amd.engine import FireEngine  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "ignite_timing.txt")
REPS = 7


def med(v, unit="us", scale=1e3):
    return "%9.1f %s [%.1f, %.1f]" % (statistics.median(v) * scale, unit, min(v) * scale, max(v) * scale)


def rows_for(rng, n, E, H, W, kind):
    """n rows spread over all environments, in the first eight rows of the grid: UNBURNED after 100 updates in all but the few
    environments whose random ignition lies up there (a row on another cell is skipped by the kernel after the same loads)."""
    q = np.zeros((n, 4), dtype=np.int32)
    q[:, 0] = np.arange(n) % E
    q[:, 1] = rng.integers(0, W, size=n)
    q[:, 2] = rng.integers(0, 8, size=n)
    q[:, 3] = kind
    return q


def fresh(w, fused, rollout, arrival):
    eng = FireEngine(**w.engine_kwargs())
    eng.set_layers(*w.layers())
    eng.set_fused(fused)
    if arrival:
        eng.enable_arrival(True)
    eng.reset(w.init_xy)
    eng.step(rollout)
    eng.sync()
    return eng


def wall(eng, call):
    t0 = time.perf_counter()
    call()
    eng.sync()
    return (time.perf_counter() - t0) * 1e3


def probe(size, E, ns, rollout, lines, yardstick_only):
    import torch
    w = workloads.c3(size, E)
    rng = np.random.default_rng(29)
    for name, fused in (("blocked plane current (after a resident launch)", 2), ("row-major planes current (after per-step launches)", 0)):
        for arrival in ((False,) if yardstick_only else (False, True)):
            eng = fresh(w, fused, rollout, arrival)
            assert eng.cell_layout() == (1 if fused == 2 else 0)
            H, W = eng.H, eng.W
            lines.append(f"{name}, arrival recording {'on' if arrival else 'off'}")
            lines.append("       n | sf_ignite_device, wall with the wait | its scatter launch, HIP events | sf_apply_mitigation_device, wall with the wait")
            if not yardstick_only:
                eng.time_ignites(True)
            for n in ns:
                ign_wall, ign_ev, mit_wall = [], [], []
                for rep in range(REPS + 1):
                    t = torch.from_numpy(rows_for(rng, n, E, H, W, 0)).cuda()
                    m = torch.from_numpy(rows_for(rng, n, E, H, W, 3)).cuda()
                    m[:, 2] += H - 8                                  # lines at the other end of the grid
                    torch.cuda.synchronize()
                    if not yardstick_only:
                        a = wall(eng, lambda: eng.ignite_torch(t))
                        b = eng.ignite_ms()
                    c = wall(eng, lambda: eng.apply_mitigation_torch(m))
                    if rep:
                        if not yardstick_only:
                            ign_wall.append(a)
                            ign_ev.append(b)
                        mit_wall.append(c)
                    assert eng.cell_layout() == (1 if fused == 2 else 0)      # neither call converts
                lines.append("%8d | %s | %s | %s" % (n, med(ign_wall) if ign_wall else "-", med(ign_ev) if ign_ev else "-", med(mit_wall)))
            lines.append("")
    if yardstick_only:
        return
    lines.append("the first stepping call behind an ignition: one 20-update call from the same 100-update state (resident launch, wall with the wait)")
    plain, behind = [], []
    for rep in range(REPS + 1):
        for with_ignition, out in ((False, plain), (True, behind)):
            eng = fresh(w, 2, rollout, False)
            if with_ignition:
                eng.ignite_torch(torch.from_numpy(rows_for(rng, 256, E, eng.H, eng.W, 0)).cuda())
                eng.sync()
            ms = wall(eng, lambda: eng.step(20))
            if rep:
                out.append(ms)
            del eng
    lines.append("  without an ignition: %s   behind 256 rows: %s   difference of the medians: %.3f ms"
                 % (med(plain, "ms", 1.0), med(behind, "ms", 1.0), statistics.median(behind) - statistics.median(plain)))


def main():
    quick, yard = "--quick" in sys.argv, "--yardstick" in sys.argv
    size, E, ns = (256, 16, (1, 256, 4096)) if quick else (1024, 256, (1, 256, 65536))
    lines = [f"ignitions during an episode: {E} x {size}^2 after 100 updates, {REPS} repetitions, median [min, max]"
             + (f"; library {os.environ.get('SIMFIRE_HIP_LIB', 'in-tree')}" if yard else ""), ""]
    probe(size, E, ns, 100, lines, yard)
    text = "\n".join(lines) + "\n"
    print(text)
    if not quick and not yard:
        with open(OUT, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
