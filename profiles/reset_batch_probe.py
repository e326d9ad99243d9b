"""Probe: what a partial reset costs (sf_reset_env loop / sf_reset_envs / sf_reset_where, simfire_amd/csrc/sf_reset_kernels.h).

C3's shape (256 x 1024^2, shared terrain) after a 100-update rollout, in both cell layouts - the blocked plane current (after a
resident launch) and the row-major planes current (after per-step launches) - for n = 1, 8, 64, 256 environments:

  (a) the ``sf_reset_env`` loop of this library (the path ``BatchedFireSimulation.reset(envs)`` took before: n calls, n waits),
  (b) one ``sf_reset_envs``,
  (c) ``sf_reset_where(NULL, ...)`` with exactly n environments out (outside the timed window they are given, with ``sf_load_state``
      from device memory, the state of a fresh environment whose ``running`` word and result row say QUIT, after the episodes that
      ended by themselves have been restarted; the count is checked in the result block).

Wall time per call: host clock around the call(s) and a ``sync``, median [min, max] of 7 after one warm-up.  For (b) and (c) also
the GPU time of the call's two launches (HIP events on the handle's stream, ``sf_time_resets``) and the bytes the launch clears
(computed from the geometry below) over it, as a share of 8 TB/s.

  python profiles/reset_batch_probe.py            # -> profiles/reset_batch_timing.txt
  python profiles/reset_batch_probe.py --quick    # 16 x 256^2, nothing written
  python profiles/reset_batch_probe.py --paths    # the two older entries alone (below), printed; nothing written

``--paths``: wall time of one ``sf_reset_env`` and of one full ``sf_reset`` with their wait, the same shape, rollout and layouts, and
one small case (1 x 64 x 64, the ``FireSimulation.reset()`` shape) - for A/B runs of two libraries (``SIMFIRE_HIP_LIB``), the way
``profiles/reset_paths_ab.txt`` was made."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from simfire_amd import workloads  # noqa: E402
from simfire_amd.engine import FireEngine  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "reset_batch_timing.txt")
PEAK = 8.0e12
REPS = 7


def cleared_bytes(eng, blocked):
    """Bytes k_reset_envs zeroes per environment (simfire_hip.hip: reset_launch), the small slices included."""
    g = eng.geometry()
    H, W, P = eng.H, eng.W, g["pitch"]
    PV = P // 16
    plane = H * P
    md = int(eng.params.max_fire_duration)
    ab = 1 if md <= 5 else (2 if md <= 13 else 4)
    cells = ((H + 3) // 4 + 2) * PV * 128 if blocked else plane + (H + 2) * P * ab
    b = cells + 8 * plane
    if eng.params.attenuate_line_ros:
        b += 4 * plane
    tiles = g["tiles_x"] * g["tiles_y"]
    b += 2 * (g["tiles_x"] + 2) * (g["tiles_y"] + 2)              # tile activity maps (a guard ring)
    b += 3 * H * ((PV + 63) // 64) * 8                            # vector bitmaps
    b += tiles + 16 * tiles                                       # tile histograms and their stale marks (when known)
    return b


def med(v):
    return "%9.3f ms  [%.3f, %.3f]" % (statistics.median(v), min(v), max(v))


def probe(size, E, ns, rollout, lines):
    w = workloads.c3(size, E)
    import torch
    for name, fused in (("blocked plane current (after a resident launch)", 2), ("row-major planes current (after per-step launches)", 0)):
        eng = FireEngine(**w.engine_kwargs())
        eng.set_layers(*w.layers())
        eng.set_fused(fused)
        eng.reset(w.init_xy)
        eng.step(rollout)
        eng.sync()
        blocked = fused == 2
        per_env = cleared_bytes(eng, blocked)
        lines.append(f"{name}: {per_env / 1e6:.2f} MB cleared per environment")
        lines.append("     n | (a) sf_reset_env loop            | (b) sf_reset_envs                | (b) launches, share of 8 TB/s | "
                     "(c) sf_reset_where(NULL)         | (c) launches, share of 8 TB/s")
        xy_all = np.ascontiguousarray(w.init_xy, dtype=np.int32)

        # the state of an environment that is out: a fresh one with EnvState.running (blob byte 128) and the row's first word (160) zero
        eng.reset_envs([0], xy_all[:1])
        blob = eng.save_state([0])
        blob[0, 128:132] = 0
        blob[0, 160:164] = 0
        out_blobs = torch.from_numpy(blob).cuda().repeat(E, 1).contiguous()

        def relayout():
            eng.step(2)                                  # (a getter or a map upload may have converted the planes)
            eng.sync()
            assert eng.cell_layout() == (1 if blocked else 0)

        for n in ns:
            envs = np.arange(n, dtype=np.int32)
            xy = xy_all[:n]

            def loop():
                t0 = time.perf_counter()
                for e in range(n):
                    eng.reset_env(e, int(xy[e, 0]), int(xy[e, 1]))
                eng.sync()
                return (time.perf_counter() - t0) * 1e3

            def batch():
                t0 = time.perf_counter()
                eng.reset_envs(envs, xy)
                eng.sync()
                return (time.perf_counter() - t0) * 1e3, eng.reset_ms()

            def where():
                eng.reset_where(None, xy_all)                # (episodes that ended by themselves start again: everything runs ...)
                eng.load_state(envs, out_blobs[:n])          # ... but these n environments
                st = eng.status()[0]
                out = np.flatnonzero(st[:, 0] == 0)
                assert out.tolist() == list(range(n)), (n, out.tolist())
                assert eng.cell_layout() == (1 if blocked else 0)
                t0 = time.perf_counter()
                eng.reset_where(None, xy_all)
                eng.sync()
                ms = (time.perf_counter() - t0) * 1e3
                assert (eng.status()[0][:, 0] == 1).all()
                return ms, eng.reset_ms()

            relayout()
            eng.time_resets(False)
            loop()
            a = [loop() for _ in range(REPS)]
            eng.time_resets(True)
            batch()
            b = [batch() for _ in range(REPS)]
            where()
            c = [where() for _ in range(REPS)]
            share = lambda runs: "%7.3f ms %5.1f %%" % (statistics.median(r[1] for r in runs),
                                                       100.0 * n * per_env / (statistics.median(r[1] for r in runs) * 1e-3) / PEAK)
            lines.append("  %4d | %s | %s | %s              | %s | %s" % (n, med(a), med([r[0] for r in b]), share(b),
                                                                        med([r[0] for r in c]), share(c)))
            print(lines[-1], flush=True)
        eng.close()


def probe_paths(w, rollout, layouts):
    """One ``sf_reset_env`` / one full ``sf_reset``, host clock around the call and a ``sync``; two updates before every timed call
    (not timed) so that each reset meets an episode under way in the layout the line names."""
    xy = np.ascontiguousarray(w.init_xy, dtype=np.int32)
    for name, fused in layouts:
        eng = FireEngine(**w.engine_kwargs())
        eng.set_layers(*w.layers())
        eng.set_fused(fused)
        eng.reset(xy)
        eng.step(rollout)
        eng.sync()

        def timed(call):
            eng.step(2)
            eng.sync()
            layout = eng.cell_layout()
            t0 = time.perf_counter()
            call()
            eng.sync()
            ms = (time.perf_counter() - t0) * 1e3
            assert eng.cell_layout() == layout
            return ms

        for what, call in (("sf_reset_env", lambda: eng.reset_env(0, int(xy[0, 0]), int(xy[0, 1]))), ("sf_reset    ", lambda: eng.reset(xy))):
            timed(call)
            print("  %-56s %s | %s" % (f"{w.name}, {name} (layout {eng.cell_layout()})", what, med([timed(call) for _ in range(REPS)])), flush=True)
        eng.close()


def main():
    quick = "--quick" in sys.argv
    if "--paths" in sys.argv:
        size, E, rollout = (256, 16, 6) if quick else (1024, 256, 100)
        probe_paths(workloads.c3(size, E), rollout, (("blocked plane current", 2), ("row-major planes current", 0)))
        probe_paths(workloads.c1(64), 10, (("automatic choice", -1),))
        return
    lines = []
    if quick:
        probe(256, 16, (1, 8, 16), 6, lines)
    else:
        probe(1024, 256, (1, 8, 64, 256), 100, lines)
    head = ("Partial resets on one MI355X: C3's shape (256 x 1024^2, shared terrain) after a 100-update rollout.  Wall time per call (host clock\n"
            "around the call(s) + sync), median [min, max] of 7 after one warm-up; launches: GPU time of the call's two launches (HIP events on the\n"
            "handle's stream), median of the same 7, and the bytes cleared over it as a share of 8 TB/s.\n")
    text = head + "\n" + "\n".join(lines) + "\n"
    print(text)
    if not quick:
        with open(OUT, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
