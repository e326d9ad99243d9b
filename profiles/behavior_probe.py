"""Probe: what fire behaviour per cell costs (sf_behavior, simfire_amd/csrc/sf_behavior_kernels.h).

C3's shape (256 x 1024^2) and C5's (64 x 1024^2 with its 64 agents), both with their one shared terrain, and 32 x 1024^2 with a
terrain table per environment (the same planes 32 times: 2 GiB of tables, nothing of them stays in cache); a fire about 200
updates old.  Timed: ``flame_length`` alone, the five planes, and the summary + point form only; beside each the byte bound of
section 25 - 64 + 4 bytes read per cell and 4 (``head``: 1) written per plane, at the 8 TB/s of HBM peak the design quotes - and
the fraction of it the call reaches; then one update of the same handle at that moment (``step_timed``) and, on C5's shape, one
``agents_step`` tick.  The summary + point form reads 1 status byte per cell and the table only for the BURNING cells: its bound
is the status plane alone.

The handle works on a stream of its own that torch does not know, so a window is a host clock around CALLS asynchronous calls that
ends in ``sync()`` + ``torch.cuda.synchronize()``; every variant is warmed by one window that is not counted, the variants take
turns window by window, and the figure is the median [min, max] of REPS windows.  The first call (it builds the heat cache) is
made before anything is timed.

  python profiles/behavior_probe.py                   # -> profiles/behavior_timing.txt
  python profiles/behavior_probe.py --out PATH        # ... written to PATH instead
  python profiles/behavior_probe.py --quick           # 8, 8 and 4 x 256^2, nothing written"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "profiles", "behavior_timing.txt")
REPS, CALLS = 7, 3
UPDATES = 200
HBM = 8.0e12            # bytes per second: the peak DESIGN.md quotes
ALL = ("hpa", "ros", "intensity", "flame_length", "head")


def med(v):
    return "%9.3f [%.3f, %.3f]" % (statistics.median(v), min(v), max(v))


def main():
    import numpy as np
    import torch
    from simfire_amd import workloads
    from simfire_amd.engine import FireEngine
    quick = "--quick" in sys.argv
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else OUT
    shapes = (("c3", 256, 8), ("c5", 256, 8), ("c3 per-env", 256, 4)) if quick else (("c3", 1024, 256), ("c5", 1024, 64), ("c3 per-env", 1024, 32))
    updates = 40 if quick else UPDATES
    text = (f"Fire behaviour per cell on one MI355X.  Wall milliseconds per call: asynchronous mode, {CALLS} calls between two syncs, median [min, max]\n"
            f"of {REPS} windows after one warm-up window; the variants take turns.  bound: the bytes of DESIGN.md section 25 at 8 TB/s; 'of bound': bound /\n"
            f"measured.  'update': one update of the same handle at that moment (device events around 10 updates / 10).\n")
    for name, size, E in shapes:
        K = 64
        w = workloads.c5(size, E, K) if name == "c5" else workloads.c3(size, E)
        if name == "c3 per-env":
            eng = FireEngine(**dict(w.engine_kwargs(), per_env_terrain=True))
            layers = w.layers()
            for e in range(E):
                eng.set_layers(*layers, env=e)
        else:
            eng = FireEngine(**w.engine_kwargs())
            eng.set_layers(*w.layers())
        eng.reset(w.init_xy)
        H = W = size
        dev = torch.device("cuda:0")
        rng = np.random.default_rng(83)
        xy = np.stack([rng.integers(W, size=(E, K)), rng.integers(H, size=(E, K))], axis=-1).astype(np.int32)
        tick_ms = None
        if name == "c5":
            eng.agents_create(K, w.init_xy, n_updates=1, weights=(-1.0, 0.1, -5.0, -0.1), only_unburned=True, auto_reset=False)
            eng.agents_place(np.arange(E), xy)
        pts = torch.from_numpy(np.concatenate([xy, np.tile(np.arange(1, K + 1), (E, 1))[..., None]], axis=-1).astype(np.int32)).to(dev)
        eng.step(updates)
        eng.step(2)                  # (a call of two updates is a resident launch here: the blocked plane is current again)
        first = eng.behavior(planes=ALL, stats=True, points=pts)            # builds the heat cache
        burning = int(first["classes"].sum().item())
        max_flame = float(first["max_flame"].max().item())
        del first
        cells = E * H * W
        variants = {
            "flame_length": (lambda: eng.behavior(planes=("flame_length",)), cells * (64 + 4 + 4)),
            "five planes": (lambda: eng.behavior(planes=ALL), cells * (64 + 4 + 4 * 4 + 1)),
            "summary + points": (lambda: eng.behavior(planes=(), stats=True, points=pts), cells * 1),
        }
        lay = eng.cell_layout()
        eng.set_async(True)
        ms = {v: [] for v in variants}
        for rep in range(REPS + 1):
            for v, (fn, _) in variants.items():
                eng.sync()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(CALLS):
                    fn()
                eng.sync()
                torch.cuda.synchronize()
                if rep:
                    ms[v].append((time.perf_counter() - t0) * 1e3 / CALLS)
        eng.set_async(False)
        assert eng.cell_layout() == lay
        step_ms = eng.step_timed(10) / 10.0
        if name == "c5":
            acts = torch.zeros((E, K), dtype=torch.int32, device=dev)
            eng.set_async(True)
            t = []
            for rep in range(4):
                eng.sync()
                t0 = time.perf_counter()
                for _ in range(20):
                    eng.agents_step(acts)
                eng.sync()
                if rep:
                    t.append((time.perf_counter() - t0) * 1e3 / 20)
            eng.set_async(False)
            tick_ms = statistics.median(t)
        text += (f"\n{name}: {E} x {size}^2, about {updates} updates after reset: {burning} BURNING cells, largest flame length {max_flame:.2f} ft, "
                 f"one update {step_ms:.3f} ms" + (f", one agents_step tick {tick_ms:.3f} ms" if tick_ms is not None else "")
                 + f", cell_layout() {lay}, heat cache {eng.behavior_builds() * H * W * 4 / 2 ** 20:.0f} MiB, tables {eng.behavior_builds() * 64 * H * W / 2 ** 20:.0f} MiB\n")
        for v, (_, nbytes) in variants.items():
            m = statistics.median(ms[v])
            bound = nbytes / HBM * 1e3
            text += (f"  {v:17s} {med(ms[v])} ms  = {m / step_ms:7.1f} updates;  {nbytes / 1e9:6.2f} GB, bound {bound:6.3f} ms, "
                     f"{100.0 * bound / m:5.1f} % of bound, {nbytes / m / 1e9:7.2f} TB/s\n")
        eng.close()
    print(text)
    if not quick:
        with open(out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
