"""Probe: what walking distance costs (sf_walk, simfire_amd/csrc/sf_walk_kernels.h).

C3's shape (256 x 1024^2) and C5's (64 x 1024^2 with its 64 agents): one band per thread, k_walk<true>; one row for 128 x 2048^2
(four passes of bands per level, k_walk<false>).  A fire about 200 updates old, BURNING through UNBURNED, the agents' four moves.
Timed: the point form capped at 64 moves and uncapped, and the plane form uncapped; beside each the levels the search ran (min /
median / max over the environments), one update of the same handle at that moment (``step_timed``), on C5's shape one ``agents_step``
tick, and what a caller does today, timed in this same script:

  torch   ``fire_maps_torch()`` + a level loop on the device (``max_pool2d`` of the cells reached, times walkable, a level number
          written where a cell is new, until nothing changes - looked at every 8th level), on TODAY_ENVS environments and scaled to
          the batch.

The yardstick is that path, not the new code.  The handle works on a stream of its own that torch does not know, so a window is a
host clock around CALLS asynchronous calls that ends in ``sync()`` + ``torch.cuda.synchronize()``; every variant is warmed by one
window that is not counted, the variants take turns window by window, and the figure is the median [min, max] of REPS windows.
Before anything is timed the new plane is compared with the torch loop, cell for cell.

  python profiles/walk_probe.py            # -> profiles/walk_timing.txt
  python profiles/walk_probe.py --quick    # 8 x 256^2 and 4 x 2048^2, nothing written"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "profiles", "walk_timing.txt")
REPS, CALLS, TODAY_ENVS = 7, 3, 4
UPDATES = 200
FAR = 2 ** 31 - 1


def med(v):
    return "%10.3f [%.3f, %.3f]" % (statistics.median(v), min(v), max(v))


def torch_moves(torch, maps):
    """Moves to BURNING through UNBURNED over the four moves of uint8 maps [n, H, W] on the device, int32 with FAR / -1: what a
    caller can write today."""
    F = torch.nn.functional
    target = (maps == 1)
    walk = (maps == 0).to(torch.float16).unsqueeze(1)
    seen = target.to(torch.float16).unsqueeze(1)
    d = torch.where(target, 0, torch.where(maps == 0, FAR, -1)).to(torch.int32)
    level = 0
    while True:
        before = seen
        for _ in range(8):
            grown = torch.maximum(F.max_pool2d(seen, (3, 1), 1, (1, 0)), F.max_pool2d(seen, (1, 3), 1, (0, 1))) * walk
            new = (grown > 0) & ~(seen > 0)
            level += 1
            d = torch.where(new.squeeze(1), level, d)
            seen = torch.maximum(seen, grown)
        if torch.equal(before, seen):
            return d, level


def main():
    import numpy as np
    import torch
    from simfire_amd import workloads
    from simfire_amd.engine import FireEngine
    quick = "--quick" in sys.argv
    shapes = (("c3", 256, 8), ("c4", 2048, 4)) if quick else (("c3", 1024, 256), ("c5", 1024, 64), ("c4", 2048, 128))
    updates = 40 if quick else UPDATES
    text = (f"Walking distance on one MI355X.  Wall milliseconds per call: asynchronous mode, {CALLS} calls between two syncs, median [min, max] of {REPS}\n"
            f"windows after one warm-up window; the variants take turns.  'update': one update of the same handle at that moment (device events\n"
            f"around 10 updates / 10).  levels: min / median / max over the environments.  torch: what a caller does today (see the probe's\n"
            f"header), timed on {TODAY_ENVS} environments and scaled to the batch.\n")
    for name, size, E in shapes:
        K = 64
        w = workloads.c5(size, E, K) if name == "c5" else (workloads.c4(size, E) if name == "c4" else workloads.c3(size, E))
        eng = FireEngine(**w.engine_kwargs())
        eng.set_layers(*w.layers())
        eng.reset(w.init_xy)
        H = W = size
        dev = torch.device("cuda:0")
        rng = np.random.default_rng(79)
        xy = np.stack([rng.integers(W, size=(E, K)), rng.integers(H, size=(E, K))], axis=-1).astype(np.int32)
        tick_us = None
        if name == "c5":
            eng.agents_create(K, w.init_xy, n_updates=1, weights=(-1.0, 0.1, -5.0, -0.1), only_unburned=True, auto_reset=False)
            eng.agents_place(np.arange(E), xy)
        pts = torch.from_numpy(np.concatenate([xy, np.tile(np.arange(1, K + 1), (E, 1))[..., None]], axis=-1).astype(np.int32)).to(dev)
        eng.step(updates)
        eng.step(2)                  # (a call of two updates is a resident launch here: the blocked plane is current again)
        n = min(TODAY_ENVS, E)
        # the two searches agree before either is timed
        new = eng.walk(plane=True, levels=True, envs=list(range(n)))
        old, turns = torch_moves(torch, eng.fire_maps_torch()[:n])
        assert torch.equal(new["moves"], old), (name, size)
        del new, old
        eng.step(2)
        variants = {
            f"{K} points, cap 64": lambda: eng.walk(points=pts, step=True, max_moves=64),
            f"{K} points": lambda: eng.walk(points=pts, step=True),
            "plane": lambda: eng.walk(plane=True),
        }
        r = eng.walk(levels=True, reached=True)
        levels, cells = r["levels"].cpu().numpy(), r["reached"].cpu().numpy()
        lay = eng.cell_layout()
        eng.set_async(True)
        ms = {v: [] for v in variants}
        for rep in range(REPS + 1):
            for v, fn in variants.items():
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
        tor = []
        for rep in range(3):
            eng.sync()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got, turns = torch_moves(torch, eng.fire_maps_torch()[:n])
            torch.cuda.synchronize()
            if rep:
                tor.append((time.perf_counter() - t0) * 1e3 * E / n)
        assert eng.cell_layout() in (lay, 0)
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
            tick_us = statistics.median(t)
        text += (f"\n{name}: {E} x {size}^2, about {updates} updates after reset: {cells.mean():.0f} cells with a route per environment, "
                 f"levels {levels.min()} / {int(np.median(levels))} / {levels.max()}, one update {step_ms:.3f} ms"
                 + (f", one agents_step tick {tick_us:.3f} ms" if tick_us is not None else "")
                 + f", cell_layout() {lay}, scratch {eng.walk_scratch_bytes() * E / 2 ** 20:.0f} MiB\n")
        for v in variants:
            m = statistics.median(ms[v])
            text += f"  {v:18s} {med(ms[v])} ms  = {m / step_ms:8.1f} updates\n"
        text += f"  {'torch (device)':18s} {med(tor)} ms  (scaled from {n} environments; {turns} levels)\n"
        text += f"  torch / plane = {statistics.median(tor) / statistics.median(ms['plane']):.0f}\n"
        eng.close()
    print(text)
    if not quick:
        with open(OUT, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
