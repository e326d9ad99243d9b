"""Probe: what labelling costs (sf_components, simfire_amd/csrc/sf_components_kernels.h).

C3's shape and layers (256 x 1024^2), about 100 and about 500 updates into the fires, three requests:

  (a) fires      BURNING, count + largest only: the label plane lives in scratch and is never written out
  (b) scars      BURNING | BURNED, labels + every row (cells, first, bbox, touch, largest, selected)
  (c) pockets    UNBURNED with touch: one huge component per map, the case with the longest union chains

and what a caller does today for the same answer, timed in this same script: ``fire_maps_torch()``, the read-back, and
``scipy.ndimage.label`` per environment on 16 host threads (labels and count only - no rows, no touch words).

Two clocks.  'device': HIP events on the handle's stream around everything a call enqueues behind its call block - the memsets of
the outputs and every launch (``time_components`` / ``components_ms``) -, one call at a time.  'wall': the handle works on a stream
of its own that torch does not know, so a window is a host clock around CALLS asynchronous calls that ends in ``sync()`` +
``torch.cuda.synchronize()``, the enqueue of the launches in it.  Every variant is warmed by one round that is not counted, the
variants take turns, and a figure is the median [min, max] of REPS.  The scars are also asked for in growing subsets of their
outputs, device clock only: a call that wants ``count`` alone stops behind the rank scan, ``first`` adds the ranks and the relabel,
the rows add the stats pass, ``largest`` the sizes of all components - the differences are the phases' shares.
Before anything is timed the labels of (b) are compared with scipy's on the first environments.

  python profiles/components_probe.py            # prints its table; profiles/components_timing.txt holds it beside the estimate
  python profiles/components_probe.py --quick    # 8 x 256^2"""
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, CALLS, TODAY_REPS, THREADS, CHECK_ENVS = 7, 3, 3, 16, 4
STRUCTURE = {4: [[0, 1, 0], [1, 1, 1], [0, 1, 0]], 8: [[1, 1, 1]] * 3}


def med(v):
    return "%10.3f [%.3f, %.3f]" % (statistics.median(v), min(v), max(v))


def main():
    import numpy as np
    import torch
    from scipy import ndimage
    from simfire_amd import workloads
    from simfire_amd.engine import FireEngine
    quick = "--quick" in sys.argv
    size, E = (256, 8) if quick else (1024, 256)
    w = workloads.c3(size, E)
    eng = FireEngine(**w.engine_kwargs())
    eng.set_layers(*w.layers())
    eng.reset(w.init_xy)
    conn = 8 if eng.params.diagonal_spread else 4
    text = (f"Connected components on one MI355X, {E} x {size}^2, C3's layers, connectivity {conn}.  Wall milliseconds per call: asynchronous mode,\n"
            f"{CALLS} calls between two syncs, median [min, max] of {REPS} windows after one warm-up window; the variants take turns.  'update': one\n"
            f"update of the same handle at that moment (device events around 10 updates / 10).  today: fire_maps_torch() + .cpu() +\n"
            f"scipy.ndimage.label per environment on {THREADS} host threads, median [min, max] of {TODAY_REPS} runs after one warm-up run.\n")
    done = 0
    for updates in ((20, 60) if quick else (100, 500)):
        eng.step(updates - done - 2)
        eng.step(2)                  # (a call of two updates is a resident launch here: the blocked plane is current again)
        done = updates
        step_ms = eng.step_timed(10) / 10.0
        done += 10
        variants = {"(a) fires: count, largest": lambda: eng.components(("BURNING",), count=True, largest=True),
                    "(b) scars: labels, all rows": lambda: eng.components(("BURNING", "BURNED"), count=True, selected=True, labels=True, cells=True,
                                                                         first=True, bbox=True, touch=True, largest=True),
                    "(c) pockets: cells, touch": lambda: eng.components(("UNBURNED",), count=True, cells=True, touch=True)}
        # the two labellings agree before either is timed
        n = min(CHECK_ENVS, E)
        got = eng.components(("BURNING", "BURNED"), envs=list(range(n)), labels=True, count=True)
        maps = eng.fire_maps_torch()[:n].cpu().numpy()
        for e in range(n):
            lab, c = ndimage.label((maps[e] == 1) | (maps[e] == 2), structure=STRUCTURE[conn])
            assert c == int(got["count"][e]) and (got["labels"][e].cpu().numpy() == lab).all(), (updates, e)
        facts = {v: fn() for v, fn in variants.items()}
        text += (f"\nabout {done} updates after reset, one update {step_ms:.3f} ms, cell_layout() {eng.cell_layout()}; per environment: fires "
                 f"{float(facts['(a) fires: count, largest']['count'].float().mean()):.1f} (largest {float(facts['(a) fires: count, largest']['largest'][:, 1].float().mean()):.0f} cells), "
                 f"scars {float(facts['(b) scars: labels, all rows']['count'].float().mean()):.1f} ({float(facts['(b) scars: labels, all rows']['selected'].float().mean()):.0f} cells), "
                 f"pockets {float(facts['(c) pockets: cells, touch']['count'].float().mean()):.1f}\n")
        del facts, got
        scar = ("BURNING", "BURNED")
        split = {"scars: count (phases 1 - 4)": lambda: eng.components(scar, count=True),
                 "scars: + first (ranks, relabel)": lambda: eng.components(scar, count=True, first=True),
                 "scars: + cells, bbox (stats)": lambda: eng.components(scar, count=True, first=True, cells=True, bbox=True),
                 "scars: + touch": lambda: eng.components(scar, count=True, first=True, cells=True, bbox=True, touch=True),
                 "scars: + largest (all sizes)": lambda: eng.components(scar, count=True, first=True, cells=True, bbox=True, touch=True, largest=True),
                 "scars: + labels = (b) - selected": lambda: eng.components(scar, count=True, first=True, cells=True, bbox=True, touch=True, largest=True, labels=True)}
        eng.time_components(True)
        dev = {v: [] for v in list(variants) + list(split)}
        for rep in range(REPS + 1):
            for v, fn in list(variants.items()) + list(split.items()):
                fn()
                if rep:
                    dev[v].append(eng.components_ms())
        eng.time_components(False)
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

        def today(select):
            maps = eng.fire_maps_torch().cpu().numpy()
            sel = np.isin(maps, select)
            with ThreadPoolExecutor(THREADS) as pool:
                return list(pool.map(lambda e: ndimage.label(sel[e], structure=STRUCTURE[conn])[1], range(E)))
        old = {"(b) scars": [], "(c) pockets": []}
        for rep in range(TODAY_REPS + 1):
            for v, select in (("(b) scars", (1, 2)), ("(c) pockets", (0,))):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                today(select)
                if rep:
                    old[v].append((time.perf_counter() - t0) * 1e3)
        for v in variants:
            text += f"  {v:30s} device {med(dev[v])} ms   wall {med(ms[v])} ms  = {statistics.median(ms[v]) / step_ms:8.1f} updates\n"
        for v in split:
            text += f"    {v:34s} device {med(dev[v])} ms\n"
        for v in old:
            text += f"  today {v:24s} {med(old[v])} ms\n"
        slowest, fastest = max(max(x) for x in ms.values()), min(min(x) for x in old.values())
        text += f"  the slowest window of the query {slowest:.3f} ms, the fastest run of today's route {fastest:.3f} ms: {fastest / slowest:.0f} x\n"
    eng.close()
    print(text)


if __name__ == "__main__":
    main()
