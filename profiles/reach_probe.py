"""Probe: what the reach of the fire costs (sf_reach, simfire_amd/csrc/sf_reach_kernels.h).

C3's shape (256 x 1024^2: one band per thread, k_reach<true>) and 128 x 2048^2 (four passes of bands per round, k_reach<false>), a
fire about 200 updates old, without and with a few hundred control-line cells per environment.  Timed: ``count`` only, ``count`` +
``value``, ``mask``, and 64 points per environment; beside each the rounds the fill took (min / median / max over the environments),
one update of the same handle at that moment (``step_timed``), and what a caller does today, timed in this same script:

  torch   ``fire_maps_torch()`` + a dilation loop on the device (``max_pool2d`` of seeds | reach, times open, until nothing changes -
          looked at every 8th turn), on TODAY_ENVS environments and scaled to the batch;
  scipy   ``fire_maps()`` + ``scipy.ndimage.label`` per environment on the host, on TODAY_ENVS environments and scaled - where scipy
          imports.

The yardstick is that path, not the new code.  The handle works on a stream of its own that torch does not know, so a window is a
host clock around CALLS asynchronous calls that ends in ``sync()`` + ``torch.cuda.synchronize()``; every variant is warmed by one
window that is not counted, the variants take turns window by window, and the figure is the median [min, max] of REPS windows.
Before anything is timed the new mask is compared with the torch fill, cell for cell.

  python profiles/reach_probe.py            # -> profiles/reach_timing.txt
  python profiles/reach_probe.py --quick    # 8 x 256^2 and 4 x 2048^2, nothing written"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "profiles", "reach_timing.txt")
REPS, CALLS, TODAY_ENVS = 7, 3, 4
UPDATES = 200


def med(v):
    return "%10.3f [%.3f, %.3f]" % (statistics.median(v), min(v), max(v))


def torch_reach(torch, maps, conn8):
    """The reach of BURNING through UNBURNED of uint8 maps [n, H, W] on the device, bool: what a caller can write today."""
    F = torch.nn.functional
    seed = (maps == 1).to(torch.float16).unsqueeze(1)
    open_ = (maps == 0).to(torch.float16).unsqueeze(1)
    r = torch.zeros_like(seed)
    turns = 0
    while True:
        before = r
        for _ in range(8):
            cur = torch.maximum(r, seed)
            if conn8:
                d = F.max_pool2d(cur, 3, 1, 1)
            else:
                d = torch.maximum(F.max_pool2d(cur, (3, 1), 1, (1, 0)), F.max_pool2d(cur, (1, 3), 1, (0, 1)))
            r = torch.maximum(r, d * open_)
            turns += 1
        if torch.equal(before, r):
            return r.squeeze(1) > 0, turns


def main():
    import numpy as np
    import torch
    from simfire_amd import workloads
    from simfire_amd.engine import FireEngine
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    quick = "--quick" in sys.argv
    shapes = ((256, 8), (2048, 4)) if quick else ((1024, 256), (2048, 128))
    updates = 40 if quick else UPDATES
    text = (f"Reach of the fire on one MI355X.  Wall milliseconds per call: asynchronous mode, {CALLS} calls between two syncs, median [min, max] of {REPS}\n"
            f"windows after one warm-up window; the variants take turns.  'update': one update of the same handle at that moment (device events\n"
            f"around 10 updates / 10).  rounds: min / median / max over the environments.  torch / scipy: what a caller does today (see the\n"
            f"probe's header), timed on {TODAY_ENVS} environments and scaled to the batch.\n")
    for size, E in shapes:
        w = workloads.c3(size, E)
        eng = FireEngine(**w.engine_kwargs())
        eng.set_layers(*w.layers())
        eng.reset(w.init_xy)
        eng.enable_arrival(True)
        H = W = size
        dev = torch.device("cuda:0")
        rng = np.random.default_rng(78)
        eng.values_set(rng.integers(0, 1000, size=(H, W)).astype(np.int32))
        pts = torch.from_numpy(np.stack([rng.integers(W, size=(E, 64)), rng.integers(H, size=(E, 64)), np.tile(np.arange(1, 65), (E, 1))],
                                        axis=-1).astype(np.int32)).to(dev)
        conn8 = bool(eng.params.diagonal_spread)
        eng.step(updates)
        for lines in (False, True):
            if lines:                # a few hundred line cells per environment: a diagonal and a horizontal piece ahead of the fire
                rows = []
                for e in range(E):
                    x0, y0 = int(w.init_xy[e][0]), int(w.init_xy[e][1])
                    rows += [(e, min(W - 1, max(0, x0 - 100 + d)), min(H - 1, y0 + 60 + updates // 4), 3) for d in range(200)]
                    rows += [(e, min(W - 1, x0 + 40 + updates // 4 + d), min(H - 1, max(0, y0 - 75 + d)), 3) for d in range(150)]
                eng.apply_mitigation(rows)
            eng.step(2)              # (a call of two updates is a resident launch here: the blocked plane is current again)
            # the two fills agree before either is timed
            new = eng.reach(mask=True, rounds=True, seeds=True, envs=list(range(min(TODAY_ENVS, E))))
            old, turns = torch_reach(torch, eng.fire_maps_torch()[:TODAY_ENVS], conn8)
            assert torch.equal(new["mask"].bool(), old), (size, lines)
            del new, old
            eng.step(2)
            variants = {
                "count": lambda: eng.reach(count=True),
                "count + value": lambda: eng.reach(count=True, value=True),
                "mask": lambda: eng.reach(count=False, mask=True),
                "64 points": lambda: eng.reach(count=False, points=pts),
            }
            r = eng.reach(rounds=True, seeds=True)
            rounds = r["rounds"].cpu().numpy()
            cells, seeds = r["count"].cpu().numpy(), r["seeds"].cpu().numpy()
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
            n = min(TODAY_ENVS, E)
            tor = []
            for rep in range(4):
                eng.sync()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got, turns = torch_reach(torch, eng.fire_maps_torch()[:n], conn8)
                got.sum(dim=(1, 2))
                torch.cuda.synchronize()
                if rep:
                    tor.append((time.perf_counter() - t0) * 1e3 * E / n)
            sci = None
            if ndimage is not None:
                sci = []
                structure = np.ones((3, 3), dtype=bool) if conn8 else ndimage.generate_binary_structure(2, 1)
                for rep in range(3):
                    t0 = time.perf_counter()
                    host = eng.fire_maps()[:n]
                    for e in range(n):
                        open_ = host[e] == 0
                        lab, _ = ndimage.label(open_, structure=structure)
                        touched = ndimage.binary_dilation(host[e] == 1, structure=structure) & open_
                        (np.isin(lab, np.unique(lab[touched])) & open_).sum()
                    sci.append((time.perf_counter() - t0) * 1e3 * E / n)
            assert eng.cell_layout() in (lay, 0)
            step_ms = eng.step_timed(10) / 10.0
            text += (f"\n{E} x {size}^2, about {updates} updates after reset, {'with' if lines else 'without'} control lines: {seeds.mean():.0f} burning cells and "
                     f"{cells.mean():.0f} reachable cells per environment, rounds {rounds.min()} / {int(np.median(rounds))} / {rounds.max()}, "
                     f"one update {step_ms:.3f} ms, cell_layout() {lay}, scratch {eng.reach_scratch_bytes() * E / 2 ** 20:.0f} MiB\n")
            for v in variants:
                m = statistics.median(ms[v])
                text += f"  {v:14s} {med(ms[v])} ms  = {m / step_ms:8.1f} updates\n"
            text += f"  {'torch (device)':14s} {med(tor)} ms  (scaled from {n} environments; {turns} dilations)\n"
            if sci is not None:
                text += f"  {'scipy (host)':14s} {med(sci)} ms  (scaled from {n} environments)\n"
            text += f"  torch / count = {statistics.median(tor) / statistics.median(ms['count']):.0f}\n"
        eng.close()
    print(text)
    if not quick:
        with open(OUT, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
