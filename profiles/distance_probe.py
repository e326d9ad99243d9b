"""Probe: what distance fields cost (sf_distance, simfire_amd/csrc/sf_dist_kernels.h).

C3's shape (256 x 1024^2) and C5's (64 x 1024^2, 64 points per environment), 20 and 500 updates after a reset, masks {BURNING} and
{BURNING, BURNED}.  Timed: the plane form (float32) capped at 16 and 64 cells and without a cap, and the point form (uncapped).
Beside each: one update of the same handle at that moment (``step_timed``, 10 updates / 10, taken after the distance windows of the
moment), the bytes the form must move (from the shapes), and what a caller does today, timed in this same script:

  torch   ``fire_maps_torch()`` (waits for the handle's stream, sweeps the blocked plane into the row-major one) + a capped exact
          distance transform written in torch on the device (column distances by cummax / cummin, then the 2 R + 1 shifted minima);
  scipy   ``fire_maps_torch()`` + copy to the host + ``scipy.ndimage.distance_transform_edt`` per environment (uncapped; timed on
          SCIPY_ENVS environments, the figure for the whole batch is that time scaled by their number) - where scipy imports.

The yardstick is that path, not the new code.  The handle works on a stream of its own that torch does not know, so a window is a
host clock around CALLS asynchronous calls that ends in ``sync()`` + ``torch.cuda.synchronize()`` (the step's figure comes from the
library's own device events); every variant is warmed by one window that is not counted, the new calls take turns window by window and
then the torch formulations do, and the figure is the median [min, max] of REPS windows.  Before anything is timed the new plane is compared with the torch
formulation, value for value.

  python profiles/distance_probe.py            # -> profiles/distance_timing.txt
  python profiles/distance_probe.py --quick    # 8 x 256^2, nothing written"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "profiles", "distance_timing.txt")
REPS, CALLS, SCIPY_ENVS = 7, 3, 4
MOMENTS = (20, 500)
MASKS = (("BURNING",), ("BURNING", "BURNED"))
CAPS = (16, 64, None)


def med(v):
    return "%10.2f [%.2f, %.2f]" % (statistics.median(v), min(v), max(v))


def torch_capped_d2(torch, maps, statuses, R):
    """Exact min(d2, R * R) of uint8 maps [n, H, W] on the device, int32: what a caller can write today."""
    n, H, W = maps.shape
    src = torch.zeros_like(maps, dtype=torch.bool)
    for s in statuses:
        src |= maps == s
    rows = torch.arange(H, device=maps.device, dtype=torch.int32).view(1, H, 1)
    big = 1 << 20
    last = torch.where(src, rows, torch.full_like(rows, -big)).cummax(dim=1).values
    nxt = torch.where(src, rows, torch.full_like(rows, big)).flip(1).cummin(dim=1).values.flip(1)
    g = torch.minimum(rows - last, nxt - rows).clamp_(max=R + 1)
    g2 = torch.where(g > R, torch.full_like(g, big * 8), g * g)
    best = torch.full_like(g2, R * R)
    for r in range(-R, R + 1):
        if r >= 0:
            best[:, :, :W - r] = torch.minimum(best[:, :, :W - r], g2[:, :, r:] + r * r)
        else:
            best[:, :, -r:] = torch.minimum(best[:, :, -r:], g2[:, :, :W + r] + r * r)
    return best


def main():
    import numpy as np
    import torch
    from simfire_amd import workloads
    from simfire_amd.engine import FireEngine
    try:
        from scipy.ndimage import distance_transform_edt
    except ImportError:
        distance_transform_edt = None
    quick = "--quick" in sys.argv
    size = 256 if quick else 1024
    shapes = (("C3", 8 if quick else 256, 0), ("C5", 4 if quick else 64, 64))
    moments = (5, 40) if quick else MOMENTS
    text = (f"Distance fields on one MI355X.  Wall milliseconds per call: asynchronous mode, {CALLS} calls between two syncs, median [min, max] of {REPS}\n"
            f"windows after one warm-up window; the new calls of a moment take turns, then the torch formulations do.  'update': one update of the same handle at that moment (device events\n"
            f"around 10 updates / 10).  'moved': the bytes the form must move, from the shapes.  torch / scipy: what a caller does today (see the probe's\n"
            f"header); scipy is timed on {SCIPY_ENVS} environments and scaled to the batch.\n")
    for label, E, k in shapes:
        w = (workloads.c5(size, E, k) if k else workloads.c3(size, E))
        eng = FireEngine(**w.engine_kwargs())
        eng.set_layers(*w.layers())
        eng.reset(w.init_xy)
        H = W = size
        P = eng.geometry()["pitch"]
        dev = torch.device("cuda:0")
        kk = k or 64
        rng = np.random.default_rng(77)
        pts = torch.from_numpy(np.stack([rng.integers(W, size=(E, kk)), rng.integers(H, size=(E, kk)), np.tile(np.arange(1, kk + 1), (E, 1))],
                                        axis=-1).astype(np.int32)).to(dev)
        out_plane = torch.empty((E, H, W), dtype=torch.float32, device=dev)
        out_pts = torch.empty((E, kk), dtype=torch.float32, device=dev)
        # bytes from the shapes: status read once, g written by the pass down, read and (at most) written by the pass up, read by the
        # row pass; the plane form writes 4 bytes per cell, the point form reads k rows' worth at most and writes k values
        cols = E * H * P * (1 + 2 + 2 + 2)
        moved = {"plane": cols + E * H * P * 2 + E * H * W * 4, "points": cols + E * kk * (12 + 4 + 2 * P)}
        today = {"torch R": "E*H*W * (1 sweep + 1 read + ~12 per shifted minimum * (2 R + 1))", "scipy": E * H * W * (1 + 1 + 1 + 8)}
        done = 0
        for upd in moments:
            eng.set_async(False)
            eng.step(upd - done)
            done = upd
            for names in MASKS:
                statuses = [dict(UNBURNED=0, BURNING=1, BURNED=2)[s] for s in names]
                # the two forms agree before either is timed (R = 16)
                new = eng.distance(names, max_dist=16, dtype="int32")
                old = torch_capped_d2(torch, eng.fire_maps_torch(), statuses, 16)
                assert torch.equal(new, old), (label, upd, names)
                sel = int(((old == 0).sum()).item())
                del new, old
                eng.step(2)                  # (a call of two updates is a resident launch here: the blocked plane is current again)
                done += 2
                variants = {}
                for R in CAPS:
                    variants["plane R=%s" % R] = lambda R=R: eng.distance(names, max_dist=R, out=out_plane)
                variants["points k=%d" % kk] = lambda: eng.distance(names, points=pts, out=out_pts)
                for R in (16, 64):
                    variants["torch R=%d" % R] = lambda R=R: torch_capped_d2(torch, eng.fire_maps_torch(), statuses, R)
                eng.set_async(True)
                ms = {v: [] for v in variants}
                # the new calls first, then the torch formulations; cell_layout() is noted in front of each group and behind both (the
                # blocked plane stays current throughout: fire_maps_torch() sweeps it into the row-major snapshot on every call)
                lays = []
                for group in ([v for v in variants if not v.startswith("torch")], [v for v in variants if v.startswith("torch")]):
                    lays.append(eng.cell_layout())
                    for rep in range(REPS + 1):
                        for v in group:
                            fn = variants[v]
                            calls = 1 if v.startswith("torch") else CALLS
                            eng.sync()
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            for _ in range(calls):
                                fn()
                            eng.sync()
                            torch.cuda.synchronize()
                            if rep:
                                ms[v].append((time.perf_counter() - t0) * 1e3 / calls)
                sci = None
                if distance_transform_edt is not None:
                    sci = []
                    for rep in range(3):
                        eng.sync()
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        host = eng.fire_maps_torch()[:SCIPY_ENVS].cpu().numpy()
                        for e in range(min(SCIPY_ENVS, E)):
                            src = np.zeros((H, W), dtype=bool)
                            for s in statuses:
                                src |= host[e] == s
                            distance_transform_edt(~src).astype(np.float32)
                        sci.append((time.perf_counter() - t0) * 1e3 * E / min(SCIPY_ENVS, E))
                eng.set_async(False)
                lays.append(eng.cell_layout())
                step_ms = eng.step_timed(10) / 10.0
                done += 10
                text += (f"\n{label}: {E} x {size}^2, {upd} updates after reset (+ {done - upd} by now), mask {'+'.join(names)} ({sel / E:.0f} selected cells per environment), "
                         f"one update {step_ms:.3f} ms; cell_layout() before the new calls, before the torch calls, behind them: {lays}\n")
                for v in variants:
                    m = statistics.median(ms[v])
                    text += f"  {v:14s} {med(ms[v])} ms  = {m / step_ms:8.1f} updates"
                    key = "plane" if v.startswith("plane") else ("points" if v.startswith("points") else None)
                    if key:
                        text += f"   moved {moved[key] / 1e6:8.1f} MB ({moved[key] / m / 1e9:.2f} TB/s)"
                    else:
                        text += f"   moved {today['torch R']}"
                    text += "\n"
                if sci is not None:
                    text += f"  {'scipy (host)':14s} {med(sci)} ms  (scaled from {min(SCIPY_ENVS, E)} environments)   moved {today['scipy'] / 1e6:.1f} MB over the host link and memory\n"
                for R in (16, 64):
                    a, b = ms["plane R=%d" % R], ms["torch R=%d" % R]
                    text += (f"  torch R={R} / plane R={R} = {statistics.median(b) / statistics.median(a):.1f}; the windows "
                             f"{'overlap' if max(min(a), min(b)) <= min(max(a), max(b)) else 'do not overlap'}\n")
        eng.close()
        del out_plane, out_pts
    print(text)
    if not quick:
        with open(OUT, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
