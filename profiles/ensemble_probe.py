"""Probe: what ensemble statistics cost (sf_ensemble_stats, simfire_amd/csrc/sf_ensemble_kernels.h).

C3's shape (256 x 1024^2), arrival recording on, 100 updates after a reset.  Asynchronous mode, 20 calls between two syncs, wall
microseconds per call, median [min, max] of 7 windows after one warm-up window; the variants take turns window by window:

  (a) G = 1, K = 256, T = 1, ``prob`` only,
  (b) G = 16, K = 16, T = 4, ``count`` + ``first`` + ``mean``,
  (c) (b) + ``loss`` under a shared value plane,
  (d) what (a) returns, assembled in torch from ``arrival_torch()``,
  (e) what (b) returns, assembled in torch from ``arrival_torch()``.

(d) and (e) use nothing this feature adds: they are the yardstick.  For (a) - (c) the bytes the kernel moves (G * K * H * P * 4 read +
the outputs written) over the time give the achieved bandwidth.

  python profiles/ensemble_probe.py            # -> profiles/ensemble_timing.txt
  python profiles/ensemble_probe.py --quick    # 16 x 256^2, nothing written"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "profiles", "ensemble_timing.txt")
REPS, CALLS, UPDATES = 7, 20, 100
PEAK_TBS = 6.3                             # achievable HBM rate of the part


def med(v):
    return "%9.1f [%.1f, %.1f]" % (statistics.median(v), min(v), max(v))


def main():
    import numpy as np
    import torch
    from simfire_amd import workloads
    from simfire_amd.engine import FireEngine
    from values_probe import value_plane
    quick = "--quick" in sys.argv
    size, E = (256, 16) if quick else (1024, 256)
    G2 = 4 if quick else 16
    w = workloads.c3(size, E)
    eng = FireEngine(**w.engine_kwargs())
    eng.set_layers(*w.layers())
    eng.reset(w.init_xy)
    eng.enable_arrival(True)
    eng.values_set(value_plane(size, size))
    eng.step(UPDATES)
    eng.sync()
    P = eng.geometry()["pitch"]
    one = np.arange(E, dtype=np.int32).reshape(1, E)
    many = np.arange(E, dtype=np.int32).reshape(G2, E // G2)
    hz4 = (UPDATES // 4, UPDATES // 2, 3 * UPDATES // 4, -1)
    a1 = eng.arrival_torch()
    many_t = torch.as_tensor(many.astype(np.int64), device=a1.device)

    def torch_a():
        return ((a1 > 0).sum(0).to(torch.float32) / float(E)).reshape(1, 1, size, size)

    def torch_b():
        counts, firsts, means = [], [], []
        for g in range(G2):
            a = a1[many_t[g]]
            counts.append(torch.stack([((a > 0) & (a <= h + 1) if h >= 0 else (a > 0)).sum(0).to(torch.int32) for h in hz4]))
            r = a > 0
            n = r.sum(0)
            firsts.append(torch.where(n > 0, torch.where(r, a - 1, torch.full_like(a, 2 ** 31 - 1)).amin(0), torch.full_like(a[0], -1)))
            s = torch.where(r, a - 1, torch.zeros_like(a)).sum(0)
            means.append(torch.where(n > 0, (s.to(torch.float64) / n.to(torch.float64)).to(torch.float32), torch.full((), -1.0, device=a.device)))
        return torch.stack(counts), torch.stack(firsts), torch.stack(means)

    variants = {
        "a": ("G = 1, K = %d, T = 1, prob" % E, lambda: eng.ensemble_stats(one, horizons=(-1,))),
        "b": ("G = %d, K = %d, T = 4, count + first + mean" % many.shape, lambda: eng.ensemble_stats(many, horizons=hz4, count=True, prob=False, first=True, mean=True)),
        "c": ("(b) + loss", lambda: eng.ensemble_stats(many, horizons=hz4, count=True, prob=False, first=True, mean=True, loss=True)),
        "d": ("(a) assembled in torch", torch_a),
        "e": ("(b) assembled in torch", torch_b),
    }
    cells = size * size
    moved = {"a": E * size * P * 4 + cells * 4, "b": E * size * P * 4 + G2 * cells * 4 * (4 + 2)}
    moved["c"] = moved["b"] + cells * 4 + G2 * 4 * 8

    # the two forms agree before either is timed
    ra, rb = variants["a"][1](), variants["b"][1]()
    eng.sync()
    tb = torch_b()
    assert torch.equal(ra["prob"], torch_a()) and torch.equal(rb["count"], tb[0]) and torch.equal(rb["first"], tb[1]) and torch.equal(rb["mean"], tb[2])
    reached = float(ra["prob"].mean())
    del ra, rb, tb

    eng.set_async(True)
    us = {v: [] for v in variants}
    for rep in range(REPS + 1):
        for v, (_, fn) in variants.items():
            eng.sync()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(CALLS):
                fn()
            eng.sync()
            torch.cuda.synchronize()
            if rep:
                us[v].append((time.perf_counter() - t0) * 1e6 / CALLS)
    text = (f"Ensemble statistics on one MI355X: {E} x {size}^2 (C3), arrival recording on, {UPDATES} updates after a reset (mean burn probability\n"
            f"{reached:.4f}).  Asynchronous mode, {CALLS} calls between two syncs, wall microseconds per call, median [min, max] of {REPS} windows after one\n"
            f"warm-up window; the variants take turns.  Bandwidth: bytes read (G * K * H * P * 4) + bytes written over the median, against {PEAK_TBS} TB/s.\n\n")
    for v, (name, _) in variants.items():
        text += f"  ({v}) {name:48s} {med(us[v])}"
        if v in moved:
            m = statistics.median(us[v])
            text += f"   {moved[v] / 1e6:8.1f} MB  {moved[v] / m / 1e6:5.2f} TB/s  floor {moved[v] / PEAK_TBS / 1e6:6.1f} us ({m / (moved[v] / PEAK_TBS / 1e6):.2f} x)"
        text += "\n"
    text += "\n"
    for x, y in (("a", "d"), ("b", "e")):
        text += (f"  ({x}) against ({y}): the windows {'overlap' if max(min(us[x]), min(us[y])) <= min(max(us[x]), max(us[y])) else 'do not overlap'}, "
                 f"({y}) / ({x}) = {statistics.median(us[y]) / statistics.median(us[x]):.1f}\n")
    text += f"  (c) - (b) = {statistics.median(us['c']) - statistics.median(us['b']):.1f} us\n"
    print(text)
    if not quick:
        with open(OUT, "w") as f:
            f.write(text)


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "profiles"))
    main()
