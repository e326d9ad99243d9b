"""Probe: what the fire's travel time costs (sf_travel, simfire_amd/csrc/sf_travel_kernels.h).

C3's shape (256 x 1024^2), C5's (64 x 1024^2 with 64 points per environment) and 128 x 2048^2, a fire about 200 updates old, BURNING
through UNBURNED, the handle's own connectivity.  Timed: the point form capped at a horizon of 64 updates' worth of minutes, the point
form uncapped and the full plane; beside each the tile activations of the search (min / median / max over the environments) and one
update of the same handle at that moment (``step_timed``).  Then what the call replaces, timed in this same script on the same handle:

  fork    ``copy_envs`` of the first half of the environments onto the second half, arrival recording on, a rollout of the horizon's
          64 updates (the whole handle steps: E environments, half of them forks), ``sync``.  The far corners need the fire's whole
          remaining life instead of 64 updates: that figure is the 64-update one scaled by last / horizon and marked as such.

The handle works on a stream of its own that torch does not know, so a window is a host clock around CALLS asynchronous calls that ends
in ``sync()`` + ``torch.cuda.synchronize()``; every variant is warmed by one window that is not counted, the variants take turns
window by window, and the figure is the median [min, max] of REPS windows.  Before anything is timed the new plane is compared, cell
for cell, with a Jacobi relaxation in torch (float32 sums over the same float32 weights, to the fixed point) on CHECK_ENVS environments.
Last, on C3's windy terrain: how far the forecast is from the automaton - the distribution of arrival * update_rate / minutes over the
cells a real rollout of 200 updates reaches, the forecast made right after the reset.

  python profiles/travel_probe.py            # -> profiles/travel_timing.txt
  python profiles/travel_probe.py --quick    # 8 x 256^2 and 4 x 512^2, nothing written"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "profiles", "travel_timing.txt")
REPS, CALLS, CHECK_ENVS = 7, 2, 2
UPDATES, HORIZON = 200, 64
SRC_OFFSETS = ((+1, +1), (0, +1), (-1, +1), (+1, 0), (-1, 0), (+1, -1), (0, -1), (-1, -1))


def med(v):
    return "%10.3f [%.3f, %.3f]" % (statistics.median(v), min(v), max(v))


T0 = time.perf_counter()


def say(*what):
    """A progress line (stderr, at once): where the probe is and how long it has run."""
    print("[%7.1f s]" % (time.perf_counter() - T0), *what, file=sys.stderr, flush=True)


def torch_minutes(torch, fire_map, R8, pixel_scale, diag):
    """The minutes plane of one environment by Jacobi relaxation on the device: uint8 map [H, W], float64 table [8, H, W]."""
    F = torch.nn.functional
    inf = float("inf")
    H, W = fire_map.shape
    w = torch.where(R8 > 0, (pixel_scale / R8), torch.full_like(R8, inf)).to(torch.float32)
    src, opn = fire_map == 1, fire_map == 0
    T = torch.where(src, 0.0, inf).to(torch.float32)
    ks = [k for k, (ox, oy) in enumerate(SRC_OFFSETS) if diag or ox == 0 or oy == 0]
    while True:
        before = T
        for _ in range(32):
            Tp = F.pad(torch.where(src | opn, T, inf), (1, 1, 1, 1), value=inf)
            best = T
            for k in ks:
                ox, oy = SRC_OFFSETS[k]
                best = torch.minimum(best, Tp[1 + oy:1 + oy + H, 1 + ox:1 + ox + W] + w[k])
            T = torch.where(opn, best, T)
        if torch.equal(before, T):
            return torch.where(src | opn, T, -1.0)


def main():
    import numpy as np
    import torch
    from simfire_amd import workloads
    from simfire_amd.engine import FireEngine
    quick = "--quick" in sys.argv
    shapes = (("c3", 256, 8), ("c4", 512, 4)) if quick else (("c3", 1024, 256), ("c5", 1024, 64), ("c4", 2048, 128))
    updates = 40 if quick else UPDATES
    text = (f"Fire travel time on one MI355X.  Wall milliseconds per call: asynchronous mode, {CALLS} calls between two syncs, median [min, max] of {REPS}\n"
            f"windows after one warm-up window; the variants take turns.  'update': one update of the same handle at that moment (device events\n"
            f"around 10 updates / 10).  activations: tiles the search loaded, min / median / max over the environments.  fork: what a caller does\n"
            f"today (see the probe's header).\n")
    ratio_text = ""
    for name, size, E in shapes:
        K = 64
        w = workloads.c5(size, E, K) if name == "c5" else (workloads.c4(size, E) if name == "c4" else workloads.c3(size, E))
        kw = w.engine_kwargs()
        eng = FireEngine(**kw)
        eng.set_layers(*w.layers())
        eng.reset(w.init_xy)
        say(name, E, size, "built")
        H = W = size
        dev = torch.device("cuda:0")
        rate, ps, diag = float(eng.params.update_rate), float(eng.params.pixel_scale), bool(eng.params.diagonal_spread)
        horizon = float(np.float32(HORIZON * rate))
        if name == "c3":
            # the forecast at the reset against the automaton's own arrival, on a few environments
            eng.enable_arrival(True)
            n = min(8, E)
            fore = eng.travel(envs=list(range(n)))["minutes"].cpu().numpy()
            eng.step(updates)
            q = []
            for e in range(n):
                arr = eng.arrival(e)
                ok = (arr > 0) & (fore[e] > 0) & np.isfinite(fore[e])
                q.append(arr[ok] * rate / fore[e][ok])
            q = np.concatenate(q)
            ratio_text = (f"\nc3's terrain, {n} environments, the forecast made right after the reset against the arrival plane of a rollout of {updates} updates:\n"
                          f"  arrival * update_rate / minutes over {q.size} cells: median {np.median(q):.3f}, 5 % {np.quantile(q, 0.05):.3f}, 95 % {np.quantile(q, 0.95):.3f}, "
                          f"min {q.min():.3f}, max {q.max():.3f}\n")
            eng.enable_arrival(False)
            say(name, "forecast against arrival done")
        else:
            eng.step(updates)
        eng.step(2)                  # (a call of two updates is a resident launch here: the blocked plane is current again)
        rng = np.random.default_rng(79)
        xy = np.stack([rng.integers(W, size=(E, K)), rng.integers(H, size=(E, K))], axis=-1).astype(np.int32)
        pts = torch.from_numpy(np.concatenate([xy, np.tile(np.arange(1, K + 1), (E, 1))[..., None]], axis=-1).astype(np.int32)).to(dev)
        n = min(CHECK_ENVS, E)
        new = eng.travel(envs=list(range(n)))["minutes"]
        maps = eng.fire_maps_torch()
        for e in range(n):
            ref = torch_minutes(torch, maps[e], torch.from_numpy(eng.get_rtable(e)).to(dev), ps, diag)
            assert torch.equal(new[e], ref), (name, size, e, int((new[e] != ref).sum()))
        del new, maps
        say(name, "checked against torch")
        eng.step(2)
        variants = {
            f"{K} points, cap {HORIZON} upd": lambda: eng.travel(points=pts, plane=False, max_minutes=horizon),
            f"{K} points": lambda: eng.travel(points=pts, plane=False),
            "plane": lambda: eng.travel(plane=True),
        }
        r = eng.travel(plane=False, reached=True, last=True, activations=True)
        rc = eng.travel(plane=False, activations=True, max_minutes=horizon)
        acts, acts_c = r["activations"].cpu().numpy(), rc["activations"].cpu().numpy()
        cells, last = r["reached"].cpu().numpy(), r["last"].cpu().numpy()
        lay = eng.cell_layout()
        say(name, "activations", int(acts.max()), int(acts_c.max()))
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
            say(name, "window", rep)
        eng.set_async(False)
        assert eng.cell_layout() == lay
        step_ms = eng.step_timed(10) / 10.0
        # what the call replaces: fork, record arrivals, roll the copies out
        half = E // 2
        fork = []
        for rep in range(3):
            eng.sync()
            t0 = time.perf_counter()
            eng.copy_envs(list(range(half)), list(range(half, 2 * half)))
            eng.enable_arrival(True)
            eng.step(HORIZON)
            eng.sync()
            fork.append((time.perf_counter() - t0) * 1e3)
            eng.enable_arrival(False)
        tiles = ((size + 31) // 32) ** 2
        text += (f"\n{name}: {E} x {size}^2 ({tiles} tiles), about {updates} updates after reset: {cells.mean():.0f} cells with a route per environment, the last after "
                 f"{np.median(last):.0f} minutes = {np.median(last) / rate:.0f} updates (median), one update {step_ms:.3f} ms, cell_layout() {lay}, "
                 f"scratch {eng.travel_scratch_bytes() * E / 2 ** 20:.0f} MiB\n"
                 f"  activations: capped {acts_c.min()} / {int(np.median(acts_c))} / {acts_c.max()}, uncapped {acts.min()} / {int(np.median(acts))} / {acts.max()}"
                 f" ({np.median(acts) / tiles:.1f} per tile)\n")
        for v in variants:
            m = statistics.median(ms[v])
            text += f"  {v:22s} {med(ms[v])} ms  = {m / step_ms:8.1f} updates\n"
        f64 = statistics.median(fork)
        text += f"  {'fork + ' + str(HORIZON) + ' updates':22s} {med(fork)} ms  ({half} forks, the whole handle steps)\n"
        text += (f"  fork to the far corners (scaled by last / horizon = {np.median(last) / horizon:.1f}): {f64 * np.median(last) / horizon:.0f} ms; "
                 f"plane / that = {statistics.median(ms['plane']) / (f64 * np.median(last) / horizon):.2f}\n")
        eng.close()
        say(name, "done")
        print(text.split("\n\n")[-1], flush=True)
    text += ratio_text
    print(text)
    if not quick:
        with open(OUT, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
