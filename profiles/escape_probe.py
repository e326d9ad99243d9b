"""Probe: what the escape slack costs (sf_escape, simfire_amd/csrc/sf_escape_kernels.h).

C3's shape (256 x 1024^2) and C5's (64 x 1024^2): one band per thread, k_escape<true>.  A fire about 200 updates old; the targets
are the grid's border, the walkable cells UNBURNED, the agents' four moves.  The closing times are ``travel`` up to the horizon,
computed ONCE outside the windows (its cost is section 26's, printed beside); the horizon is 64 and 512 moves, a move being
horizon / moves minutes.  Timed: 64 points per environment, and the plane form; beside each the largest deadline and the cells by
slack, one update of the same handle at that moment (``step_timed``), and what a caller does today, timed in this same script:

  torch   the same procedure on the device: the deadlines from the minutes plane, a flood over the NEVER cells, then one level per
          move index from the top down (``max_pool2d`` of the whole safe set, times the cells open at that level, a level number
          written where a cell is new), on TODAY_ENVS environments and scaled to the batch.

The yardstick is that path, not the new code.  The handle works on a stream of its own that torch does not know, so a window is a
host clock around CALLS asynchronous calls that ends in ``sync()`` + ``torch.cuda.synchronize()``; every variant is warmed by one
window that is not counted, the variants take turns window by window, and the figure is the median [min, max] of REPS windows;
the torch loop is run TODAY_REPS times after one warm-up run.
Before anything is timed the new plane is compared with the torch loop, cell for cell.

  python profiles/escape_probe.py            # -> profiles/escape_timing.txt
  python profiles/escape_probe.py --quick    # 8 x 256^2, nothing written"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "profiles", "escape_timing.txt")
REPS, CALLS, TODAY_ENVS, TODAY_REPS = 7, 3, 2, 3
HORIZON_ENVS, FALLBACK_MINUTES = 8, 100.0
UPDATES = 200
SAFE = 2 ** 31 - 1


def med(v):
    return "%10.3f [%.3f, %.3f]" % (statistics.median(v), min(v), max(v))


def torch_slack(torch, maps, minutes, targets, per_move, horizon):
    """The escape slack of uint8 maps [n, H, W] under float32 minutes [n, H, W], targets bool [H, W], over the four moves, margin 0:
    what a caller can write today.  Returns (int32 plane, levels run)."""
    F = torch.nn.functional

    def grow(a):
        a = a.to(torch.float16).unsqueeze(1)
        return (torch.maximum(F.max_pool2d(a, (3, 1), 1, (1, 0)), F.max_pool2d(a, (1, 3), 1, (0, 1))) > 0).squeeze(1)
    tgt = targets.unsqueeze(0).expand_as(maps)
    walk = (maps == 0) & ~tgt
    never = (minutes < 0) | ~(minutes.double() < horizon)
    D = torch.where(never, SAFE, torch.clamp(torch.ceil(minutes.double() / per_move), min=0).to(torch.int64)).to(torch.int64)
    S = torch.where(tgt, SAFE, torch.where(walk, -1, -2)).to(torch.int32)
    A = tgt.clone()
    U = walk & never
    while True:                               # the flood through the NEVER cells
        new = grow(A) & U
        if not bool(new.any()):
            break
        A |= new
        U &= ~new
    S = torch.where(A & walk, SAFE, S)
    finite = walk & ~never
    top = int(D[finite].max()) if bool(finite.any()) else 0
    for v in range(top - 1, -1, -1):
        new = grow(A) & ((walk & (D > v)) & ~A)
        S = torch.where(new, v, S)
        A |= new
    return S, top


def main():
    import numpy as np
    import torch
    from simfire_amd import workloads
    from simfire_amd.engine import FireEngine
    quick = "--quick" in sys.argv
    shapes = (("c3", 256, 8),) if quick else (("c3", 1024, 256), ("c5", 1024, 64))
    updates = 40 if quick else UPDATES
    text = (f"Escape slack on one MI355X.  Wall milliseconds per call: asynchronous mode, {CALLS} calls between two syncs, median [min, max] of {REPS}\n"
            f"windows after one warm-up window; the variants take turns.  'update': one update of the same handle at that moment (device events\n"
            f"around 10 updates / 10).  The closing times come from one travel call outside the windows (its own wall time is printed).  torch:\n"
            f"what a caller does today (see the probe's header), timed on {TODAY_ENVS} environments and scaled to the batch, median [min, max] of {TODAY_REPS} runs\n"
            f"after one warm-up run.\n")
    for name, size, E in shapes:
        K = 64
        w = workloads.c5(size, E, K) if name == "c5" else workloads.c3(size, E)
        eng = FireEngine(**w.engine_kwargs())
        eng.set_layers(*w.layers())
        eng.reset(w.init_xy)
        H = W = size
        dev = torch.device("cuda:0")
        rng = np.random.default_rng(83)
        xy = np.stack([rng.integers(W, size=(E, K)), rng.integers(H, size=(E, K))], axis=-1).astype(np.int32)
        pts = torch.from_numpy(np.concatenate([xy, np.tile(np.arange(1, K + 1), (E, 1))[..., None]], axis=-1).astype(np.int32)).to(dev)
        tg = torch.zeros((H, W), dtype=torch.uint8, device=dev)
        tg[0, :] = tg[H - 1, :] = 1
        tg[:, 0] = tg[:, W - 1] = 1
        eng.step(updates)
        eng.step(2)                  # (a call of two updates is a resident launch here: the blocked plane is current again)
        step_ms = eng.step_timed(10) / 10.0
        # the horizon, in minutes: the median finite travel time over the first HORIZON_ENVS environments - a time in which their
        # fires cross a good part of the grid; FALLBACK_MINUTES when none of them burns any more (the text says which it was)
        free = eng.travel(plane=True, envs=list(range(min(HORIZON_ENVS, E))))["minutes"]
        free = free[torch.isfinite(free) & (free > 0)]
        horizon = float(torch.quantile(free[:: max(1, free.numel() // 100000)], 0.5)) if free.numel() else FALLBACK_MINUTES
        source = f"the median finite travel time of the first {min(HORIZON_ENVS, E)} environments" if free.numel() else "the fallback: none of them burns"
        del free
        n = min(TODAY_ENVS, E)
        text += (f"\n{name}: {E} x {size}^2, about {updates} updates after reset, one update {step_ms:.3f} ms, cell_layout() {eng.cell_layout()}, "
                 f"scratch {eng.escape_scratch_bytes() * E / 2 ** 20:.0f} MiB; horizon {horizon:.1f} minutes ({source})\n")
        for moves in (64, 512):
            per_move = horizon / moves
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mins = eng.travel(max_minutes=float(np.float32(horizon)), plane=True)["minutes"]
            eng.sync()
            travel_ms = (time.perf_counter() - t0) * 1e3
            kw = dict(targets=tg, minutes_per_move=per_move, horizon_minutes=horizon)
            # the two searches agree before either is timed
            new = eng.escape(mins[:n], envs=list(range(n)), plane=True, summary=True, **kw)
            old, top = torch_slack(torch, eng.fire_maps_torch()[:n], mins[:n], tg.bool(), per_move, horizon)
            assert torch.equal(new["slack"], old), (name, size, moves, int((new["slack"] != old).sum()))
            del new, old
            variants = {f"{K} points": lambda: eng.escape(mins, points=pts, step=True, **kw),
                        "plane": lambda: eng.escape(mins, plane=True, **kw)}
            s = eng.escape(mins, summary=True, **kw)
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
            for rep in range(TODAY_REPS + 1):       # (one call is a window here: hundreds of launches; the first is the warm-up)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                torch_slack(torch, eng.fire_maps_torch()[:n], mins[:n], tg.bool(), per_move, horizon)
                torch.cuda.synchronize()
                if rep:
                    tor.append((time.perf_counter() - t0) * 1e3 * E / n)
            text += (f" horizon {moves} moves ({horizon:.1f} minutes): top {int(s['top'].min())} / {int(s['top'].max())}, per environment safe "
                     f"{float(s['safe'].float().mean()):.0f}, escapable {float(s['escapable'].float().mean()):.0f}, lost {float(s['lost'].float().mean()):.0f}; "
                     f"travel to the horizon {travel_ms:.3f} ms\n")
            for v in variants:
                m = statistics.median(ms[v])
                text += f"  {v:18s} {med(ms[v])} ms  = {m / step_ms:8.1f} updates\n"
            text += f"  {'torch (device)':18s} {med(tor)} ms  (scaled from {n} environments; {top} levels)\n"
            text += f"  torch / plane = {statistics.median(tor) / statistics.median(ms['plane']):.0f}\n"
            del mins
        eng.close()
    print(text)
    if not quick:
        with open(OUT, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
