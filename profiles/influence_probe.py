"""Probe: what fire influence costs (sf_influence, simfire_amd/csrc/sf_influence_kernels.h).

C3's shape (256 x 1024^2) and C5's (64 x 1024^2 with 64 points per environment), spread graph and arrival recording on from the reset,
about 200 updates into the fires.  Timed: the history source (the ignition tree; ``cells``), the forecast source (the ``pred`` plane of a
``travel`` call capped at 64 updates' worth of minutes, made once and fed on; ``cells``) and the point form (64 points per environment
with routes of up to 256 cells, history source, no plane output).  Beside each what the call replaces, timed in this same script on
CHECK_ENVS environments and scaled to the batch: the read-back (``spread_parents`` + ``arrival``, or the ``pred`` rows to the host) and a
level-by-level scatter-add in torch over the same parent pointers, one round per level of the tree.

The handle works on a stream of its own that torch does not know, so a window is a host clock around CALLS asynchronous calls that ends
in ``sync()`` + ``torch.cuda.synchronize()``; every variant is warmed by one window that is not counted, the variants take turns
window by window, and the figure is the median [min, max] of REPS windows.  Before anything is timed the new planes are compared, cell
for cell, with that torch loop on CHECK_ENVS environments, for both sources.  The tree's height and its forest cells are printed beside
the timings: DESIGN.md section 28 states the expected cost in them.  Last, three synthetic planes on 256 x 1024^2 that take the terms
of that estimate apart: no parent anywhere, chains of 8 cells, one chain per row.

  python profiles/influence_probe.py            # -> profiles/influence_timing.txt (its trailing bench.py block is kept)
  python profiles/influence_probe.py --quick    # 8 x 256^2 and 4 x 256^2, nothing written"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "profiles", "influence_timing.txt")
REPS, CALLS, CHECK_ENVS = 7, 2, 2
UPDATES, HORIZON, ROUTE = 200, 64, 256
SRC_OFFSETS = ((+1, +1), (0, +1), (-1, +1), (+1, 0), (-1, 0), (+1, -1), (0, -1), (-1, -1))
T0 = time.perf_counter()


def med(v):
    return "%10.3f [%.3f, %.3f]" % (statistics.median(v), min(v), max(v))


def say(*what):
    """A progress line (stderr, at once): where the probe is and how long it has run."""
    print("[%7.1f s]" % (time.perf_counter() - T0), *what, file=sys.stderr, flush=True)


def torch_parents(torch, codes):
    """Flat parent index int64 [H * W] of an int8 code plane [H, W] on the device (-1: none); the codes are sanitised."""
    H, W = codes.shape
    c = codes.to(torch.int64)
    off = torch.tensor(SRC_OFFSETS, device=codes.device)
    ok = (c >= 0) & (c <= 7)
    o = off[torch.where(ok, c, 0)]
    y, x = torch.meshgrid(torch.arange(H, device=codes.device), torch.arange(W, device=codes.device), indexing="ij")
    nx, ny = x + o[..., 0], y + o[..., 1]
    ok &= (nx >= 0) & (nx < W) & (ny >= 0) & (ny < H)
    return torch.where(ok, ny * W + nx, -1).reshape(-1)


def torch_influence(torch, par):
    """(cells int64 [N], levels): leaves first, one scatter-add per level of the forest.  Acyclic parents only."""
    n = par.numel()
    has = par >= 0
    left = torch.bincount(par[has], minlength=n)
    acc = torch.zeros(n, dtype=torch.int64, device=par.device)
    front = ((left == 0) & has).nonzero().reshape(-1)
    levels = 0
    while front.numel():
        p = par[front]
        acc.index_add_(0, p, acc[front] + 1)
        left.index_add_(0, p, torch.full_like(p, -1))
        up = torch.unique(p)
        front = up[(left[up] == 0) & (par[up] >= 0)]
        levels += 1
    return acc, levels


def history_codes_torch(torch, masks, arr1, bit_to_code):
    """The ignition tree of one environment in torch: uint8 masks [H, W], raw arrival (update + 1, 0 never) int64 [H, W]."""
    H, W = arr1.shape
    F = torch.nn.functional
    best = torch.full((H, W), -1, dtype=torch.int8, device=arr1.device)
    best_a = torch.zeros((H, W), dtype=torch.int64, device=arr1.device)
    ap = F.pad(arr1, (1, 1, 1, 1), value=0)
    code_to_bit = {c: b for b, c in enumerate(bit_to_code)}
    for k, (dx, dy) in enumerate(SRC_OFFSETS):
        an = ap[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
        ok = (((masks.to(torch.int64) >> code_to_bit[k]) & 1) == 1) & (arr1 > 0) & (an > 0) & (an < arr1) & (an > best_a)
        best = torch.where(ok, torch.full_like(best, k), best)
        best_a = torch.where(ok, an, best_a)
    return best


def synthetic(np, torch, FireEngine, E, size):
    """The three terms of DESIGN.md section 28's estimate apart, on hand-made planes shared by E environments of size x size: no
    forest at all (the streaming passes alone), chains of 8 cells (every hop, hardly any height) and one chain per row (height
    size - 1, one walker per row).  Wall ms per call, 2 calls between two syncs, median of 3 windows after a warm-up."""
    H = W = size
    eng = FireEngine(n_envs=E, shape=(H, W), max_fire_duration=4, pixel_scale=30.0, update_rate=1.0, max_time=None, attenuate_line_ros=False,
                     diagonal_spread=True)
    eng.set_rtable(np.full((8, H, W), 1e-3))
    eng.reset(np.zeros((E, 2), dtype=np.int32))
    eng.set_async(True)
    text = f"\nsynthetic planes, {E} x {size}^2, one plane shared by all, `cells` only:\n"
    for kind, what in (("empty", "no parent anywhere"), ("short", "chains of 8 cells along the rows"), ("rows", f"one chain of {W} cells per row")):
        p = np.full((H, W), -1, dtype=np.int8)
        if kind != "empty":
            p[:, 1:] = 4
        if kind == "short":
            p[:, ::8] = -1
        pred, ms = torch.from_numpy(p).cuda(), []
        for rep in range(4):
            eng.sync()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(CALLS):
                eng.influence(pred=pred)
            eng.sync()
            torch.cuda.synchronize()
            if rep:
                ms.append((time.perf_counter() - t0) * 1e3 / CALLS)
        forest = int((p >= 0).sum()) * E
        text += f"  {what:36s} {med(ms)} ms  ({forest} forest cells" + (f", {statistics.median(ms) * 1e6 / forest:.1f} ns each)\n" if forest else ")\n")
        say("synthetic", kind)
    eng.close()
    return text


def main():
    import numpy as np
    import torch
    from simfire_amd import influence, workloads
    from simfire_amd.engine import FireEngine
    quick = "--quick" in sys.argv
    shapes = (("c3", 256, 8), ("c5", 256, 4)) if quick else (("c3", 1024, 256), ("c5", 1024, 64))
    updates = 40 if quick else UPDATES
    text = (f"Fire influence on one MI355X.  Wall milliseconds per call: asynchronous mode, {CALLS} calls between two syncs, median [min, max] of {REPS}\n"
            f"windows after one warm-up window; the variants take turns.  'update': one update of the same handle at that moment (device events\n"
            f"around 10 updates / 10; the spread graph is on, so these are the per-step kernels).  today: what the call replaces, measured on\n"
            f"{CHECK_ENVS} environments and scaled to the batch (see the probe's header).\n")
    for name, size, E in shapes:
        K = 64
        w = workloads.c5(size, E, K) if name == "c5" else workloads.c3(size, E)
        eng = FireEngine(**w.engine_kwargs())
        eng.set_layers(*w.layers())
        eng.enable_spread_graph(True)
        eng.enable_arrival(True)
        eng.reset(w.init_xy)
        H = W = size
        dev = torch.device("cuda:0")
        rate = float(eng.params.update_rate)
        horizon = float(np.float32(HORIZON * rate))
        eng.step(updates)
        say(name, E, size, "rolled out")
        rng = np.random.default_rng(83)
        xy = np.stack([rng.integers(W, size=(E, K)), rng.integers(H, size=(E, K))], axis=-1).astype(np.int32)
        pts = torch.from_numpy(np.concatenate([xy, np.tile(np.arange(1, K + 1), (E, 1))[..., None]], axis=-1).astype(np.int32)).to(dev)
        fore = eng.travel(plane=False, pred=True, reached=True, max_minutes=horizon)
        eng.sync()
        pred = fore["pred"]
        # the check: two environments, both sources, cell for cell against the torch loop; the same loop is what a caller runs today
        n = min(CHECK_ENVS, E)
        got_h = eng.influence(history=True, envs=list(range(n)), pred_out=True, counts=True)
        got_f = eng.influence(pred=pred[:n].contiguous(), envs=list(range(n)), counts=True)
        eng.sync()
        today_h, today_f, heights = [], [], []
        for e in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            masks, arr = torch.from_numpy(eng.spread_parents(e)).to(dev), torch.from_numpy(eng.arrival(e)).to(dev).to(torch.int64) + 1
            codes = history_codes_torch(torch, masks, arr, influence.BIT_TO_CODE)
            ref, lv = torch_influence(torch, torch_parents(torch, codes))
            torch.cuda.synchronize()
            today_h.append((time.perf_counter() - t0) * 1e3)
            assert torch.equal(got_h["pred"][e], codes), (name, e, "history codes")
            assert torch.equal(got_h["cells"][e].reshape(-1).to(torch.int64), ref), (name, e, int((got_h["cells"][e].reshape(-1) != ref).sum()))
            assert int(got_h["cyclic"][e]) == 0
            heights.append(lv)
            t0 = time.perf_counter()
            host = pred[e].cpu()                                  # (the read-back of the pred row a host walk would start from)
            ref, lv_f = torch_influence(torch, torch_parents(torch, host.to(dev)))
            torch.cuda.synchronize()
            today_f.append((time.perf_counter() - t0) * 1e3)
            assert torch.equal(got_f["cells"][e].reshape(-1).to(torch.int64), ref), (name, e, "forecast")
        say(name, "checked against torch", heights)
        counts = eng.influence(history=True, cells=False, counts=True)
        counts_f = eng.influence(pred=pred, cells=False, counts=True)
        eng.sync()
        forest, forest_f = counts["forest"].cpu().numpy(), counts_f["forest"].cpu().numpy()
        routes = eng.influence(history=True, cells=False, points=pts, max_route=ROUTE)
        eng.sync()
        hops = routes["point_hops"].cpu().numpy()
        del got_h, got_f, routes
        variants = {
            "history, cells": lambda: eng.influence(history=True),
            "forecast pred, cells": lambda: eng.influence(pred=pred),
            f"{K} points + routes": lambda: eng.influence(history=True, cells=False, points=pts, max_route=ROUTE),
        }
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
        step_ms = eng.step_timed(10) / 10.0
        need = eng.influence_scratch_bytes()
        text += (f"\n{name}: {E} x {size}^2, about {updates} updates after reset, one update {step_ms:.3f} ms; scratch {need / 2 ** 20:.0f} MiB per environment of a chunk\n"
                 f"  history tree: forest cells per environment {forest.min()} / {int(np.median(forest))} / {forest.max()} (min / median / max), height {heights} levels on the checked ones;\n"
                 f"  forecast tree (cap {HORIZON} updates): forest cells {forest_f.min()} / {int(np.median(forest_f))} / {forest_f.max()};"
                 f" routes: {int((hops >= 0).sum())} of {hops.size} points burned, longest {int(hops.max())} hops, {int((hops == -2).sum())} cut at {ROUTE}\n")
        for v in variants:
            text += f"  {v:22s} {med(ms[v])} ms  = {statistics.median(ms[v]) / step_ms:8.1f} updates\n"
        text += (f"  today, history:  read-back of masks and arrivals + torch levels {statistics.median(today_h):.1f} ms per environment = "
                 f"{statistics.median(today_h) * E:.0f} ms for {E}\n"
                 f"  today, forecast: read-back of pred + torch levels {statistics.median(today_f):.1f} ms per environment = {statistics.median(today_f) * E:.0f} ms for {E}\n")
        eng.close()
        say(name, "done")
        print(text.split("\n\n")[-1], flush=True)
    text += synthetic(np, torch, FireEngine, *((8, 256) if quick else (256, 1024)))
    print(text)
    if not quick:
        # the record also ends with bench.py's lines under the parent commit and under the change, which this probe does not make:
        # a re-run keeps that block as it stands
        kept = ""
        if os.path.exists(OUT):
            old = open(OUT).read()
            at = old.find("\nbench.py ")
            kept = old[at:] if at >= 0 else ""
        with open(OUT, "w") as f:
            f.write(text + kept)


if __name__ == "__main__":
    main()
