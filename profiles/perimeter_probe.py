"""Probe: what the fire's perimeter costs (sf_perimeter, simfire_amd/csrc/sf_perimeter_kernels.h).

C3's shape (256 x 1024^2), BURNING | BURNED, the handle's own connectivity, after 100 and after 500 updates.  Timed:

  summary          the summary form: ``edges`` and ``cells`` (one streaming launch, no scratch)
  summary + front  the same with the ``front`` plane (256 MiB written)
  trace            the trace form with the default capacities (2^18 edges an environment: the list is worked through in chunks
                   under the default budget of 1 GiB)
  trace, tight     the trace form with ``max_edges`` = the power of two above twice the longest perimeter found (one chunk)

and what each replaces, timed in this same script on the same handle:

  torch            ``fire_maps_torch()`` (the refresh of the row-major plane and the wait) plus the same two counts in torch
  host             ``fire_maps()`` (256 MiB to the host) plus the test oracle (tests/_perimeter_oracle.py) on ORACLE_ENVS
                   environments, scaled to all of them and marked as such

The handle works on a stream of its own that torch does not know, so a window is a host clock around CALLS asynchronous calls that
ends in ``sync()`` + ``torch.cuda.synchronize()``; every variant is warmed by one window that is not counted, the variants take turns
window by window, and the figure is the median [min, max] of REPS windows.  Before anything is timed the summary form is compared
with torch on every environment and the trace form with the oracle on ORACLE_ENVS environments, by equality.

  python profiles/perimeter_probe.py            # -> profiles/perimeter_timing.txt
  python profiles/perimeter_probe.py --quick    # 8 x 256^2, nothing written"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OUT = os.path.join(ROOT, "profiles", "perimeter_timing.txt")
REPS, CALLS, ORACLE_ENVS = 7, 2, 4

T0 = time.perf_counter()


def med(v):
    return "%10.3f [%.3f, %.3f]" % (statistics.median(v), min(v), max(v))


def say(*what):
    """A progress line (stderr, at once): where the probe is and how long it has run."""
    print("[%7.1f s]" % (time.perf_counter() - T0), *what, file=sys.stderr, flush=True)


def torch_counts(torch, maps):
    """(edges, cells) int64 [E] of BURNING | BURNED from the uint8 maps [E, H, W], in torch."""
    S = (maps == 1) | (maps == 2)
    cells = S.sum(dim=(1, 2))
    edges = (S[:, 1:] != S[:, :-1]).sum(dim=(1, 2)) + (S[:, :, 1:] != S[:, :, :-1]).sum(dim=(1, 2))
    edges = edges + S[:, 0].sum(dim=1) + S[:, -1].sum(dim=1) + S[:, :, 0].sum(dim=1) + S[:, :, -1].sum(dim=1)
    return edges, cells


def main():
    import numpy as np
    import torch
    import _perimeter_oracle as po
    from simfire_amd import workloads
    from simfire_amd.engine import FireEngine
    quick = "--quick" in sys.argv
    size, E = (256, 8) if quick else (1024, 256)
    stages = (20, 60) if quick else (100, 500)
    text = (f"Fire perimeters on one MI355X, {E} x {size}^2 (C3), BURNING | BURNED.  Wall milliseconds per call: asynchronous mode, {CALLS} calls between\n"
            f"two syncs, median [min, max] of {REPS} windows after one warm-up window; the variants take turns.  'update': one update of the same\n"
            f"handle at that moment (device events around 10 updates / 10).  torch / host: what a caller does today (see the probe's header).\n")
    w = workloads.c3(size, E)
    eng = FireEngine(**w.engine_kwargs())
    eng.set_layers(*w.layers())
    eng.reset(w.init_xy)
    conn = 8 if eng.params.diagonal_spread else 4
    done = 0
    for upd in stages:
        eng.step(upd - done - 2)
        eng.step(2)                  # (a call of two updates is a resident launch here: the blocked plane is current again)
        done = upd
        say(upd, "updates made")
        cheap = eng.perimeter(front=True)
        ne = cheap["edges"].cpu().numpy()
        tight = 1 << int(2 * int(ne.max()) - 1).bit_length()
        full = eng.perimeter(trace=True, max_edges=tight)
        full = {k: v.cpu().numpy() for k, v in full.items()}
        lay = eng.cell_layout()
        maps_t = eng.fire_maps_torch()
        te, tc = torch_counts(torch, maps_t)
        assert torch.equal(te.to(torch.int32), cheap["edges"]) and torch.equal(tc.to(torch.int32), cheap["cells"])
        assert (full["edges"] == ne).all() and (full["cells"] == cheap["cells"].cpu().numpy()).all()
        maps = eng.fire_maps()
        t0 = time.perf_counter()
        for e in range(min(ORACLE_ENVS, E)):
            want = po.answer(po.mask_of_status(maps[e], 6), conn)
            for name in ("edges", "cells", "loops", "holes", "n_vertices"):
                assert int(full[name][e]) == want[name], (upd, e, name)
            nl, nv = want["loops"], want["n_vertices"]
            assert (full["vertices"][e][:nv] == want["vertices"]).all() and (full["loop_start"][e][:nl + 1] == want["loop_start"]).all()
            assert (full["loop_area"][e][:nl] == want["loop_area"]).all() and (full["loop_edges"][e][:nl] == want["loop_edges"]).all()
            assert (cheap["front"][e].cpu().numpy() == want["front"]).all()
        oracle_ms = (time.perf_counter() - t0) * 1e3 / min(ORACLE_ENVS, E)
        say(upd, "checked against torch and the oracle")
        del maps_t, te, tc
        eng.step(2)
        variants = {
            "summary": lambda: eng.perimeter(),
            "summary + front": lambda: eng.perimeter(front=True),
            "trace": lambda: eng.perimeter(trace=True),
            "trace, tight": lambda: eng.perimeter(trace=True, max_edges=tight),
        }
        eng.set_async(True)
        ms = {v: [] for v in variants}
        for rep in range(REPS + 1):
            for v, fn in variants.items():
                eng.sync()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                keep = [fn() for _ in range(CALLS)]
                eng.sync()
                torch.cuda.synchronize()
                if rep:
                    ms[v].append((time.perf_counter() - t0) * 1e3 / CALLS)
                del keep
            say(upd, "window", rep)
        eng.set_async(False)
        assert eng.cell_layout() == lay
        step_ms = eng.step_timed(10) / 10.0
        done += 12
        tor, host = [], []
        for rep in range(4):
            eng.sync()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            te, tc = torch_counts(torch, eng.fire_maps_torch())
            torch.cuda.synchronize()
            if rep:
                tor.append((time.perf_counter() - t0) * 1e3)
            eng.step(2)              # (the next window reads the blocked plane again)
            done += 2
        for rep in range(3):
            eng.sync()
            t0 = time.perf_counter()
            maps = eng.fire_maps()
            host.append((time.perf_counter() - t0) * 1e3)
        from simfire_amd import perimeter
        text += (f"\nabout {upd} updates after reset: perimeter {ne.min()} / {int(np.median(ne))} / {ne.max()} cell edges (min / median / max over the environments), "
                 f"{int(np.median(full['loops']))} loops and {int(np.median(full['n_vertices']))} corners (median), one update {step_ms:.3f} ms, cell_layout() {lay}\n"
                 f"  scratch per environment: default capacities {perimeter.scratch_need(size, size, 1 << 18) / 2 ** 20:.1f} MiB, max_edges {tight}: "
                 f"{perimeter.scratch_need(size, size, tight) / 2 ** 20:.2f} MiB\n")
        for v in variants:
            text += f"  {v:22s} {med(ms[v])} ms  = {statistics.median(ms[v]) / step_ms:8.1f} updates\n"
        text += f"  {'torch':22s} {med(tor)} ms  (fire_maps_torch() + the two counts in torch); summary / that = {statistics.median(ms['summary']) / statistics.median(tor):.3f}\n"
        h = statistics.median(host)
        text += (f"  {'host':22s} {med(host)} ms  fire_maps() alone; the oracle {oracle_ms:.1f} ms an environment ({min(ORACLE_ENVS, E)} timed), scaled to {E}: "
                 f"{h + oracle_ms * E:.0f} ms; trace, tight / that = {statistics.median(ms['trace, tight']) / (h + oracle_ms * E):.4f}\n")
        print(text.split("\n\n")[-1], flush=True)
    eng.close()
    print(text)
    if not quick:
        with open(OUT, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
