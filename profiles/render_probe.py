"""Probe: frames (sf_render, simfire_amd/csrc/sf_render_kernels.h) at BASELINE C3 (256 x 1024^2), and what recording=True adds to
FireSimulation.run at 1024^2.

  python profiles/render_probe.py [--out FILE]          # default: profiles/render_timing.txt

Per case: `sync` = wall time of one synchronous render into a preallocated tensor (host work + launch + kernel + wait), median of
15; `pipelined` = 20 renders enqueued back to back in async mode and one sync, divided by 20.  The background is built once, before
the timed calls.  Bytes: the status bytes k_render reads (1 B per cell row-major, 2 B per cell blocked: the status half of each
64-byte sector comes with the mask half), the shared background once (4 B per cell) and the output; share of 8 TB/s (peak) and of
6.3 TB/s (achievable) from the pipelined time.  Recording: the same FireSimulation.run(k) with recording False and True (fuel
background, scale 1, frames fetched to the host), per executed update."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from simfire_amd.engine import FireEngine  # noqa: E402
from simfire_amd.workloads import c3  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "render_timing.txt")


def time_render(eng, kw):
    out = eng.render(**kw)
    torch.cuda.synchronize()
    t = []
    for _ in range(15):
        t0 = time.perf_counter()
        eng.render(out=out, **kw)
        t.append(time.perf_counter() - t0)
    eng.set_async(True)
    eng.sync()
    t0 = time.perf_counter()
    for _ in range(20):
        eng.render(out=out, **kw)
    eng.sync()
    pipe = (time.perf_counter() - t0) / 20
    eng.set_async(False)
    return statistics.median(t), pipe, out.numel()


def fire_sim(size):
    import yaml
    from simfire_amd.config import Config
    from simfire_amd.simulation import FireSimulation
    y = yaml.safe_load(open(os.path.join(ROOT, "tests", "golden", "configs", "functional_config.yml")))
    y["area"]["screen_size"] = [size, size]
    y["simulation"]["headless"] = True
    return FireSimulation(Config(config_dict=y, simplex_topography=True))


def recording_cost(size=1024, k=128):
    res = {}
    for rec in (False, True):
        sim = fire_sim(size)
        sim.recording = rec
        sim.run(4)                                    # warm-up (history ring, background, first launches)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sim.run(k)
        dt = time.perf_counter() - t0
        res[rec] = (dt, sim.elapsed_steps - 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    w = c3()
    E, (H, W) = w.n_envs, w.shape
    lines = [f"Frames at C3 ({E} x {H}x{W}) on one MI355X: sf_render, fuel background with contours, agents none.",
             "sync = one synchronous call (median of 15), pipelined = 20 calls enqueued in async mode / 20; bytes = status read + "
             "background once + output.", ""]
    for layout, fused, steps in (("blocked (after a resident run)", 2, 20), ("row-major (after per-step kernels)", 0, 1)):
        eng = FireEngine(**w.engine_kwargs())
        eng.set_layers(*w.layers())
        eng.reset(w.init_xy)
        eng.set_fused(fused)
        eng.step(steps)
        got = eng.cell_layout()
        lines.append(f"layout: {layout}  (cell_layout() = {got})")
        for scale, mode in ((1, "nearest"), (4, "sprites"), (4, "mean")):
            sync, pipe, n_out = time_render(eng, dict(scale=scale, mode=mode))
            total = E * H * W * (2 if got else 1) + 4 * H * W + n_out
            lines.append(f"  scale {scale} {mode:8s} sync {sync * 1e6:9.1f} us  pipelined {pipe * 1e6:9.1f} us  bytes {total / 1e6:7.1f} MB  "
                         f"({100 * total / pipe / 8e12:5.1f} % of 8 TB/s, {100 * total / pipe / 6.3e12:5.1f} % of 6.3 TB/s)")
            print(lines[-1], flush=True)
        eng.close()
        lines.append("")
    res = recording_cost()
    (t0, n0), (t1, n1) = res[False], res[True]
    lines.append(f"FireSimulation.run(128) at 1024^2: recording off {t0 * 1e6 / max(n0, 1):9.1f} us per update ({n0} updates), "
                 f"on {t1 * 1e6 / max(n1, 1):9.1f} us per update ({n1} updates): +{(t1 / max(n1, 1) - t0 / max(n0, 1)) * 1e6:.1f} us per update")
    print(lines[-1], flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
