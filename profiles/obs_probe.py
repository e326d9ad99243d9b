"""Probe: observation tensors (sf_observe, simfire_amd/csrc/sf_obs_kernels.h) at BASELINE C3 (256 x 1024^2) against the torch pipeline
they replace (fire_maps_torch + attribute_data_torch + casts / one-hot / min-max / stack / pooling / cropping).

  python profiles/obs_probe.py                 # -> profiles/obs_timing.txt

Cases: (1) fire_map only, full resolution; (2) 9 channels (fire_map, 6 indicators, elevation, wind_speed), pool 8, mean; (3) the same
9 channels in a 128^2 crop around per-environment centers, pool 2.  Each in both layouts: after a resident run (the blocked plane is
current) and after per-step kernels (row-major plane).  Per call: `sync` = wall time of one synchronous observe into a preallocated
tensor (host work + launch + kernel + wait), median of 15; `pipelined` = wall time of 30 observes enqueued back to back in async mode
and one sync, divided by 30 (the GPU's time per call once the host runs ahead).  Bytes: the status bytes the kernel reads (1 B per cell
row-major, 2 B per cell blocked: the status half of each 64-byte sector comes with the mask half), the attribute planes once (one
shared table, 8 B per cell and plane) and the output; fraction of 6.3 TB/s from the pipelined time."""
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

OUT = os.path.join(ROOT, "profiles", "obs_timing.txt")
NINE = ["fire_map"] + [f"burn_status:{s}" for s in ("UNBURNED", "BURNING", "BURNED", "FIRELINE", "SCRATCHLINE", "WETLINE")] + \
       ["elevation", "wind_speed"]
BOUNDS = {"elevation": (-282.0, 11000.0), "wind_speed": (0.0, 250.0)}
HBM = 6.3e12


def cases(E, H, W):
    rng = np.random.default_rng(7)
    centers = np.stack([rng.integers(0, W, E), rng.integers(0, H, E)], 1).astype(np.int32)
    return [("1 fire_map, full resolution", dict(channels=["fire_map"], pool=1), 1, 0, 4 * H * W),
            ("2 nine channels, pool 8 mean", dict(channels=NINE, pool=8), 1, 2, 9 * 4 * (H // 8) * (W // 8)),
            ("3 nine channels, 128^2 crop, pool 2", dict(channels=NINE, pool=2, crop=(128, 128), centers=centers), 128 * 128 / (H * W), 2,
             9 * 4 * 64 * 64)]


def time_observe(eng, kw):
    spec_out = eng.observe(**kw)
    torch.cuda.synchronize()
    t = []
    for _ in range(15):
        t0 = time.perf_counter()
        eng.observe(out=spec_out, **kw)
        t.append(time.perf_counter() - t0)
    eng.set_async(True)
    eng.sync()
    t0 = time.perf_counter()
    for _ in range(30):
        eng.observe(out=spec_out, **kw)
    eng.sync()
    pipe = (time.perf_counter() - t0) / 30
    eng.set_async(False)
    return statistics.median(t), pipe


def torch_pipeline(eng, name, kw):
    """What a harness does today for the same tensor (float32)."""
    dev = "cuda:0"
    maps = eng.fire_maps_torch()
    ch = kw["channels"]
    planes = []
    attrs = eng.attribute_data_torch() if any(c in BOUNDS for c in ch) else None
    for c in ch:
        if c == "fire_map":
            planes.append(maps.to(torch.float32))
        elif c.startswith("burn_status:"):
            s = ("UNBURNED", "BURNING", "BURNED", "FIRELINE", "SCRATCHLINE", "WETLINE").index(c.split(":")[1])
            planes.append((maps == s).to(torch.float32))
        else:
            lo, hi = BOUNDS[c]
            planes.append(((attrs[c] - lo) / (hi - lo)).to(torch.float32))
    x = torch.stack(planes, 1)
    if "crop" in kw:
        ch_, cw_ = kw["crop"]
        cen = torch.as_tensor(kw["centers"], device=dev)
        xp = torch.nn.functional.pad(x, (cw_ // 2, cw_ - cw_ // 2, ch_ // 2, ch_ - ch_ // 2))
        ys = cen[:, 1, None] + torch.arange(ch_, device=dev)[None, :]
        xs = cen[:, 0, None] + torch.arange(cw_, device=dev)[None, :]
        e = torch.arange(x.shape[0], device=dev)[:, None, None]
        x = xp.permute(0, 2, 3, 1)[e, ys[:, :, None], xs[:, None, :]].permute(0, 3, 1, 2)
    if kw["pool"] > 1:
        x = torch.nn.functional.avg_pool2d(x, kw["pool"])
    torch.cuda.synchronize()
    return x


def time_torch(eng, name, kw):
    torch_pipeline(eng, name, kw)
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        torch_pipeline(eng, name, kw)
        t.append(time.perf_counter() - t0)
    return statistics.median(t)


def main():
    w = c3()
    E, (H, W) = w.n_envs, w.shape
    lines = [f"Observation tensors at C3 ({E} x {H}x{W}) on one MI355X: sf_observe against the torch pipeline it replaces.",
             "sync = one synchronous call (median of 15), pipelined = 30 calls enqueued in async mode / 30; bytes = status read + "
             "attribute planes once + output; % of 6.3 TB/s from the pipelined time.", ""]
    for layout, fused, steps in (("blocked (after a resident run)", 2, 20), ("row-major (after per-step kernels)", 0, 1)):
        eng = FireEngine(**w.engine_kwargs())
        eng.set_layers(*w.layers())
        eng.reset(w.init_xy)
        eng.set_fused(fused)
        eng.step(steps)
        got = eng.cell_layout()
        lines.append(f"layout: {layout}  (cell_layout() = {got}, last launch kind {eng.last_launch_kind()})")
        for name, kw, frac, n_attr, out_bytes in cases(E, H, W):
            s_bytes = E * H * W * frac * (2 if got else 1)
            total = s_bytes + n_attr * 8 * H * W + E * out_bytes
            sync, pipe = time_observe(eng, kw)
            tt = time_torch(eng, name, kw)
            lines.append(f"  case {name:38s} sync {sync * 1e6:9.1f} us  pipelined {pipe * 1e6:9.1f} us  bytes {total / 1e6:8.1f} MB "
                         f"({100 * total / pipe / HBM:5.1f} % of 6.3 TB/s)  | torch pipeline {tt * 1e6:10.1f} us  ({tt / sync:6.1f}x)")
            print(lines[-1], flush=True)
        eng.close()
        lines.append("")
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
