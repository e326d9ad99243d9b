"""Probe: what drawing a new episode's parameters on the device costs (sf_episodes_*, simfire_amd/csrc/sf_episode_kernels.h).

C5's shape with a terrain per environment (64 x 1024^2, 64 agents per environment, attenuation on), asynchronous mode, one ``sync``
per 100 ticks, random action tensors drawn on the device ahead of the timed window.  A tick is ``FireEngine.agents_step`` with all
five outputs:

  (a)  the parent commit's library (``--parent-lib PATH``: a build of the commit before this feature; measured in a child
       process, which loads that library through SIMFIRE_HIP_LIB), randomisation does not exist: max_ticks = 0
  (b)  this library, randomisation off, the same tick as (a)                       <- the only bar: (b) against (a) overlap
  (b') this library, randomisation off, max_ticks = 64 with the environments' episodes staggered by one tick, so that one
       environment restarts per tick: what the restart itself costs (the batched reset of a 1024^2 environment)
  (c)  as (b') with the ignition (live cells) and the agents' start cells drawn
  (d)  as (b') with the ignition and a uniform wind drawn: one 1024^2 table rebuilt per tick
  (e)  the host assembly (d) replaces: auto_reset off, ``done`` read back every tick, then ``reset_envs``, ``set_wind`` and
       ``agents_place`` from the host for the environments that are done (their parameters from a NumPy generator)

Wall time per tick: host clock around 100 ticks and the sync, divided by 100; median [min, max] of 7 windows after one warm-up
window (in which the staggering is set up).  Nothing but (b) against (a) is gated on these numbers.

  python profiles/episode_draw_probe.py --parent-lib PATH     # -> profiles/episode_draw_timing.txt
  python profiles/episode_draw_probe.py --quick                # 8 x 256^2, 8 agents, no row (a), nothing written"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from simfire_amd import workloads  # noqa: E402
from simfire_amd.engine import FireEngine  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "episode_draw_timing.txt")
REPS, TICKS = 7, 100
WEIGHTS = (-1.0, 0.1, -5.0, -0.1)
U_RANGE, D_RANGE = (440.0, 1760.0), (0.0, 360.0)          # 5 .. 20 mph


def engine(w):
    eng = FireEngine(per_env_terrain=True, **w.engine_kwargs())
    eng.set_layers(*w.layers())                            # (replicated into every environment's table)
    eng.reset(w.init_xy)
    eng.set_async(True)
    return eng


def starts(E, K, H, W):
    rng = np.random.default_rng(9000)
    return np.stack([rng.integers(W, size=(E, K)), rng.integers(H, size=(E, K))], axis=2).astype(np.int32)


def windows(tick, eng, warm=None):
    out = []
    for rep in range(REPS + 1):
        t0 = time.perf_counter()
        for t in range(TICKS):
            if rep == 0 and warm is not None:
                warm(t)
            tick(rep * TICKS + t)
        eng.sync()
        out.append((time.perf_counter() - t0) * 1e6 / TICKS)
    return out[1:]


def row(size, E, K, which):
    """The windows of one row; ``which``: "off0" (rows a, b), "off", "ign_agents", "ign_wind", "host"."""
    import torch
    w = workloads.c5(size, E, K)
    H = W = size
    dev = "cuda:0"
    xy0 = starts(E, K, H, W)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    acts = [torch.randint(0, 20, (E, K), dtype=torch.int32, device=dev, generator=gen) for _ in range(TICKS)]
    eng = engine(w)
    period = 0 if which == "off0" else E                  # one restart per tick once the episodes are staggered
    eng.agents_create(K, w.init_xy, n_updates=1, weights=WEIGHTS, only_unburned=True, max_ticks=period, auto_reset=which != "host")
    eng.agents_place(np.arange(E), xy0)
    box = (size // 8, size // 8, size - size // 8 - 1, size - size // 8 - 1)
    if which == "ign_agents":
        eng.episodes_set(11, ignition_box=box, live_cells=True, agent_box=(0, 0, W - 1, H - 1))
    elif which == "ign_wind":
        eng.episodes_set(11, ignition_box=box, live_cells=True, wind_speed=U_RANGE, wind_direction=D_RANGE)
    o = dict(reward=torch.empty(E, dtype=torch.float32, device=dev), done=torch.empty(E, dtype=torch.uint8, device=dev),
             terms=torch.empty((E, 4), dtype=torch.int32, device=dev), final_len=torch.empty(E, dtype=torch.int32, device=dev),
             final_ret=torch.empty(E, dtype=torch.float64, device=dev))

    def stagger(t):                                        # warm-up window: environment t's episode statistics start at tick t
        if period and t < E:
            eng.agents_place([t], xy0[t:t + 1])
    rng = np.random.default_rng(12)

    def host_tick(t):
        eng.agents_step(acts[t % TICKS], **o)
        eng.sync()
        envs = np.flatnonzero(o["done"].cpu().numpy())
        if len(envs):
            n = len(envs)
            xy = np.stack([rng.integers(box[0], box[2] + 1, size=n), rng.integers(box[1], box[3] + 1, size=n)], axis=1).astype(np.int32)
            eng.reset_envs(envs, xy)
            eng.set_wind(rng.uniform(*U_RANGE, size=n), rng.uniform(*D_RANGE, size=n), envs=envs)
            eng.agents_place(envs, xy0[envs])
    out = windows(host_tick if which == "host" else (lambda t: eng.agents_step(acts[t % TICKS], **o)), eng, stagger)
    restarts = None
    if which in ("ign_agents", "ign_wind"):
        restarts = int(eng.episodes_torch()["index"].sum().item())
    eng.close()
    return out, restarts


def med(v):
    return "%8.1f us  [%.1f, %.1f]" % (statistics.median(v), min(v), max(v))


def main():
    quick = "--quick" in sys.argv
    size, E, K = (256, 8, 8) if quick else (1024, 64, 64)
    if "--row-a" in sys.argv:                              # the child of row (a): this process loads the parent's library,
        from simfire_amd import _lib                       # which has none of the entries this feature adds
        for name in [n for n in _lib.SIGNATURES if n.startswith("sf_episodes_")]:
            del _lib.SIGNATURES[name]
        print("ROW_A " + json.dumps(row(size, E, K, "off0")[0]))
        return
    parent = sys.argv[sys.argv.index("--parent-lib") + 1] if "--parent-lib" in sys.argv else None
    a = None
    if parent:
        env = dict(os.environ, SIMFIRE_HIP_LIB=os.path.abspath(parent))
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--row-a"] + (["--quick"] if quick else []), env=env,
                             capture_output=True, text=True, check=True)
        a = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("ROW_A ")][-1][6:])
    b, _ = row(size, E, K, "off0")
    b2, _ = row(size, E, K, "off")
    c, nc = row(size, E, K, "ign_agents")
    d, nd = row(size, E, K, "ign_wind")
    e, _ = row(size, E, K, "host")
    per = (REPS + 1) * TICKS
    overlap = None if a is None else (min(a) <= max(b) and min(b) <= max(a))
    text = (f"New episodes drawn on the device, one MI355X: {E} x {size}^2 with a terrain per environment, {K} agents per environment"
            f"{'' if quick else ' (C5 shape)'},\nasynchronous mode, one sync per {TICKS} ticks.  Wall time per agents_step tick, median [min, max] of {REPS} windows of "
            f"{TICKS} ticks\nafter one warm-up window.\n\n"
            f"  (a)  the parent commit's library, max_ticks = 0                        {med(a) if a else '   (not measured: no --parent-lib)'}\n"
            f"  (b)  this library, randomisation off, max_ticks = 0                    {med(b)}\n"
            f"  (b') randomisation off, max_ticks = {E}: one restart per tick            {med(b2)}\n"
            f"  (c)  (b') + ignition (live cells) and agent start cells drawn          {med(c)}   ({nc / per:.2f} restarts per tick)\n"
            f"  (d)  (b') + ignition and wind drawn: one table rebuilt per tick        {med(d)}   ({nd / per:.2f} restarts per tick)\n"
            f"  (e)  host assembly of (d): done read back, reset_envs + set_wind\n"
            f"       + agents_place from the host                                      {med(e)}\n\n"
            + ("" if a is None else f"  (b) against (a): the windows {'overlap' if overlap else 'DO NOT overlap'} - randomisation off "
                                    f"{'costs nothing' if overlap else 'is not free'}.\n")
            + f"  (c) - (b') = {statistics.median(c) - statistics.median(b2):.1f} us: the draw kernel (expected: launch-bound, a few us).\n"
              f"  (d) - (b') = {statistics.median(d) - statistics.median(b2):.1f} us: the draw, the memset of the due count and one table rebuilt from the cache\n"
              f"  (expected: ~200 MB moved per restart, tens of us at HBM rates).\n"
              f"  (e) / (d) = {statistics.median(e) / statistics.median(d):.2f}\n")
    print(text)
    if not quick:
        with open(OUT, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
