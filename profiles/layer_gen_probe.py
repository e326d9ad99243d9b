"""Probe: seeded worlds drawn on the GPU (sf_generate_layers, simfire_amd/csrc/sf_gen_kernels.h) - milliseconds per
``BatchedFireSimulation.set_seeds`` + ``reset`` that redraws every seeded layer (perlin elevation, chaparral fuel, perlin wind speed and
direction) of every environment, host clock around the calls with the handle's stream synchronised, median [min, max] of 7 runs after a
warm-up run.  The ``sf_generate_layers`` call alone is timed the same way (it returns after its work is done).

The host path for the same worlds - a ``Config`` per environment (NumPy generators) and ``sf_set_layers_env`` - is timed on one
environment (median of 3, other seeds each time: ``simplex_field`` caches) and multiplied by the number of environments.

  python profiles/layer_gen_probe.py            # every shape -> profiles/layer_gen_timing.txt
  python profiles/layer_gen_probe.py --quick    # one small shape, nothing written"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from simfire_amd.config import Config  # noqa: E402
from simfire_amd.simulation import BatchedFireSimulation, _config_layers, _set_config_layers  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "layer_gen_timing.txt")
SHAPES = [(1024, 256), (2048, 64), (225, 1)]


def config_dict(n, elev_seed=827, fuel_seed=1113, speed_seed=2345, dir_seed=650):
    """configs/functional_config.yml's terrain (perlin topography, chaparral fuel) with configs/operational_config.yml's perlin wind."""
    return {
        "area": {"screen_size": [n, n], "pixel_scale": 50},
        "display": {"fire_size": 2, "control_line_size": 2, "agent_size": 4},
        "simulation": {"update_rate": 1, "runtime": "24h", "headless": True, "draw_spread_graph": False, "record": False,
                       "save_data": False, "data_type": "npy", "sf_home": "~/.simfire"},
        "mitigation": {"ros_attenuation": True},
        "terrain": {"topography": {"type": "functional", "functional": {"function": "perlin", "perlin": {
                        "octaves": 3, "persistence": 0.7, "lacunarity": 2.0, "seed": elev_seed, "range_min": 100.0, "range_max": 300.0}}},
                    "fuel": {"type": "functional", "functional": {"function": "chaparral", "chaparral": {"seed": fuel_seed}}}},
        "fire": {"fire_initial_position": {"type": "static", "static": {"position": "(16, 16)"}}, "max_fire_duration": 4,
                 "diagonal_spread": True},
        "environment": {"moisture": 0.03},
        "wind": {"function": "perlin", "perlin": {
            "speed": {"seed": speed_seed, "scale": 400, "octaves": 3, "persistence": 0.7, "lacunarity": 2.0, "range_min": 7, "range_max": 47},
            "direction": {"seed": dir_seed, "scale": 1500, "octaves": 2, "persistence": 0.9, "lacunarity": 1.0, "range_min": 0.0,
                          "range_max": 360.0}}},
    }


def probe(n, envs):
    sim = BatchedFireSimulation(Config(config_dict=config_dict(n), simplex_topography=True), envs, per_env_terrain=True)
    eng = sim._engine
    base = np.arange(envs, dtype=np.int64)

    def redraw(k):
        sim.set_seeds({"elevation": base + 1000 * k, "fuel": base + 7 * k, "wind_speed": base - 3 * k, "wind_direction": base + 11 * k})
        t0 = time.perf_counter()
        sim.reset()
        eng.sync()
        return (time.perf_counter() - t0) * 1e3

    redraw(1)
    full = [redraw(k) for k in range(2, 9)]
    sim.set_seeds({"elevation": base + 5, "fuel": base, "wind_speed": base, "wind_direction": base})
    pend = sorted(sim._pending)
    gen = []
    for _ in range(8):
        for e in pend:
            sim._pending[e] = {"elevation", "fuel", "wind_speed", "wind_direction"}
        t0 = time.perf_counter()
        sim._regenerate(pend)
        gen.append((time.perf_counter() - t0) * 1e3)
    gen = gen[1:]
    host = []
    for k in range(3):
        t0 = time.perf_counter()
        c = Config(config_dict=config_dict(n, 5000 + k, 5000 + k, 5000 + k, 5000 + k), simplex_topography=True)
        fuels, elev = _config_layers(c)
        _set_config_layers(eng, c, fuels, elev, 0 if envs > 1 else None)     # (a one-environment handle addresses its table as "all")
        host.append((time.perf_counter() - t0) * 1e3)
    mem = eng.memory_bytes()
    sim._engine.close()
    return full, gen, host, mem


def fmt(ts):
    return f"{statistics.median(ts):10.3f} ms  [{min(ts):.3f}, {max(ts):.3f}]"


def main():
    quick = "--quick" in sys.argv
    lines = ["Seeded worlds on one MI355X: every seeded layer (perlin elevation 3 octaves, chaparral fuel, perlin wind speed 3 octaves and",
             "direction 2 octaves) of every environment redrawn.  set_seeds + reset: host clock around reset() + sync (the regeneration is",
             "one sf_generate_layers call, then sf_reset); sf_generate_layers alone: host clock around the call.  Median [min, max] of 7 runs",
             "after a warm-up.  Host path: Config (NumPy generators) + sf_set_layers_env for ONE environment, median of 3, times E.", ""]
    for n, envs in ([(225, 4)] if quick else SHAPES):
        full, gen, host, mem = probe(n, envs)
        h = statistics.median(host)
        lines.append(f"{n:5d}^2 x {envs:3d} envs  (handle {mem / 2**30:6.2f} GiB)")
        lines.append(f"    set_seeds + reset       {fmt(full)}")
        lines.append(f"    sf_generate_layers      {fmt(gen)}")
        lines.append(f"    host path, 1 env        {fmt(host)}   -> x {envs} = {h * envs / 1e3:9.2f} s "
                     f"({h * envs / statistics.median(full):,.0f}x the GPU path)")
        print("\n".join(lines[-4:]), flush=True)
    if not quick:
        with open(OUT, "w") as f:
            f.write("\n".join(lines) + "\n")
        print("wrote", OUT)


if __name__ == "__main__":
    main()
