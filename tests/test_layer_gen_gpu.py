"""Seeded worlds drawn on the GPU (``sf_generate_layers``), bit for bit against the host oracles.

- the planes against ``workloads.perlin_elevation`` / ``simplex_field`` / ``config.chaparral_fuel``, read back losslessly through
  ``sf_get_attribute_data``, and the R tables against a handle that was given the oracle planes through ``sf_set_layers_env``;
- environments and planes a call does not name keep their bytes;
- ``BatchedFireSimulation.set_seeds`` + ``reset`` against a batch built from host ``Config`` objects with the same seeds, in the
  per-step and the resident launch structures;
- the behaviour of the seed surface (pending until reset, subsets, invalid keys, shared terrain, ignitions, observe, clone, the
  closed loop, ``FireSimulation``'s wind seeds)."""
import copy
import warnings

import numpy as np
import pytest

from simfire_amd.config import Config, chaparral_fuel
from simfire_amd.engine import FireEngine
from simfire_amd.parameters import fuel_planes
from simfire_amd.simulation import BatchedFireSimulation, FireSimulation
from simfire_amd.units import mph_to_ftpm
from simfire_amd.workloads import perlin_elevation, simplex_field

pytestmark = pytest.mark.gpu

ELEV = dict(octaves=3, persistence=0.7, lacunarity=2.0, range_min=100.0, range_max=2000.0)
SPEED = dict(scale=40, octaves=3, persistence=0.7, lacunarity=2.0, range_min=7, range_max=47)
DIRECTION = dict(scale=150, octaves=2, persistence=0.9, lacunarity=1.0, range_min=0.0, range_max=360.0)


def _dict(H, W, elev_seed=827, fuel_seed=1113, speed_seed=2345, dir_seed=650, max_fire_duration=4):
    return {
        "area": {"screen_size": [H, W], "pixel_scale": 50},
        "display": {"fire_size": 2, "control_line_size": 2, "agent_size": 4},
        "simulation": {"update_rate": 1, "runtime": "24h", "headless": True, "draw_spread_graph": False, "record": False,
                       "save_data": False, "data_type": "npy", "sf_home": "~/.simfire"},
        "mitigation": {"ros_attenuation": True},
        "terrain": {"topography": {"type": "functional", "functional": {"function": "perlin", "perlin": dict(ELEV, seed=elev_seed)}},
                    "fuel": {"type": "functional", "functional": {"function": "chaparral", "chaparral": {"seed": fuel_seed}}}},
        "fire": {"fire_initial_position": {"type": "static", "static": {"position": "(5, 5)"}},
                 "max_fire_duration": max_fire_duration, "diagonal_spread": True},
        "environment": {"moisture": 0.03},
        "wind": {"function": "perlin", "perlin": {"speed": dict(SPEED, seed=speed_seed), "direction": dict(DIRECTION, seed=dir_seed)}},
    }


def _oracle(H, W, elev_seed, fuel_seed, speed_seed, dir_seed):
    """The seven planes the host path builds for these seeds (Config semantics: speed mapped in ft/min, float32, widened)."""
    f = chaparral_fuel(fuel_seed)
    el = perlin_elevation(H, W, ELEV["octaves"], ELEV["persistence"], ELEV["lacunarity"], elev_seed, ELEV["range_min"], ELEV["range_max"])
    sp = simplex_field(H, W, speed_seed, SPEED["scale"], SPEED["octaves"], SPEED["persistence"], SPEED["lacunarity"],
                       mph_to_ftpm(SPEED["range_min"]), mph_to_ftpm(SPEED["range_max"])).astype(np.float64)
    dr = simplex_field(H, W, dir_seed, DIRECTION["scale"], DIRECTION["octaves"], DIRECTION["persistence"], DIRECTION["lacunarity"],
                       DIRECTION["range_min"], DIRECTION["range_max"]).astype(np.float64)
    full = lambda v: np.full((H, W), v)
    return full(f.w_0), full(f.delta), full(f.M_x), full(f.sigma), el, sp, dr


def _specs(elev_seed, fuel_seed, speed_seed, dir_seed):
    f = chaparral_fuel(fuel_seed)
    el = dict(seed=elev_seed, scale=1.0, octaves=ELEV["octaves"], persistence=ELEV["persistence"], lacunarity=ELEV["lacunarity"],
              lo=ELEV["range_min"], hi=ELEV["range_max"])
    sp = dict(seed=speed_seed, scale=SPEED["scale"], octaves=SPEED["octaves"], persistence=SPEED["persistence"],
              lacunarity=SPEED["lacunarity"], lo=mph_to_ftpm(SPEED["range_min"]), hi=mph_to_ftpm(SPEED["range_max"]))
    dr = dict(seed=dir_seed, scale=DIRECTION["scale"], octaves=DIRECTION["octaves"], persistence=DIRECTION["persistence"],
              lacunarity=DIRECTION["lacunarity"], lo=DIRECTION["range_min"], hi=DIRECTION["range_max"])
    return el, (f.w_0, f.delta, f.M_x, f.sigma), sp, dr


def _engine(H, W, E):
    eng = FireEngine((H, W), n_envs=E, pixel_scale=50.0, per_env_terrain=True)
    eng.set_layers(0.5, 2.0, 0.2, 1500.0, 0.0, 400.0, 45.0)          # a flat world in every table
    return eng


def _layers(eng, e):
    a = eng.attribute_data(e)
    return [a[k].copy() for k in ("w_0", "delta", "M_x", "sigma", "elevation", "wind_speed", "wind_direction")]


SEEDS = [(0, 1113, 2345, 650), (-5, 7, -300, 1000), (300, 99, 4242, -1), (827, 123456, 1, 257)]


@pytest.mark.parametrize("H,W,n", [(37, 101, 4), (225, 225, 4), (1024, 1024, 2)])
def test_planes_and_tables_match_the_oracle(H, W, n):
    seeds = SEEDS[:n]
    E = n + 1
    eng = _engine(H, W, E)
    envs = list(range(1, E))[::-1]                                   # out of order: environment 0 stays as it is
    specs = [_specs(*seeds[e - 1]) for e in envs]
    eng.generate_layers(envs, elevation=[s[0] for s in specs], fuel=[s[1] for s in specs], wind_speed=[s[2] for s in specs],
                        wind_direction=[s[3] for s in specs])
    ref = FireEngine((H, W), n_envs=E, pixel_scale=50.0, per_env_terrain=True)
    ref.set_layers(0.5, 2.0, 0.2, 1500.0, 0.0, 400.0, 45.0)
    for e in range(1, E):
        want = _oracle(H, W, *seeds[e - 1])
        got = _layers(eng, e)
        for k in range(4):                                           # the fuel planes come back in get_attribute_data's dtypes
            np.testing.assert_array_equal(got[k], want[k].astype(got[k].dtype))
        for k in range(4, 7):                                        # elevation and wind: lossless f64
            assert got[k].tobytes() == np.ascontiguousarray(want[k]).tobytes(), (e, k)
        ref.set_layers(*want, env=e)
        assert eng.get_rtable(e).tobytes() == ref.get_rtable(e).tobytes(), e
    assert eng.get_rtable(0).tobytes() == ref.get_rtable(0).tobytes()
    assert np.ptp(_layers(eng, 1)[4]) > 100.0 and np.ptp(_layers(eng, 1)[6]) > 1.0      # (fields, not constants)


def test_planes_and_environments_not_named_keep_their_bytes():
    H, W, E = 64, 96, 5
    eng = _engine(H, W, E)
    eng.generate_layers([0, 1, 2, 3, 4], elevation=[_specs(e, 0, 0, 0)[0] for e in range(E)],
                        wind_speed=[_specs(0, 0, 10 + e, 0)[2] for e in range(E)], wind_direction=[_specs(0, 0, 0, 20 + e)[3] for e in range(E)])
    before = [_layers(eng, e) for e in range(E)]
    tabs = [eng.get_rtable(e) for e in range(E)]
    el, fu, sp, dr = _specs(77, 5, 88, 99)
    eng.generate_layers([1], elevation=el)                          # env 1: elevation only
    eng.generate_layers([3], fuel=fu, wind_direction=dr)            # env 3: fuel and direction only
    eng.generate_layers([4], wind_speed=250.0)                      # env 4: a constant speed
    eng.generate_layers([], elevation=el)                           # nothing
    after = [_layers(eng, e) for e in range(E)]
    changed = {1: {4}, 3: {0, 1, 2, 3, 6}, 4: {5}}
    for e in range(E):
        for k in range(7):
            same = before[e][k].tobytes() == after[e][k].tobytes()
            assert same == (k not in changed.get(e, ())), (e, k)
    for e in (0, 2):
        assert eng.get_rtable(e).tobytes() == tabs[e].tobytes()
    for e in (1, 3, 4):
        assert eng.get_rtable(e).tobytes() != tabs[e].tobytes()
    assert (after[4][5] == 250.0).all()
    np.testing.assert_array_equal(after[1][4], perlin_elevation(H, W, 3, 0.7, 2.0, 77, 100.0, 2000.0))


def test_generate_layers_refuses_bad_arguments_before_any_work():
    H, W, E = 32, 40, 3
    eng = _engine(H, W, E)
    before = [_layers(eng, e) for e in range(E)]
    el = _specs(1, 1, 1, 1)[0]
    bad = [dict(envs=[3], elevation=el), dict(envs=[-1], elevation=el), dict(envs=[1, 1], elevation=el),
           dict(envs=[0, 1], elevation=[el, dict(el, scale=0.0)]), dict(envs=[0], elevation=dict(el, octaves=0)),
           dict(envs=[0], elevation=dict(el, octaves=17)), dict(envs=[0], wind_speed=dict(el, lo=5.0, hi=5.0)),
           dict(envs=[0, 1], elevation=[el])]
    for kw in bad:
        envs = kw.pop("envs")
        with pytest.raises(ValueError):
            eng.generate_layers(envs, **kw)
    for e in range(E):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before[e], _layers(eng, e)))
    shared = FireEngine((H, W), n_envs=2, pixel_scale=50.0)
    shared.set_layers(0.5, 2.0, 0.2, 1500.0, 0.0, 400.0, 45.0)
    with pytest.raises(RuntimeError, match="per_env_terrain"):
        shared.generate_layers([0], elevation=el)


def _host_batch(H, W, seeds, fire, **kw):
    cfgs = [Config(config_dict=_dict(H, W, *s), simplex_topography=True) for s in seeds]
    return BatchedFireSimulation(cfgs, len(seeds), seeds=fire, **kw)


def _same_state(a, b):
    sa, ea = a.results()
    sb, eb = b.results()
    np.testing.assert_array_equal(sa, sb)
    assert ea.tobytes() == eb.tobytes()
    assert a._engine.fire_maps().tobytes() == b._engine.fire_maps().tobytes()
    for e in range(a.n_envs):
        assert a._engine.burn(e).tobytes() == b._engine.burn(e).tobytes()


@pytest.mark.parametrize("kind", [0, 2])
def test_set_seeds_reset_equals_host_configs(kind):
    H, W, E = 128, 144, 6
    seeds = [(11 * e - 20, 1113 + e, 300 + 7 * e, 650 - 3 * e) for e in range(E)]
    fire = [4000 + e for e in range(E)]
    sim = BatchedFireSimulation(Config(config_dict=_dict(H, W), simplex_topography=True), E, per_env_terrain=True)
    assert set(sim.get_seeds()) == {"elevation", "fuel", "wind_speed", "wind_direction", "fire_initial_position"}
    assert sim.set_seeds({"elevation": [s[0] for s in seeds], "fuel": [s[1] for s in seeds], "wind_speed": [s[2] for s in seeds],
                          "wind_direction": [s[3] for s in seeds], "fire_initial_position": fire}) is True
    sim.reset()
    host = _host_batch(H, W, seeds, fire)
    np.testing.assert_array_equal(sim.ignitions, host.ignitions)
    for e in range(E):
        assert sim._engine.get_rtable(e).tobytes() == host._engine.get_rtable(e).tobytes()
    for s in (sim, host):
        s._engine.set_fused(kind)
    rng = np.random.default_rng(kind)
    for it in range(4):
        if it == 2:
            pts = rng.integers(0, [W, H, 3], size=(8, E, 4, 3)).astype(np.int32)
            pts[..., 2] += 3
            ma, aa = sim.rollout(pts, return_maps=True)
            mb, ab = host.rollout(pts, return_maps=True)
        else:
            ma, aa = sim.run(12)
            mb, ab = host.run(12)
            assert sim._engine.last_launch_kind() == kind and host._engine.last_launch_kind() == kind
        assert ma.tobytes() == mb.tobytes()
        np.testing.assert_array_equal(aa, ab)
        _same_state(sim, host)
    assert sim.results()[0][:, 1].min() > 0


def test_seed_surface_behaviour():
    H, W, E = 64, 80, 4
    d = _dict(H, W)
    sim = BatchedFireSimulation(Config(config_dict=d, simplex_topography=True), E, per_env_terrain=True)
    base = [_layers(sim._engine, e) for e in range(E)]
    got = sim.get_seeds()
    assert got["elevation"].dtype == np.int64 and (got["elevation"] == 827).all() and (got["fuel"] == 1113).all()
    np.testing.assert_array_equal(got["fire_initial_position"], 1234 + np.arange(E))
    np.testing.assert_array_equal(sim.get_seeds([2])["wind_speed"], [2345])
    # nothing changes before reset; then only the subset that is reset
    assert sim.set_seeds({"elevation": 5, "wind_direction": [8, 9]}, envs=[1, 3])
    np.testing.assert_array_equal(sim.get_seeds()["elevation"], [827, 5, 827, 5])
    for e in range(E):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(base[e], _layers(sim._engine, e)))
    sim.reset([3])
    now = [_layers(sim._engine, e) for e in range(E)]
    for e in (0, 1, 2):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(base[e], now[e]))
    np.testing.assert_array_equal(now[3][4], _oracle(H, W, 5, 1113, 2345, 9)[4])
    np.testing.assert_array_equal(now[3][6], _oracle(H, W, 5, 1113, 2345, 9)[6])
    np.testing.assert_array_equal(now[3][5], base[3][5])
    sim.reset()
    np.testing.assert_array_equal(_layers(sim._engine, 1)[6], _oracle(H, W, 5, 1113, 2345, 8)[6])
    # invalid keys warn and make the result False; the valid ones are applied
    with pytest.warns(UserWarning, match="Valid keys"):
        assert sim.set_seeds({"fuel": 3, "humidity": 1}) is False
    np.testing.assert_array_equal(sim.get_seeds()["fuel"], [3] * E)
    with pytest.raises(ValueError, match="values"):
        sim.set_seeds({"fuel": [1, 2]})
    # fire_initial_position: default_rng(seed), as the constructor draws it
    sim.set_seeds({"fire_initial_position": [7, 8]}, envs=[0, 2])
    for e, sd in ((0, 7), (2, 8)):
        rng = np.random.default_rng(sd)
        assert tuple(sim.ignitions[e]) == (rng.integers(W, dtype=int), rng.integers(H, dtype=int))
    sim.reset([0, 2])
    m = sim._engine.fire_maps()
    for e in (0, 2):
        x, y = sim.ignitions[e]
        assert m[e, y, x] == 1 and (m[e] == 1).sum() == 1
    # observe() shows the new planes
    torch = pytest.importorskip("torch")
    sim.set_seeds({"elevation": 41, "wind_speed": -12}, envs=[2])
    sim.reset([2])
    obs = sim.observe(["elevation", "wind_speed"], envs=[2], normalize=False).cpu().numpy()
    want = _oracle(H, W, 41, 3, -12, 650)
    np.testing.assert_array_equal(obs[0, 0], want[4].astype(np.float32))
    np.testing.assert_array_equal(obs[0, 1], want[5].astype(np.float32))
    del torch
    # a shared-terrain batch refuses layer seeds, takes ignition seeds
    shared = BatchedFireSimulation(Config(config_dict=d, simplex_topography=True), 2)
    with pytest.raises(ValueError, match="per_env_terrain"):
        shared.set_seeds({"elevation": 1})
    assert shared.set_seeds({"fire_initial_position": 5})
    # explicit ignitions: no fire seed
    fixed = BatchedFireSimulation(Config(config_dict=d, simplex_topography=True), 2, ignitions=[[1, 1], [2, 2]], per_env_terrain=True)
    assert "fire_initial_position" not in fixed.get_seeds()


def test_configs_are_dropped_and_clone_carries_layers_and_seeds():
    H, W, E = 48, 64, 4
    seeds = [(e, 1113, 2345, 650) for e in range(E)]
    sim = _host_batch(H, W, seeds, [10, 11, 12, 13])
    np.testing.assert_array_equal(sim.get_seeds()["elevation"], [0, 1, 2, 3])
    sim.set_seeds({"elevation": 99, "fuel": 5}, envs=[1])
    assert sim.configs[1] is not None                                 # pending: still the old world
    sim.reset([1])
    assert sim.configs[1] is None and sim.terrains[1] is None and sim.configs[0] is not None
    np.testing.assert_array_equal(_layers(sim._engine, 1)[4], _oracle(H, W, 99, 5, 2345, 650)[4])
    sim.run(5)
    sim.clone_envs([1], [3], terrain=True)
    for a, b in zip(_layers(sim._engine, 1), _layers(sim._engine, 3)):
        assert a.tobytes() == b.tobytes()
    assert sim._engine.get_rtable(1).tobytes() == sim._engine.get_rtable(3).tobytes()
    got = sim.get_seeds()
    assert got["elevation"][3] == 99 and got["fuel"][3] == 5 and got["fire_initial_position"][3] == 11
    assert sim.configs[3] is None
    # a seed still pending on src goes with it: both draw the same world at their next reset
    sim.set_seeds({"wind_speed": 31}, envs=[0])
    sim.clone_envs([0], [2], terrain=True)
    sim.reset([0, 2])
    for a, b in zip(_layers(sim._engine, 0), _layers(sim._engine, 2)):
        assert a.tobytes() == b.tobytes()
    np.testing.assert_array_equal(_layers(sim._engine, 2)[5], _oracle(H, W, 0, 1113, 31, 650)[5])


def test_regenerating_during_the_closed_loop():
    H, W, E = 64, 64, 3
    cfg = Config(config_dict=_dict(H, W), simplex_topography=True)
    a = BatchedFireSimulation(cfg, E, per_env_terrain=True)
    b = BatchedFireSimulation(copy.deepcopy(cfg), E, per_env_terrain=True)
    a.loop_start(1)
    for _ in range(4):
        a.loop_step(None)
        b.run(1)
    for s in (a, b):
        s.set_seeds({"elevation": 17, "wind_direction": 3}, envs=[1])
        s.reset([1])
    a.loop_start(1)
    for _ in range(6):
        ra, ea = a.loop_step(None)
        b.run(1)
        rb, eb = b.results()
        np.testing.assert_array_equal(ra, rb)
        assert ea.tobytes() == eb.tobytes()
    a.loop_stop()
    _same_state(a, b)
    np.testing.assert_array_equal(_layers(a._engine, 1)[4], _oracle(H, W, 17, 1113, 2345, 3)[4])


def test_fire_simulation_wind_seeds_round_trip():
    H, W = 48, 56
    d = _dict(H, W)
    d["terrain"]["topography"]["functional"]["function"] = "flat"
    sim = FireSimulation(Config(config_dict=d))
    assert sim.get_seeds() == {"fuel": 1113, "wind_speed": 2345, "wind_direction": 650}
    assert sim.set_seeds({"wind_speed": 9, "wind_direction": -4}) is True
    assert sim.get_seeds() == {"fuel": 1113, "wind_speed": 9, "wind_direction": -4}
    sim.reset()
    want = _oracle(H, W, 0, 1113, 9, -4)
    a = sim._engine.attribute_data(0)
    assert a["wind_speed"].tobytes() == want[5].tobytes() and a["wind_direction"].tobytes() == want[6].tobytes()
    assert sim.set_seeds({"wind_speed": 2345}) is True and sim.get_seeds()["wind_speed"] == 2345
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        d2 = _dict(H, W)
        d2["terrain"]["topography"]["functional"]["function"] = "flat"
        d2["wind"] = {"function": "simple", "simple": {"speed": 7, "direction": 90.0}}
        assert FireSimulation(Config(config_dict=d2)).get_seeds() == {"fuel": 1113}
