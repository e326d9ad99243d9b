"""CFD wind on the GPU (sf_cfd_*, simfire_amd/wind.py, `wind.function: cfd` in Config): Vx / Vy bit for bit against the numpy
restatement tests/_cfd_oracle.py (itself bit-exact against the reference's own fixtures, tests/test_cfd_cpu.py)."""
import copy
import glob
import os

import numpy as np
import pytest
import yaml

import _cfd_oracle as cfd

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CFG = os.path.join(GOLD, "configs")
FIXTURES = sorted(glob.glob(os.path.join(GOLD, "cfd_*.npz")))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return a.shape == b.shape and (bits(a) == bits(b)).all()


def solver(n, n_envs=1, itr=1, dt=1.0, visc=1e-7, speed=19.0, direction="north"):
    from simfire_amd.wind import _Solver, direction_code
    return _Solver(n, n_envs, itr, dt, visc, speed, direction_code(direction))


def masks(n, seed):
    """no terrain, random 30 %, blobs touching rows and columns 1, 2, N-3, N-2"""
    rng = np.random.default_rng(seed)
    blobs = np.zeros((n, n), np.uint8)
    for r, c in ((1, n // 3), (n - 3, n // 2), (n // 3, 1), (n // 2, n - 3), (n // 2, n // 2)):
        blobs[r:r + 2, c:c + 2] = 1
    return [np.zeros((n, n), np.uint8), (rng.random((n, n)) < 0.3).astype(np.uint8), blobs]


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(f)[4:-4] for f in FIXTURES])
def test_golden_fixtures(path):
    z = np.load(path)
    n = int(z["n"])
    s = solver(n, 1, int(z["result_accuracy"]), float(z["timestep_dt"]), float(z["viscosity"]), float(z["speed"]),
               str(z["direction"]))
    s.set_terrain(0, z["mask"].astype(np.uint8))
    for it in range(int(z["iterations"])):
        s.step(2, 2)
        vx, vy = s.velocity(0)
        assert same(vx, z["planes"][it, 0]) and same(vy, z["planes"][it, 1]), f"iteration {it}"


@pytest.mark.parametrize("n", [64, 225])
@pytest.mark.parametrize("direction", ["north", "east", "south", "west"])
@pytest.mark.parametrize("itr", [1, 4])
def test_against_oracle(n, direction, itr):
    ms = masks(n, n + itr)
    s = solver(n, len(ms), itr, direction=direction, speed=5.3)
    for e, m in enumerate(ms):
        s.set_terrain(e, m)
    s.step(24, 2)
    for e, m in enumerate(ms):
        f = cfd.Fluid(n, itr, 1.0, 1e-7, m)
        f.train(12, direction, 5.3)
        vx, vy = s.velocity(e)
        assert same(vx, f.Vx) and same(vy, f.Vy), f"mask {e}"


def test_row_strips_n1030():
    """More interior rows than lanes of a workgroup: the Gauss-Seidel pass runs in strips of 1024 rows."""
    n = 1030
    m = masks(n, 7)[1]
    s = solver(n, 1, 2, direction="west", speed=5.3)
    s.set_terrain(0, m)
    s.step(4, 2)
    f = cfd.Fluid(n, 2, 1.0, 1e-7, m)
    f.train(2, "west", 5.3)
    vx, vy = s.velocity(0)
    assert same(vx, f.Vx) and same(vy, f.Vy)


def test_batch_equals_single_environments():
    n, itr = 48, 2
    rng = np.random.default_rng(3)
    ms = [(rng.random((n, n)) < p).astype(np.uint8) for p in (0.0, 0.1, 0.2, 0.3, 0.4, 0.5)]
    b = solver(n, 6, itr, direction="south", speed=7.0)
    for e, m in enumerate(ms):
        b.set_terrain(e, m)
    b.step(10, 2)
    for e, m in enumerate(ms):
        one = solver(n, 1, itr, direction="south", speed=7.0)
        one.set_terrain(-1, m)
        one.step(10, 2)
        vb, vo = b.velocity(e), one.velocity(0)
        assert same(vb[0], vo[0]) and same(vb[1], vo[1]), e
        f = cfd.Fluid(n, itr, 1.0, 1e-7, m)
        f.train(5, "south", 7.0)
        assert same(vb[0], f.Vx) and same(vb[1], f.Vy), e


def test_split_calls_equal_one_call():
    n, T = 40, 6
    m = masks(n, 11)[2]
    one = solver(n, 1, 3, direction="north")
    one.set_terrain(0, m)
    one.step(2 * T, 2)
    split = solver(n, 1, 3, direction="north")
    split.set_terrain(0, m)
    for k in (2, 4, 6):
        split.step(k, 2)
    assert all(same(a, b) for a, b in zip(one.velocity(0), split.velocity(0)))


def test_controller_sequence_equals_training_call():
    from simfire_amd.wind import WindControllerCFD, generate_cfd_wind_layer
    n, T = 33, 4
    el = np.random.default_rng(5).random((n, n, 1)) * 100
    wc = WindControllerCFD(screen_size=(n, n), result_accuracy=2, timestep=1.0, viscosity=1e-7, terrain_features=el,
                           wind_speed=5.3, wind_direction="West")
    assert wc.get_screen_size() == (n, n) and wc.get_wind_scale() == 1 and not wc.get_wind_density_field().any()
    for _ in range(T):
        wc.iterate_wind_step()
        wc.step()
    s = solver(n, 1, 2, direction="west", speed=5.3)
    s.set_terrain(0, cfd.terrain_mask(el))
    s.step(2 * T, 2)
    vx, vy = s.velocity(0)
    assert same(wc.get_wind_velocity_field_x(), vx) and same(wc.get_wind_velocity_field_y(), vy)
    f = cfd.Fluid(n, 2, 1.0, 1e-7, cfd.terrain_mask(el))
    f.train(T, "west", 5.3)
    assert same(vx, f.Vx) and same(vy, f.Vy)
    wc2 = WindControllerCFD(screen_size=(n, n), result_accuracy=2, timestep=1.0, viscosity=1e-7, terrain_features=el,
                            wind_speed=5.3, wind_direction="west")
    mag, dr = generate_cfd_wind_layer(T, wc2)
    sp, dr2 = cfd.wind_fields(el, result_accuracy=2, timestep_dt=1.0, viscosity=1e-7, speed=5.3, direction="west",
                              train_steps=T)
    assert same(mag * 196.85, sp) and np.abs(dr - dr2).max() <= 1e-9


def test_cfd_wind_fields_batched():
    from simfire_amd.wind import cfd_wind_fields
    n = 30
    rng = np.random.default_rng(9)
    el = rng.random((3, n, n))
    kw = dict(result_accuracy=1, timestep_dt=1.0, viscosity=1e-7, speed=19, direction="north", train_steps=3)
    sp, dr = cfd_wind_fields(el, **kw)
    assert sp.shape == dr.shape == (3, n, n) and sp.dtype == dr.dtype == np.float64
    for e in range(3):
        so, do = cfd.wind_fields(el[e], **kw)
        assert same(sp[e], so) and np.abs(dr[e] - do).max() <= 1e-9
        s1, d1 = cfd_wind_fields(el[e][..., None], **kw)
        assert same(s1, sp[e]) and same(d1, dr[e])


CFD_KEYS = dict(result_accuracy=2, timestep_dt=1.0, viscosity=0.0000001, speed=19, direction="north", train_steps=3)


def _cfd_dict(name, size=None):
    d = yaml.safe_load(open(os.path.join(CFG, name)))
    d["terrain"]["topography"]["functional"]["function"] = "flat"
    if size:
        d["area"]["screen_size"] = [size, size]
    d["wind"]["function"] = "cfd"
    d["wind"]["cfd"] = dict(d["wind"].get("cfd") or {}, **CFD_KEYS)
    return d


@pytest.mark.parametrize("name,size", [("test_config_flat_simple.yml", None), ("functional_config.yml", None)])
def test_config_cfd_wind(name, size):
    from simfire_amd.config import Config
    c = Config(config_dict=_cfd_dict(name, size))
    H, W = c.area.screen_size
    sp, dr = cfd.wind_fields(np.zeros((H, W)), **CFD_KEYS)
    assert same(c.wind.speed, sp) and np.abs(c.wind.direction - dr).max() <= 1e-9
    assert c.wind.speed_function.name == c.wind.direction_function.name == "cfd"
    assert c.wind.speed_function.kwargs["train_steps"] == 3
    before = c.wind.speed.copy(), c.wind.direction.copy()
    c.reset_wind()
    assert same(c.wind.speed, before[0]) and same(c.wind.direction, before[1])


def test_fire_simulation_with_cfd_wind():
    from simfire_amd.config import Config
    from simfire_amd.simulation import FireSimulation
    d = _cfd_dict("functional_config.yml", 48)
    d["wind"]["cfd"]["speed"] = 5.3
    d["wind"]["cfd"]["direction"] = "west"
    c = Config(config_dict=d)
    kw = dict(CFD_KEYS, speed=5.3, direction="west")
    sp, dr = cfd.wind_fields(np.zeros((48, 48)), **kw)
    assert np.abs(sp).max() > 0
    ref = Config.from_arrays(copy.deepcopy(d), c.terrain.fuel_layer.data[..., 0], np.zeros((48, 48)), sp, dr)
    a, b = FireSimulation(c), FireSimulation(ref)
    a.run(40)
    b.run(40)
    assert (a.fire_map == b.fire_map).all() and (a.fire_map > 0).sum() > 1


def test_cfd_precompute_setup():
    from simfire_amd.config import Config
    from simfire_amd.wind import WindControllerCFD, cfd_wind_fields, generate_cfd_wind_layer
    d = _cfd_dict("test_config_flat_simple.yml")
    c = Config(config_dict=d, cfd_precompute=True)
    assert not hasattr(c, "wind") and isinstance(c.cfd_setup, WindControllerCFD)
    assert c.cfd_setup.get_wind_scale() == d["area"]["pixel_scale"]
    mag, dr = generate_cfd_wind_layer(CFD_KEYS["train_steps"], c.cfd_setup)
    sp, dr2 = cfd_wind_fields(c.terrain.topography_layer.data, **CFD_KEYS)
    assert same(mag * 196.85, sp) and same(dr, dr2)
