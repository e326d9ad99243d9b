"""CFD wind (`wind.function: cfd`) without a GPU: the numpy restatement (tests/_cfd_oracle.py) against fixtures made by the
reference itself (tests/golden/make_golden_cfd.py), and the Config checks that run before any device call."""
import copy
import glob
import os

import numpy as np
import pytest
import yaml

import _cfd_oracle as cfd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CFG = os.path.join(GOLD, "configs")
FIXTURES = sorted(glob.glob(os.path.join(GOLD, "cfd_*.npz")))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_fixture_set_covers_the_issue_cases():
    assert len(FIXTURES) >= 12
    seen = [np.load(f) for f in FIXTURES]
    assert {int(z["n"]) for z in seen} >= {9, 10, 17, 24, 32}
    assert {str(z["direction"]).lower() for z in seen} == set(cfd.DIRECTIONS)
    assert {int(z["result_accuracy"]) for z in seen} == {1, 2, 3}
    assert any(z["mask"].any() for z in seen) and any(not z["mask"].any() for z in seen)


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(f)[4:-4] for f in FIXTURES])
def test_oracle_equals_reference_bit_for_bit(path):
    z = np.load(path)
    n = int(z["n"])
    el = z["elevation"] if bool(z["has_elevation"]) else None
    mask = np.zeros((n, n), np.uint8) if el is None else cfd.terrain_mask(el)
    assert (mask == z["mask"]).all()
    f = cfd.Fluid(n, int(z["result_accuracy"]), float(z["timestep_dt"]), float(z["viscosity"]), mask)
    for it in range(int(z["iterations"])):
        f.iterate_wind_step(str(z["direction"]), float(z["speed"]))
        f.step()
        for k, plane in enumerate((f.Vx, f.Vy, f.Vx0, f.Vy0)):
            assert (bits(plane) == bits(z["planes"][it, k])).all(), f"iteration {it} plane {('Vx', 'Vy', 'Vx0', 'Vy0')[k]}"
    # the wind module's host-side formulas (speed bit for bit, direction within 1e-9 degrees)
    from simfire_amd import wind
    assert (bits(wind.magnitude(f.Vx, f.Vy)) == bits(z["magnitude"])).all()
    assert np.abs(wind.direction_deg(f.Vx, f.Vy) - z["direction_deg"]).max() <= 1e-9
    assert (wind.terrain_mask(el if el is not None else np.zeros((n, n))) == mask).all()


def test_east_wind_trains_to_zero():
    """The east inflow writes a boundary cell that diffuse overwrites before it is read (wind_controller.py:162)."""
    vx, vy = cfd.velocity(np.zeros((12, 12)), result_accuracy=2, timestep_dt=1.0, viscosity=1e-7, speed=19.0, direction="east",
                          train_steps=3)
    assert not vx.any() and not vy.any()


def _cfd_config(name="test_config_flat_simple.yml", **cfd_keys):
    d = yaml.safe_load(open(os.path.join(CFG, name)))
    d["wind"]["function"] = "cfd"
    d["wind"]["cfd"] = dict(d["wind"].get("cfd") or {}, **cfd_keys)
    return d


def test_config_cfd_missing_train_steps_names_the_key():
    from simfire_amd.config import Config, ConfigError
    with pytest.raises(ConfigError, match="train_steps"):
        Config(config_dict=_cfd_config(result_accuracy=1, timestep_dt=1.0, viscosity=1e-7, speed=19, direction="north"))
    with pytest.raises(ConfigError, match="result_accuracy"):
        Config(config_dict=_cfd_config(train_steps=2, timestep_dt=1.0, viscosity=1e-7, speed=19, direction="north"))


def test_config_cfd_rejects_non_square_grid_and_bad_direction():
    from simfire_amd.config import Config, ConfigError
    good = _cfd_config(result_accuracy=1, timestep_dt=1.0, viscosity=1e-7, speed=19, direction="north", train_steps=2)
    d = copy.deepcopy(good)
    d["area"]["screen_size"] = [16, 20]
    with pytest.raises(ConfigError, match="square"):
        Config(config_dict=d)
    with pytest.raises(ConfigError, match="square"):
        Config(config_dict=d, cfd_precompute=True)
    d = copy.deepcopy(good)
    d["wind"]["cfd"]["direction"] = "northeast"
    with pytest.raises(ConfigError, match="northeast"):
        Config(config_dict=d)
    with pytest.raises(ConfigError, match="northeast"):
        Config(config_dict=d, cfd_precompute=True)
    from simfire_amd.wind import cfd_wind_fields, direction_code
    assert [direction_code(s) for s in ("North", "EAST", "south", "West")] == [0, 1, 2, 3]
    with pytest.raises(ConfigError, match="square"):
        cfd_wind_fields(np.zeros((16, 20)), result_accuracy=1, timestep_dt=1.0, viscosity=1e-7, speed=1.0, direction="north",
                        train_steps=1)
