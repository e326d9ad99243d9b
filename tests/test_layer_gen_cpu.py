"""Host oracles of the seeded world generators and the ``simplex_topography`` opt-in of ``Config``.

No GPU: ``workloads.fractal_simplex`` / ``perlin_elevation`` against ``simplex_field`` and their own properties, and perlin
topography loaded from the reference's ``configs/functional_config.yml`` (inline: the file is not part of this repository)."""
import copy

import numpy as np
import pytest

from simfire_amd.config import Config, ConfigError
from simfire_amd.workloads import fractal_simplex, perlin_elevation, simplex_field

# configs/functional_config.yml of the reference (simfire v2.0.1), the keys this package reads
FUNCTIONAL = {
    "area": {"screen_size": [225, 225], "pixel_scale": 50},
    "display": {"fire_size": 2, "control_line_size": 2, "agent_size": 4},
    "simulation": {"update_rate": 1, "runtime": "24h", "headless": False, "draw_spread_graph": False, "record": False,
                   "save_data": False, "data_type": "npy", "sf_home": "~/.simfire"},
    "mitigation": {"ros_attenuation": True},
    "operational": {"seed": None, "latitude": 39.67, "longitude": 119.8, "height": 4000, "width": 4000, "resolution": 30, "year": 2020},
    "terrain": {"topography": {"type": "functional",
                               "functional": {"function": "perlin",
                                              "perlin": {"octaves": 3, "persistence": 0.7, "lacunarity": 2.0, "seed": 827,
                                                         "range_min": 100.0, "range_max": 300.0},
                                              "gaussian": {"amplitude": 500, "mu_x": 50, "mu_y": 50, "sigma_x": 50, "sigma_y": 50}}},
                "fuel": {"type": "functional", "functional": {"function": "chaparral", "chaparral": {"seed": 1113}}}},
    "fire": {"fire_initial_position": {"type": "static", "static": {"position": "(16, 16)"}, "random": {"seed": 1234}},
             "max_fire_duration": 4, "diagonal_spread": True},
    "environment": {"moisture": 0.03},
    "wind": {"function": "simple",
             "cfd": {"time_to_train": 1000, "iterations": 1, "scale": 1, "timestep_dt": 1.0, "diffusion": 0.0, "viscosity": 0.0000001,
                     "speed": 19, "direction": "north"},
             "simple": {"speed": 7, "direction": 90.0},
             "perlin": {"speed": {"seed": 2345, "scale": 400, "octaves": 3, "persistence": 0.7, "lacunarity": 2.0, "range_min": 7,
                                  "range_max": 47},
                        "direction": {"seed": 650, "scale": 1500, "octaves": 2, "persistence": 0.9, "lacunarity": 1.0,
                                      "range_min": 0.0, "range_max": 360.0}}},
}


def elev(seed, H=64, W=80, lo=100.0, hi=300.0):
    return perlin_elevation(H, W, 3, 0.7, 2.0, seed, lo, hi)


def test_fractal_simplex_is_simplex_field_before_its_map():
    for args in ((37, 101, 2345, 400, 3, 0.7, 2.0), (64, 64, -7, 12.5, 4, 0.5, 2.0), (50, 30, 300, 1.0, 1, 0.9, 1.0)):
        f = fractal_simplex(*args)
        assert f.dtype == np.float64 and f.shape == args[:2]
        for lo, hi in ((7.0 * 88, 47.0 * 88), (0.0, 360.0)):
            want = simplex_field(*args, lo, hi)
            np.testing.assert_array_equal((((f + 1.0) * (hi - lo)) / 2.0 + lo).astype(np.float32), want)


def test_perlin_elevation_range_and_seeds():
    a = elev(827)
    assert a.dtype == np.float64 and a.shape == (64, 80)
    assert a.min() >= 100.0 and a.max() <= 300.0 and a.std() > 1.0
    np.testing.assert_array_equal(a, elev(827))                    # deterministic in its seed
    assert not np.array_equal(a, elev(828))                        # another seed, another field
    np.testing.assert_array_equal(a, elev(827 + 256))              # simplex2 offsets the permutation indices mod 256
    np.testing.assert_array_equal(elev(-5), elev(251))             # 64-bit (i + seed) & 255: negative seeds as in NumPy
    assert not np.array_equal(elev(0), elev(-5))


def test_perlin_elevation_z_is_float32():
    for seed in (0, 827, -3, 999):
        z = fractal_simplex(64, 80, seed, 1.0, 3, 0.7, 2.0).astype(np.float32).astype(np.float64)
        want = ((z + 1) / 2) * (300.0 - 100.0) + 100.0
        a = elev(seed)
        np.testing.assert_array_equal(a, want)
        back = (a - 100.0) / 200.0 * 2 - 1                          # the float32 z the map was made from (up to rounding of the map)
        assert np.abs(back - z).max() < 1e-12


def test_perlin_elevation_rejects_an_empty_range():
    with pytest.raises(ValueError):
        elev(1, lo=300.0, hi=300.0)
    with pytest.raises(ValueError):
        elev(1, lo=300.0, hi=100.0)


def test_config_simplex_topography_opt_in():
    with pytest.raises(ConfigError):                               # the default is unchanged: perlin topography needs the `noise` wheel
        Config(config_dict=FUNCTIONAL)
    c = Config(config_dict=FUNCTIONAL, simplex_topography=True)
    el = c.terrain.topography_layer.data.squeeze()
    np.testing.assert_array_equal(el, perlin_elevation(225, 225, 3, 0.7, 2.0, 827, 100.0, 300.0))
    assert c.terrain.topography_function.name == "perlin" and c.terrain.topography_function.kwargs["seed"] == 827
    c.reset_terrain(topography_seed=11)
    el11 = c.terrain.topography_layer.data.squeeze()
    assert not np.array_equal(el11, el) and c.terrain.topography_function.kwargs["seed"] == 11
    np.testing.assert_array_equal(el11, perlin_elevation(225, 225, 3, 0.7, 2.0, 11, 100.0, 300.0))
    c.reset_terrain(topography_seed=827)
    np.testing.assert_array_equal(c.terrain.topography_layer.data.squeeze(), el)
    d = copy.deepcopy(FUNCTIONAL)
    del d["terrain"]["topography"]["functional"]["perlin"]["octaves"]
    with pytest.raises(ConfigError, match="octaves"):
        Config(config_dict=d, simplex_topography=True)
    d = copy.deepcopy(FUNCTIONAL)
    d["terrain"]["topography"]["functional"]["perlin"]["range_min"] = 400.0
    with pytest.raises(ValueError):
        Config(config_dict=d, simplex_topography=True)
