#!/usr/bin/env python3
"""Generate the CFD wind fixtures ``cfd_*.npz`` in this directory from the REAL reference.

Runs only where the reference is importable (see ``_refshim.py``).  Drives the reference's ``WindControllerCFD`` and ``Fluid``
(simfire/world/wind_mechanics/) directly: the loop body of ``generate_cfd_wind_layer`` (iterate_wind_step(); fvect.step(),
simfire/utils/generate_cfd_wind_layer.py:99-105) for a fixed count of iterations instead of its clock, then the reference's
``generate_magnitude_array`` / ``generate_direction_array``.  Each fixture holds the inputs, the reference's terrain mask,
``Vx, Vy, Vx0, Vy0`` after every iteration and the final speed (m/s) and direction (degrees)::

    python tests/golden/make_golden_cfd.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refshim  # noqa: E402,F401

from simfire.utils import generate_cfd_wind_layer as gen  # noqa: E402
from simfire.utils.layers import FunctionalTopographyLayer  # noqa: E402
from simfire.world import elevation_functions  # noqa: E402
from simfire.world.wind_mechanics.wind_controller import WindControllerCFD  # noqa: E402


def blob_mask(n):
    """Terrain blobs touching rows and columns 1, 2, N-3 and N-2 (the edges of set_bnd's terrain range 2..N-3)."""
    m = np.zeros((n, n))
    m[1:3, n // 3:n // 3 + 2] = 1
    m[n - 3:n - 1, n // 2:n // 2 + 2] = 1
    m[n // 3:n // 3 + 2, 1:3] = 1
    m[n // 2:n // 2 + 3, n - 3:n - 1] = 1
    m[n // 2 - 1:n // 2 + 1, n // 2 - 1:n // 2 + 2] = 1
    return m


def random_mask(n, seed):
    return (np.random.default_rng(seed).random((n, n)) < 0.3).astype(np.float64)


def gaussian_topography():
    """The 9 x 9 gaussian topography of configs/test_config_gaussian.yml, made by the reference's own layer."""
    fn = elevation_functions.gaussian(amplitude=500, mu_x=50, mu_y=50, sigma_x=50, sigma_y=50)
    return FunctionalTopographyLayer(9, 9, fn, "gaussian").data


def run(name, n, direction, itr, iterations, elevation=None, speed=19.0, dt=1.0, visc=0.0000001):
    wc = WindControllerCFD(screen_size=(n, n), result_accuracy=itr, scale=1, timestep=dt, diffusion=0.0, viscosity=visc,
                           terrain_features=elevation, wind_speed=speed, wind_direction=direction, time_to_train=0)
    planes = []
    for _ in range(iterations):
        wc.iterate_wind_step()
        wc.fvect.step()
        f = wc.fvect
        planes.append(np.stack([f.Vx, f.Vy, f.Vx0, f.Vy0]))
    vx, vy = wc.get_wind_velocity_field_x(), wc.get_wind_velocity_field_y()
    out = dict(n=n, direction=direction, result_accuracy=itr, iterations=iterations, speed=speed, timestep_dt=dt,
               viscosity=visc, has_elevation=elevation is not None,
               elevation=np.zeros((n, n)) if elevation is None else np.asarray(elevation, dtype=np.float64),
               mask=np.asarray(wc.terrain_features, dtype=np.float64).reshape(n, n), planes=np.stack(planes),
               magnitude=gen.generate_magnitude_array(vx, vy), direction_deg=gen.generate_direction_array(vx, vy))
    np.savez_compressed(os.path.join(HERE, f"cfd_{name}.npz"), **out)
    print(name, "max |V|", float(np.abs(out["planes"][-1, :2]).max()))


def main():
    dirs = ("north", "east", "south", "west")
    for k, (n, d) in enumerate(zip((9, 10, 17, 24), dirs)):
        run(f"n{n}_{d}_flat", n, d, 1 + k % 3, 3)
    for k, (n, d) in enumerate(zip((10, 17, 24, 32), dirs)):
        run(f"n{n}_{d}_random", n, d, 1 + (k + 1) % 3, 3, elevation=random_mask(n, 100 + n), speed=5.3)
    for k, (n, d) in enumerate(zip((17, 24, 32, 9), dirs)):
        run(f"n{n}_{d}_blobs", n, d, 1 + (k + 2) % 3, 3, elevation=blob_mask(n))
    run("n17_north_viscous", 17, "north", 3, 3, elevation=blob_mask(17), dt=0.1, visc=0.05)
    run("n9_north_gaussian", 9, "north", 1, 4, elevation=gaussian_topography(), speed=19)
    run("n32_south_flat_long", 32, "South", 2, 6)


if __name__ == "__main__":
    main()
