"""CFD wind fields on the GPU: the reference's stable-fluids solver (``wind.function: cfd``).

Drop-in for ``WindControllerCFD`` (simfire/world/wind_mechanics/wind_controller.py:100-185), ``Fluid``
(simfire/world/wind_mechanics/cfd_wind.py) and ``generate_cfd_wind_layer`` (simfire/utils/generate_cfd_wind_layer.py:83-115),
run by the HIP library (``sf_cfd_*`` of include/simfire_hip.h): one workgroup per environment, the planes bit-identical to
the reference's float64 loops.  The host forms the terrain mask (the reference's numpy expression) and turns the velocity
into speed and direction (vectorized numpy, the reference's formulas).

The one deliberate difference: the reference trains for ``time_to_train`` wall-clock seconds, so its field depends on the
machine; here training takes a count of iterations (``train_steps``), and one iteration is the reference's loop body,
``iterate_wind_step()`` followed by ``fvect.step()``.
"""
import ctypes as C
import math
from typing import Optional, Tuple

import numpy as np

from . import _lib
from .config import ConfigError

DIRECTIONS = ("north", "east", "south", "west")
MS_TO_FTPM = 196.85       # scale_ms_to_ftpm (simfire/utils/units.py:14-16)


def direction_code(direction) -> int:
    """Inflow side of iterate_wind_step (wind_controller.py:156-170), case-insensitive; anything else is a ``ConfigError``
    (the reference logs an error and trains a field without inflow)."""
    d = str(direction).lower()
    if d not in DIRECTIONS:
        raise ConfigError(f"CFD wind direction `{direction}` is not one of {', '.join(DIRECTIONS)}")
    return DIRECTIONS.index(d)


def terrain_mask(elevation: np.ndarray) -> np.ndarray:
    """wind_controller.py:131-143: 1 where the elevation is above its average, else 0, as uint8 [N, N]."""
    el = np.asarray(elevation)
    return (el > np.average(el)).astype(np.uint8).reshape(el.shape[0], el.shape[1])


_POW = np.vectorize(math.pow, otypes=[np.float64])


def magnitude(vx: np.ndarray, vy: np.ndarray) -> np.ndarray:
    """generate_magnitude_array (generate_cfd_wind_layer.py:57-66), m/s.  The reference squares numpy float64 SCALARS, which
    calls libm's pow(v, 2) - not always the bits of v * v (numpy's array square) - so the squares are taken with math.pow."""
    return np.sqrt(_POW(vx, 2.0) + _POW(vy, 2.0))


def direction_deg(vx: np.ndarray, vy: np.ndarray) -> np.ndarray:
    """generate_direction_array (generate_cfd_wind_layer.py:69-80), degrees."""
    return np.mod(-np.degrees(np.arctan2(-vy, vx)) + 90, 360)


def _square(n) -> int:
    n = tuple(int(v) for v in n)
    if len(n) != 2 or n[0] != n[1]:
        raise ConfigError(f"CFD wind needs a square grid, got screen_size {n} (the reference's set_bnd indexes out of range)")
    if n[0] < 4:
        raise ConfigError(f"CFD wind needs a grid of at least 4 x 4 cells, got {n}")
    return n[0]


class _Solver:
    """One ``sf_cfd`` handle: n_envs solvers of one grid size."""

    def __init__(self, n: int, n_envs: int, result_accuracy: int, timestep_dt: float, viscosity: float, speed: float,
                 direction: int):
        self._lib = _lib.load()
        p = _lib.SfCfdParams(n=n, n_envs=n_envs, result_accuracy=int(result_accuracy), direction=direction,
                             timestep_dt=float(timestep_dt), viscosity=float(viscosity), speed=float(speed))
        h = C.c_void_p()
        _lib.check(self._lib.sf_cfd_create(C.byref(p), C.byref(h)), self._lib)
        self._h = h
        self.n, self.n_envs = n, n_envs

    def set_terrain(self, env: int, mask: np.ndarray) -> None:
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        assert m.shape == (self.n, self.n)
        _lib.check(self._lib.sf_cfd_set_terrain(self._h, int(env), m.ctypes.data), self._lib)

    def step(self, n_steps: int, inflow_every: int) -> None:
        _lib.check(self._lib.sf_cfd_step(self._h, int(n_steps), int(inflow_every)), self._lib)

    def velocity(self, env: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        vx = np.empty((self.n, self.n), dtype=np.float64)
        vy = np.empty((self.n, self.n), dtype=np.float64)
        _lib.check(self._lib.sf_cfd_get_velocity(self._h, int(env), vx.ctypes.data, vy.ctypes.data), self._lib)
        return vx, vy

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.sf_cfd_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


def cfd_velocity(elevation, *, result_accuracy: int, timestep_dt: float, viscosity: float, speed: float, direction,
                 train_steps: int) -> Tuple[np.ndarray, np.ndarray]:
    """``Fluid.Vx``, ``Fluid.Vy`` after ``train_steps`` training iterations, for elevation [N, N], [N, N, 1] or [E, N, N]
    (then [E, N, N] each; every environment has its own terrain mask, all are solved in one batch)."""
    el = np.asarray(elevation)
    batched = el.ndim == 3 and el.shape[-1] != 1
    if not batched and el.ndim == 3:
        el = el[..., 0]
    if el.ndim == 2:
        el = el[None]
    if el.ndim != 3:
        raise ConfigError(f"elevation must be [N, N], [N, N, 1] or [E, N, N], got shape {np.asarray(elevation).shape}")
    n = _square(el.shape[1:])
    code = direction_code(direction)
    if int(train_steps) < 0 or int(result_accuracy) < 0:
        raise ConfigError("train_steps and result_accuracy must be >= 0")
    s = _Solver(n, el.shape[0], result_accuracy, timestep_dt, viscosity, speed, code)
    try:
        for e in range(el.shape[0]):
            s.set_terrain(e, terrain_mask(el[e]))
        s.step(2 * int(train_steps), 2)
        out = [s.velocity(e) for e in range(el.shape[0])]
    finally:
        s.close()
    vx, vy = np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
    return (vx, vy) if batched else (vx[0], vy[0])


def cfd_wind_fields(elevation, *, result_accuracy: int, timestep_dt: float, viscosity: float, speed: float, direction,
                    train_steps: int) -> Tuple[np.ndarray, np.ndarray]:
    """``(speed_ftpm, direction_deg)``, float64, of the CFD wind trained ``train_steps`` iterations over ``elevation``
    ([N, N], [N, N, 1] or [E, N, N]: the result has the same leading shape, one field per environment - for
    ``FireEngine.set_layers(..., env=e)``).  What ``Config`` loads for ``wind.function: cfd`` (config.py:866-891)."""
    vx, vy = cfd_velocity(elevation, result_accuracy=result_accuracy, timestep_dt=timestep_dt, viscosity=viscosity,
                          speed=speed, direction=direction, train_steps=train_steps)
    return magnitude(vx, vy) * MS_TO_FTPM, direction_deg(vx, vy)


class WindControllerCFD:
    """wind_controller.py:100-185 on the GPU: same constructor; ``step()`` is the reference's ``fvect.step()``.
    ``diffusion`` and ``time_to_train`` are kept as attributes only: diffusion drives the density plane, which never feeds the
    velocity, and training here takes a count (``generate_cfd_wind_layer``)."""

    def __init__(self, screen_size: Tuple[int, int] = (225, 450), result_accuracy: int = 1, scale: int = 1,
                 timestep: float = 1.0, diffusion: float = 0.0, viscosity: float = 0.0000001,
                 terrain_features: Optional[np.ndarray] = None, wind_speed: float = 27.0, wind_direction: str = "north",
                 time_to_train: int = 1000) -> None:
        self.N = screen_size
        self.iterations = result_accuracy
        self.scale = scale
        self.timestep = timestep
        self.diffusion = diffusion
        self.viscosity = viscosity
        self.wind_speed = wind_speed
        self.wind_direction = wind_direction
        self.time_to_train = time_to_train
        n = _square(screen_size)
        code = direction_code(wind_direction)
        if terrain_features is None:
            self.terrain_features = np.zeros((n, n), dtype=np.float32)
        else:
            el = np.asarray(terrain_features)
            if el.shape[:2] != (n, n):
                raise ConfigError(f"terrain_features shape {el.shape} does not match screen_size {tuple(screen_size)}")
            self.terrain_features = terrain_mask(el).astype(np.float32)
        self._solver = _Solver(n, 1, result_accuracy, timestep, viscosity, wind_speed, code)
        self._solver.set_terrain(0, self.terrain_features.astype(np.uint8))

    def iterate_wind_step(self) -> None:
        """The inflow, then one Fluid.step() (wind_controller.py:156-172)."""
        self._solver.step(1, 1)

    def step(self) -> None:
        """One Fluid.step() without inflow (the reference's ``fvect.step()``)."""
        self._solver.step(1, 0)

    def train(self, train_steps: int) -> None:
        """``train_steps`` iterations of generate_cfd_wind_layer's loop body (iterate_wind_step(); fvect.step()) in one call."""
        self._solver.step(2 * int(train_steps), 2)

    def get_wind_density_field(self) -> np.ndarray:
        """Zeros: in this flow the density is never non-zero (nothing adds density), and it is not computed."""
        n = self._solver.n
        return np.zeros((n, n))

    def get_wind_velocity_field_x(self) -> np.ndarray:
        return self._solver.velocity(0)[0]

    def get_wind_velocity_field_y(self) -> np.ndarray:
        return self._solver.velocity(0)[1]

    def get_wind_scale(self) -> int:
        return self.scale

    def get_screen_size(self) -> tuple:
        return self.N


def generate_cfd_wind_layer(train_steps: int, cfd_setup: WindControllerCFD) -> Tuple[np.ndarray, np.ndarray]:
    """generate_cfd_wind_layer.py:83-115 with a count instead of a clock: ``train_steps`` iterations of
    ``iterate_wind_step(); fvect.step()`` on ``cfd_setup``, then ``(magnitude_ms, direction_deg)``.  Writes no files (the
    reference saves both arrays under ``pregenerated_wind_files/`` in the working directory)."""
    cfd_setup.train(train_steps)
    vx, vy = cfd_setup._solver.velocity(0)
    return magnitude(vx, vy), direction_deg(vx, vy)
