"""numpy restatement of the reference's CFD wind solver (simfire/world/wind_mechanics/cfd_wind.py, wind_controller.py:100-185),
the yardstick of the sf_cfd_* tests.  Every value is the reference's float64 expression in its evaluation order, so the planes
are bit-identical to the Python loops (tests/test_cfd_cpu.py checks that against fixtures made by the reference itself).

The in-place Gauss-Seidel pass of lin_solve (j outer, i inner) is evaluated along anti-diagonals i + j = s: cell (i, j) reads
(i-1, j) and (i, j-1) from this pass (diagonal s - 1) and (i+1, j), (i, j+1) from before it (diagonal s + 1), so a whole
diagonal at once gives the same bits - and is fast enough at 225^2 and above.  set_bnd's terrain step is order-free (a mask
cell in rows / columns 2..N-3 becomes 0.0, every other cell is negated once per such mask neighbour on the b axis).
"""
import math

import numpy as np

DIRECTIONS = ("north", "east", "south", "west")
_DIAG = {}


def _diagonals(N):
    if N not in _DIAG:
        out = []
        for s in range(2, 2 * (N - 2) + 1):
            i = np.arange(max(1, s - (N - 2)), min(N - 2, s - 1) + 1)
            out.append((i, s - i))
        _DIAG[N] = out
    return _DIAG[N]


def terrain_mask(elevation):
    el = np.asarray(elevation)
    return (el > np.average(el)).astype(np.uint8).reshape(el.shape[0], el.shape[1])


def set_bnd(b, x, mask):
    N = x.shape[0]
    r = slice(1, N - 1)
    x[r, 0] = -x[r, 1] if b == 2 else x[r, 1]
    x[r, N - 1] = -x[r, N - 2] if b == 2 else x[r, N - 2]
    x[0, r] = -x[1, r] if b == 1 else x[1, r]
    x[N - 1, r] = -x[N - 2, r] if b == 1 else x[N - 2, r]
    x[0, 0] = 0.5 * (x[1, 0] + x[0, 1])
    x[0, N - 1] = 0.5 * (x[1, N - 1] + x[0, N - 2])
    x[N - 1, 0] = 0.5 * (x[N - 2, 0] + x[N - 1, 1])
    x[N - 1, N - 1] = 0.5 * (x[N - 2, N - 1] + x[N - 1, N - 2])
    if b in (1, 2):
        m = mask.astype(bool)
        M = np.zeros_like(m)
        M[2:N - 2, 2:N - 2] = m[2:N - 2, 2:N - 2]
        cnt = np.zeros(x.shape, dtype=np.int32)
        if b == 2:
            cnt[:, :-1] += M[:, 1:]
            cnt[:, 1:] += M[:, :-1]
        else:
            cnt[:-1, :] += M[1:, :]
            cnt[1:, :] += M[:-1, :]
        flip = ~m & (cnt % 2 == 1)
        x[flip] = -x[flip]
        x[M] = 0.0


def lin_solve(b, x, x0, a, c, itr, mask):
    cr = 1.0 / c
    m = mask.astype(bool)
    for _ in range(itr):
        for i, j in _diagonals(x.shape[0]):
            calc = (x0[i, j] + a * (((x[i + 1, j] + x[i - 1, j]) + x[i, j + 1]) + x[i, j - 1])) * cr
            x[i, j] = np.where(m[i, j], 0.0, calc)
        set_bnd(b, x, mask)


def diffuse(b, x, x0, visc, dt, itr, mask):
    N = x.shape[0]
    a = dt * visc * (N - 2) * (N - 2)
    lin_solve(b, x, x0, a, 1 + 6 * a, itr, mask)


def project(u, v, p, div, itr, mask):
    N = u.shape[0]
    r = slice(1, N - 1)
    div[r, r] = (-0.5 * (((u[2:, r] - u[:-2, r]) + v[r, 2:]) - v[r, :-2])) / N
    p[r, r] = 0.0
    set_bnd(0, div, mask)
    set_bnd(0, p, mask)
    lin_solve(0, p, div, 1, 6, itr, mask)
    u[r, r] = u[r, r] - (0.5 * (p[2:, r] - p[:-2, r])) * N
    v[r, r] = v[r, r] - (0.5 * (p[r, 2:] - p[r, :-2])) * N
    set_bnd(1, u, mask)
    set_bnd(2, v, mask)


def advect(b, d, d0, u, v, dt, mask):
    """cfd_wind.py:250-298, including its quirk: only `s0 * (t0*d0[i0][j0] + t1*d0[i0][j1])` is assigned (the `+s1*(...)` on the
    next line is a separate statement whose value is discarded)."""
    N = d.shape[0]
    r = slice(1, N - 1)
    dtx = dt * (N - 2)
    I, J = np.meshgrid(np.arange(1, N - 1), np.arange(1, N - 1), indexing="ij")
    x = I - dtx * u[r, r]
    y = J - dtx * v[r, r]
    hi = (N - 2) + 0.5
    x = np.where(x < 0.5, 0.5, x)
    x = np.where(x > hi, hi, x)
    y = np.where(y < 0.5, 0.5, y)
    y = np.where(y > hi, hi, y)
    i0, j0 = np.floor(x), np.floor(y)
    s1 = x - i0
    s0 = 1.0 - s1
    t1 = y - j0
    t0 = 1.0 - t1
    i0, j0 = i0.astype(np.int64), j0.astype(np.int64)
    d[r, r] = s0 * (t0 * d0[i0, j0] + t1 * d0[i0, j0 + 1])
    set_bnd(b, d, mask)


class Fluid:
    """The velocity part of cfd_wind.Fluid (density and `s` never feed it)."""

    def __init__(self, n, itr, dt, visc, mask=None):
        self.N, self.itr, self.dt, self.visc = n, itr, dt, visc
        self.mask = np.zeros((n, n), np.uint8) if mask is None else np.asarray(mask, np.uint8)
        self.Vx, self.Vy, self.Vx0, self.Vy0 = (np.zeros((n, n)) for _ in range(4))

    def step(self):
        m, itr = self.mask, self.itr
        diffuse(1, self.Vx0, self.Vx, self.visc, self.dt, itr, m)
        diffuse(2, self.Vy0, self.Vy, self.visc, self.dt, itr, m)
        project(self.Vx0, self.Vy0, self.Vx, self.Vy, itr, m)
        advect(1, self.Vx, self.Vx0, self.Vx0, self.Vy0, self.dt, m)
        advect(2, self.Vy, self.Vy0, self.Vx0, self.Vy0, self.dt, m)
        project(self.Vx, self.Vy, self.Vx0, self.Vy0, itr, m)

    def inflow(self, direction, speed):
        """WindControllerCFD.iterate_wind_step's addVelocity loop (wind_controller.py:156-168)."""
        N, d = self.N, DIRECTIONS.index(str(direction).lower())
        if d == 0:
            self.Vx[:, 1] += 0
            self.Vy[:, 1] += speed
        elif d == 1:
            self.Vx[N - 1, :] += -1 * speed
            self.Vy[N - 1, :] += 0
        elif d == 2:
            self.Vx[1, :] += -1 * speed
            self.Vy[1, :] += 0
        else:
            self.Vx[1, :] += speed
            self.Vy[1, :] += 0

    def iterate_wind_step(self, direction, speed):
        self.inflow(direction, speed)
        self.step()

    def train(self, iterations, direction, speed):
        """generate_cfd_wind_layer's loop body (generate_cfd_wind_layer.py:99-105), `iterations` times."""
        for _ in range(iterations):
            self.iterate_wind_step(direction, speed)
            self.step()


def velocity(elevation, *, result_accuracy, timestep_dt, viscosity, speed, direction, train_steps):
    el = np.asarray(elevation)
    f = Fluid(el.shape[0], result_accuracy, timestep_dt, viscosity, terrain_mask(el))
    f.train(train_steps, direction, speed)
    return f.Vx, f.Vy


def wind_fields(elevation, **kw):
    """(speed ft/min, direction degrees) as Config loads them for `wind.function: cfd`."""
    vx, vy = velocity(elevation, **kw)
    sq = np.vectorize(lambda v: math.pow(v, 2), otypes=[np.float64])       # the reference squares scalars: libm pow
    return np.sqrt(sq(vx) + sq(vy)) * 196.85, np.mod(-np.degrees(np.arctan2(-vy, vx)) + 90, 360)
