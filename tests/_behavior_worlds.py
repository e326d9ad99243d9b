"""The scenes of ``tests/test_behavior_gpu.py`` / ``tests/test_behavior_cpu.py`` (``sf_behavior``): terrains
with layers (fuel mosaics with an unburnable block, perlin elevation, a wind field), engines in both cell layouts, points, control
lines, and the 5 x 5 hand scene of the rules."""
import numpy as np

import _behavior_oracle as bo

M_F = 0.03
PARTICLE = (8000.0, 0.0555, 0.01, 32.0)
SHAPES = ((9, 9), (33, 17), (40, 130), (64, 64), (70, 1030))
U, B, D, FL, SL, WL = 0, 1, 2, 3, 4, 5
NAMES = ("UNBURNED", "BURNING", "BURNED", "FIRELINE", "SCRATCHLINE", "WETLINE")


def mask_of(names):
    return sum(1 << NAMES.index(n) for n in names) if names else 0


def terrain(seed, H, W, E, codes=(1, 2, 4, 5, 8, 9, 10)):
    """Per environment [w_0, delta, M_x, sigma, elevation, U, U_dir]: a fuel mosaic of its own (the models ``codes``, rotated per
    environment) with a block of w_0 = 0 whose sigma is 0 too, perlin elevation, a wind field."""
    from simfire_amd.parameters import fuel_planes
    from simfire_amd.workloads import perlin_elevation
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    out = []
    for e in range(E):
        mine = [codes[(i + e) % len(codes)] for i in range(3 + e % 3)]
        w0, de, mx, sg = fuel_planes(rng.choice(mine, size=(H, W)))
        w0, sg = w0.copy(), sg.copy()
        py, px = int(rng.integers(0, H - 3)), int(rng.integers(0, W - 3))
        w0[py:py + 3, px:px + 3] = 0.0
        sg[py:py + 2, px:px + 2] = 0.0                   # (384 / 0: an unburnable cell's HPA is 0 whatever its sigma)
        el = perlin_elevation(H, W, 3, 0.7, 2.0, 800 + e + seed, 100.0, 900.0)
        out.append([w0, de, mx, sg, el, 600.0 + 300.0 * np.sin(x / 7.0 + e), 40.0 * e + 25.0 * np.cos(y / 5.0)])
    return out


def engine(H, W, layers, per_env=True, mode="fused0", n_envs=None, **kw):
    """A handle with layers.  ``per_env``: one table per environment (``layers`` has one entry each); else ``layers[0]`` for all
    ``n_envs``.  ``mode``: ``fused0`` (per-step kernels, row-major cells) or ``run`` (the resident launch, blocked cells)."""
    from simfire_amd.engine import FireEngine
    kw = dict(dict(pixel_scale=30.0, max_fire_duration=4, M_f=M_F, particle=PARTICLE), **kw)
    E = len(layers) if per_env else int(n_envs)
    eng = FireEngine((H, W), n_envs=E, per_env_terrain=per_env, **kw)
    eng.set_fused({"fused0": 0, "run": 2}[mode])
    if per_env:
        for e, p in enumerate(layers):
            eng.set_layers(*p, env=e)
    else:
        eng.set_layers(*layers[0])
    return eng


def ignitions(H, W, E, seed=0):
    rng = np.random.default_rng(seed + 31 * H + W)
    return np.stack([rng.integers(W // 4, W - W // 4, size=E), rng.integers(H // 4, H - H // 4, size=E)], axis=1).astype(np.int32)


def line_rows(E, H, W, inits):
    """``apply_mitigation`` rows (env, column, row, type): a short line of each environment's own type two rows below its ignition."""
    rows = []
    for e in range(E):
        x0, y = int(inits[e][0]), min(H - 1, int(inits[e][1]) + 2)
        rows += [(e, x, y, FL + e % 3) for x in range(max(0, x0 - 3), min(W, x0 + 4))]
    return rows


def points(H, W, seed=0, k=13):
    """[k, 3] = (column, row, id): random cells, some off the grid, padding ids, a duplicate, the corners and the borders."""
    rng = np.random.default_rng(H * 1000 + W + seed)
    pts = np.stack([rng.integers(-1, W + 1, size=k), rng.integers(-1, H + 1, size=k), rng.integers(0, 4, size=k)], axis=-1).astype(np.int32)
    pts[0] = (W - 1, H - 1, 1)
    pts[1] = pts[2] = (0, 0, 2)
    pts[3] = (0, 0, 0)
    pts[4] = (W, 0, 1)
    pts[5] = (0, -1, 1)
    pts[6] = (W - 1, 0, 5)
    pts[7] = (0, H - 1, 5)
    pts[8] = (W // 2, 0, 1)
    pts[9] = (0, H // 2, -3)
    return pts


def points_near(inits, H, W, k=13):
    """[E, k, 3]: ``points`` with three entries moved onto and beside each environment's ignition (where the fire is)."""
    out = np.stack([points(H, W, e, k) for e in range(len(inits))])
    for e, (x, y) in enumerate(np.asarray(inits).tolist()):
        out[e, 10] = (x, y, 1)
        out[e, 11] = (min(W - 1, x + 1), max(0, y - 1), 2)
        out[e, 12] = (max(0, x - 2), y, 3)
    return out


def hand_scene():
    """The 5 x 5 scene of the rules: (R8 float64 [8, 5, 5], hpa float32 [5, 5], fire map uint8 [5, 5]).  hpa is 600 BTU/ft2
    everywhere, so with R_head in ft/min: I_B = 10 * R_head and L = 0.45 * (10 R_head) ** 0.46.
      (0, 0): all eight entries 0                   -> head -1, everything 0
      (0, 1): entries 2 and 5 tie at 7.0            -> head 2
      (0, 2): every entry 3.0                       -> head 0
      (1, 1): entry 7 alone, 30.0                   -> head 7; BURNING
      (2, 2): R_head 100 (L = 10.8 ft: class 2)     -> BURNING
      (2, 3): R_head 400 (L = 20.4 ft: class 3)     -> BURNING
      (3, 3): R_head 5 (L = 2.7 ft: class 0)        -> BURNING
      (4, 4): R_head 40 (L = 7.08 ft: class 1)      -> BURNED: not in the default summary
    every other cell: entry 1 = 1.0, UNBURNED."""
    R8 = np.zeros((8, 5, 5))
    R8[1] = 1.0
    R8[:, 0, 0] = 0.0
    R8[:, 0, 1] = [1, 2, 7, 3, 0, 7, 6, 5]
    R8[:, 0, 2] = 3.0
    R8[:, 1, 1] = [0, 0, 0, 0, 0, 0, 0, 30]
    R8[:, 2, 2] = [100, 1, 1, 1, 1, 1, 1, 1]
    R8[:, 2, 3] = [1, 1, 1, 400, 1, 1, 1, 1]
    R8[:, 3, 3] = [1, 1, 5, 1, 1, 1, 1, 1]
    R8[:, 4, 4] = [1, 1, 1, 1, 1, 1, 40, 1]
    fm = np.zeros((5, 5), dtype=np.uint8)
    fm[1, 1] = fm[2, 2] = fm[2, 3] = fm[3, 3] = B
    fm[4, 4] = D
    return R8, np.full((5, 5), 600.0, dtype=np.float32), fm


def expect(eng, envs, layers_of, status_mask=0, per_env=True):
    """The oracle's masked planes for the listed environments, fed with the maps and the handle's OWN tables fetched now (call it
    after the engine computed): [(unmasked planes, masked planes) per listed environment] + the maps.  ``layers_of(e)``: environment
    e's layers; ``per_env``: whether the handle has a table per environment."""
    maps = eng.fire_maps()
    out, cache, tables = [], {}, {}
    for e in envs:
        if e not in cache:
            tab = e if per_env else 0
            if tab not in tables:
                tables[tab] = bo.cells(eng.get_rtable(tab), bo.hpa_plane(layers_of(e), PARTICLE, M_F))
            cache[e] = (tables[tab], bo.masked(tables[tab], maps[e], status_mask))
        out.append(cache[e])
    return out, maps
