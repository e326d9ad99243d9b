"""Scenes for ``sf_perimeter``: hand-made sets of cells on an ``H`` x ``W`` grid - each made to go wrong in one
place of a tracer - and random ones at three densities.  A scene is ``dict(name, mask)`` with ``mask`` bool [H, W]; ``fire_map`` turns
a mask into a BurnStatus map whose BURNING | BURNED cells are the mask (the other cells UNBURNED with a sprinkle of control lines)."""
import numpy as np

SCENE_SHAPES = ((1, 1), (3, 5), (16, 64), (17, 65), (33, 130), (40, 1030))
PIXEL_SCALE = 30.0
U, B, D, FL = 0, 1, 2, 3


def engine_kwargs(H, W, diag=True, md=4):
    return dict(shape=(H, W), max_fire_duration=md, pixel_scale=PIXEL_SCALE, update_rate=1.0, max_time=None, attenuate_line_ros=False,
                diagonal_spread=diag)


def slow_table(H, W):
    """A uniform R table under which one update ignites nothing (a cell takes ten)."""
    return np.full((8, H, W), 3.0)


def fire_map(mask):
    """uint8 [H, W]: the mask's cells BURNING or BURNED (mixed), the rest UNBURNED or, here and there, FIRELINE."""
    mask = np.asarray(mask, dtype=bool)
    H, W = mask.shape
    y, x = np.mgrid[0:H, 0:W]
    m = np.where((x + 2 * y) % 7 == 0, FL, U).astype(np.uint8)
    m[mask] = np.where((7 * x + 3 * y) % 5 == 0, B, D)[mask]
    return m


def empty(H, W):
    return np.zeros((H, W), dtype=bool)


def full(H, W):
    return np.ones((H, W), dtype=bool)


def corner_cell(H, W):
    m = empty(H, W)
    m[H - 1, W - 1] = True
    return m


def one_cell_hole(H, W):
    m = empty(H, W)
    m[0:min(3, H), 0:min(3, W)] = True
    if H >= 3 and W >= 3:
        m[1, 1] = False
    return m


def nested_rings(H, W):
    """Squares inside squares, two cells apart: ring, gap, ring, ... - outer loops and holes in turn."""
    m = empty(H, W)
    k = 0
    while 2 * k < min(H, W):
        m[k:H - k, k:W - k] = k % 2 == 0
        k += 1
    return m


def saddle_pair(H, W):
    """Two cells that touch at a corner, and a second pair the other way round: one loop each under 4, one loop a pair under 8."""
    m = empty(H, W)
    if H >= 2 and W >= 2:
        m[0, 0] = m[1, 1] = True
    if H >= 2 and W >= 5:
        m[1, 3] = m[0, 4] = True
    if H >= 5 and W >= 3:                         # a saddle inside a block: the hole's corner touches the outside's
        m[2:5, 0:3] = True
        m[3, 1] = False
        if W >= 4 and H >= 6:
            m[5, 3] = True
    return m


def checkerboard(H, W):
    y, x = np.mgrid[0:H, 0:W]
    return (x + y) % 2 == 0


def serpentine(H, W, thick=1):
    """Bands of ``thick`` rows, ``thick`` rows apart, joined at alternating ends: one long loop."""
    m = empty(H, W)
    k = 0
    for y in range(H):
        band, inside = divmod(y, 2 * thick)
        if inside < thick:
            m[y, :] = True
        elif y + (2 * thick - inside) < H:                    # a joint, where another band follows
            m[y, W - 1 if band % 2 == 0 else 0] = True
    return m


def spiral(H, W):
    """A turtle that walks clockwise from the corner and keeps one cell between its track and itself: one loop that winds inwards."""
    m = empty(H, W)
    y, x, d = 0, 0, 0
    m[0, 0] = True
    step = ((0, 1), (1, 0), (0, -1), (-1, 0))

    def free(yy, xx):
        return not (0 <= yy < H and 0 <= xx < W) or not m[yy, xx]
    turns = 0
    while turns < 2:
        dy, dx = step[d]
        ny, nx = y + dy, x + dx
        if 0 <= ny < H and 0 <= nx < W and not m[ny, nx] and free(ny + dy, nx + dx):
            y, x, turns = ny, nx, 0
            m[y, x] = True
        else:
            d, turns = (d + 1) % 4, turns + 1
    return m


def four_borders(H, W):
    """A cross that touches all four borders, with a blob off each arm."""
    m = empty(H, W)
    m[H // 2, :] = True
    m[:, W // 2] = True
    m[0, 0] = m[H - 1, W - 1] = True
    return m


def run_to_word_boundary(H, W):
    """Runs that end exactly at column 63 / 64 (a 64-bit word boundary) and one that crosses it; further ones at 127 / 128."""
    m = empty(H, W)
    for r, (a, b) in enumerate(((40, 64), (64, 80), (50, 70), (63, 64), (64, 65), (120, 128), (128, 140), (0, W))):
        if 2 * r < H:
            m[2 * r, min(a, W):min(b, W)] = True
    return m


def band_rows(H, W):
    """A band that ends at row 15 and one that ends at row 16 (either side of a boundary of 16 rows), and a cell below the first
    band's corner that only the 8-neighbourhood joins to it."""
    m = empty(H, W)
    m[max(0, min(12, H - 1)):min(16, H), 1:max(2, W // 3)] = True
    if H > 16:
        m[13:17, W // 2:max(W // 2 + 1, W - 1)] = True
        m[16, max(2, W // 3)] = True
    return m


def random_mask(seed, H, W, density):
    return np.random.default_rng(seed).random((H, W)) < density


HAND_MADE = (("empty", empty), ("full", full), ("corner_cell", corner_cell), ("one_cell_hole", one_cell_hole), ("nested_rings", nested_rings),
             ("saddle_pair", saddle_pair), ("checkerboard", checkerboard), ("serpentine", serpentine), ("spiral", spiral),
             ("four_borders", four_borders), ("run_to_word_boundary", run_to_word_boundary), ("band_rows", band_rows))


def scenes(H, W):
    out = [dict(name=name, mask=np.ascontiguousarray(f(H, W), dtype=bool)) for name, f in HAND_MADE]
    for k, density in enumerate((0.08, 0.5, 0.9)):
        out.append(dict(name="random_%d" % k, mask=random_mask(2700 + 31 * k + H * 7 + W, H, W, density)))
    return out


def per_env_member(E, H, W):
    """uint8 [E, H, W]: a different random set per environment (values 0, 1 and 255)."""
    rng = np.random.default_rng(2750 + E)
    return (rng.random((E, H, W)) < np.linspace(0.1, 0.8, E)[:, None, None]).astype(np.uint8) * rng.choice([1, 255], size=(E, H, W)).astype(np.uint8)
