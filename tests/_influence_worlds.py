"""Hand-made forests for ``sf_influence``: parent-code planes, weights and include planes, and what each scene is
there for.  Shared by ``tests/test_influence_cpu.py`` (the oracle alone) and ``tests/test_influence_gpu.py`` (the engine against it).
A code is an index into ``SRC_OFFSETS`` = (dx, dy): 0 (+1,+1) 1 (0,+1) 2 (-1,+1) 3 (+1,0) 4 (-1,0) 5 (+1,-1) 6 (0,-1) 7 (-1,-1).
The shapes: one workgroup and an odd width (9 x 9), W % 4 != 0 (33 x 17), several workgroups (40 x 130, 64 x 64) and a wide grid whose
serpentine is 72 100 cells high (70 x 1030)."""
import numpy as np

SCENE_SHAPES = ((9, 9), (33, 17), (40, 130), (64, 64), (70, 1030))
SRC_OFFSETS = ((+1, +1), (0, +1), (-1, +1), (+1, 0), (-1, 0), (+1, -1), (0, -1), (-1, -1))
RIGHT, LEFT, DOWN, UP, UP_LEFT = 3, 4, 1, 6, 7
PIXEL_SCALE = 30.0


def engine_kwargs(H, W, diag=True, md=4):
    return dict(shape=(H, W), max_fire_duration=md, pixel_scale=PIXEL_SCALE, update_rate=1.0, max_time=None, attenuate_line_ros=False,
                diagonal_spread=diag)


def none(H, W):
    return np.full((H, W), -1, dtype=np.int8)


def serpentine(H, W):
    """ONE chain over the whole grid, the greatest height there is: even rows run towards column 0, odd rows towards column W - 1,
    the last cell of a row climbs to the row above.  The root is (0, 0)."""
    p = none(H, W)
    p[0::2, :] = LEFT
    p[0::2, 0] = UP
    p[1::2, :] = RIGHT
    p[1::2, W - 1] = UP
    p[0, 0] = -1
    return p


def star(H, W):
    """Eight children of the centre cell and nothing else: siblings that collide on one accumulator."""
    p = none(H, W)
    cy, cx = H // 2, W // 2
    for k, (dx, dy) in enumerate(SRC_OFFSETS):
        p[cy - dy, cx - dx] = k
    return p


def comb(H, W):
    """Row 0 is the spine (towards column 0), every other cell climbs its column."""
    p = np.full((H, W), UP, dtype=np.int8)
    p[0, :] = LEFT
    p[0, 0] = -1
    return p


def one_tree(H, W):
    """One tree covering the grid, along the diagonals: the interior points up-left, the first row and column lead to (0, 0)."""
    p = np.full((H, W), UP_LEFT, dtype=np.int8)
    p[0, :] = LEFT
    p[:, 0] = UP
    p[0, 0] = -1
    return p


def random_forest(H, W, seed=0):
    """Every cell points at a random neighbour if that one is on the grid and of lower random priority: acyclic, bushy, many roots."""
    rng = np.random.default_rng(2800 + seed)
    prio = rng.permutation(H * W).reshape(H, W)
    code = rng.integers(0, 8, size=(H, W))
    p = none(H, W)
    for y in range(H):
        for x in range(W):
            dx, dy = SRC_OFFSETS[code[y, x]]
            if 0 <= x + dx < W and 0 <= y + dy < H and prio[y + dy, x + dx] < prio[y, x]:
                p[y, x] = code[y, x]
    return p


def two_cycle(H, W):
    p = none(H, W)
    p[1, 1], p[1, 2] = RIGHT, LEFT
    return p


def fed_cycle(H, W):
    """A cycle of four cells, (2,2) -> (3,2) -> (3,3) -> (2,3) -> (2,2) as (x, y), in a grid whose other cells climb their columns:
    the columns 2 and 3 below row 3 are trees that feed into the cycle, the cells above it and the other columns are plain chains."""
    p = np.full((H, W), UP, dtype=np.int8)
    p[2, 2], p[2, 3], p[3, 3], p[3, 2] = RIGHT, DOWN, LEFT, UP
    return p


def off_grid(H, W):
    """Codes that point off the grid on all four borders - the last column's RIGHT would land in the next row of a dense plane - and
    diagonally at the corners; the interior runs towards column 0, whose cells are the roots."""
    p = np.full((H, W), LEFT, dtype=np.int8)
    p[0, :], p[H - 1, :] = UP, DOWN
    p[:, W - 1] = RIGHT
    p[0, 0], p[0, W - 1], p[H - 1, 0], p[H - 1, W - 1] = 7, 5, 2, 0
    return p


def bad_bytes(H, W):
    """A random forest with the bytes 8, -2 and 127 sprinkled in: no parent, not an error."""
    rng = np.random.default_rng(2899)
    p = random_forest(H, W, 7)
    hit = rng.random((H, W)) < 0.15
    p[hit] = rng.choice(np.array([8, -2, 127], dtype=np.int8), size=int(hit.sum()))
    p[0, 0], p[0, 1], p[1, 0] = 8, -2, 127
    return p


HAND_MADE = (("serpentine", serpentine), ("star", star), ("comb", comb), ("one_tree", one_tree), ("random_0", lambda H, W: random_forest(H, W, 0)),
             ("random_1", lambda H, W: random_forest(H, W, 1)), ("two_cycle", two_cycle), ("fed_cycle", fed_cycle), ("off_grid", off_grid),
             ("bad_bytes", bad_bytes), ("all_none", none))


def scenes(H, W):
    """[dict(name, pred)] for an H x W grid (H >= 5, W >= 4)."""
    return [dict(name=name, pred=make(H, W)) for name, make in HAND_MADE]


def weights(H, W, seed=0):
    """int32 [H, W]: negative entries, and large ones - a chain of three already sums beyond 2^31."""
    rng = np.random.default_rng(2850 + seed)
    w = rng.integers(-(1 << 30), (1 << 31) - 1, size=(H, W), dtype=np.int64)
    w[rng.random((H, W)) < 0.2] = 0
    w[0, 0] = (1 << 31) - 1
    w[H - 1, W - 1] = -(1 << 31)
    return w.astype(np.int32)


def include(H, W, seed=0):
    """uint8 [H, W]: about a third of the cells knocked out, interior links among them (a knocked-out cell still hands its children on)."""
    rng = np.random.default_rng(2870 + seed)
    inc = (rng.random((H, W)) < 0.67).astype(np.uint8) * rng.integers(1, 256, size=(H, W)).astype(np.uint8)
    inc[H // 2, W // 2] = 0
    return inc


def default_points(H, W, seed=0, k=12):
    """int32 [k, 3]: random points, some off the grid or padding (id <= 0), a duplicate pair, the far corner, the cycle cell (2, 2) of
    ``fed_cycle`` / ``two_cycle``'s (1, 1), and a cell below the cycle whose route runs into it."""
    rng = np.random.default_rng(2880 + seed)
    pts = np.stack([rng.integers(-2, W + 2, size=k), rng.integers(-2, H + 2, size=k), rng.integers(-1, 4, size=k)], axis=-1).astype(np.int32)
    pts[0] = (W - 1, H - 1, 1)
    pts[1] = pts[2] = (W // 2, H // 2, 2)
    pts[3] = (0, 0, 0)
    pts[4] = (W, 0, 1)
    pts[5] = (0, -1, 1)
    pts[6] = (2, 2, 5)
    pts[7] = (1, 1, 1)
    pts[8] = (2, H - 1, 1)
    pts[9] = (0, 0, 3)
    return pts
