"""The worlds of ``tests/test_reach_gpu.py`` and the loops that drive them.  A handle is anything with the older API (``reset``,
``step``, ``apply_mitigation``, ``load_fire_map``, ``fire_map``): the GPU test drives an engine and asks it for the reach at every
query point; ``tests/test_reach_cpu.py`` drives ``StandIn`` (``_arrival_worlds.DenseStandIn`` + ``load_fire_map``) through the same
loops and checks with ``_reach_oracle`` what the scenes claim and that the reach is a superset of every later fire."""
import numpy as np

import _arrival_worlds as aw
import _reach_oracle as ro

U, B, D, FL, SL, WL = 0, 1, 2, 3, 4, 5            # UNBURNED, BURNING, BURNED, FIRELINE, SCRATCHLINE, WETLINE
CALLS = (1, 2, 3, 5, 7, 11)                       # updates per call; a query behind each
MASK_PAIRS = ((("BURNING",), ("UNBURNED",)),
              (("BURNING",), ("UNBURNED",) + ro.LINES),
              (("BURNING", "BURNED"), ("UNBURNED",)),
              (("FIRELINE",), ("UNBURNED", "BURNED")))
CONNS = (0, 4, 8)
EPISODE_CASES = ("24x40", "33x17", "70x1030_wide", "72x80_win", "136x64_team")
PAIRS = [(case, mode) for case in EPISODE_CASES for mode in aw.CASES[case]["modes"]]
SCENE_SHAPES = ((9, 9), (33, 17), (40, 130), (70, 1030), (64, 64))


class StandIn(aw.DenseStandIn):
    """``DenseStandIn`` with the ``load_fire_map`` of the engines."""

    def load_fire_map(self, e, fire_map):
        self.o[e].load_fire_map(0, np.ascontiguousarray(fire_map, dtype=np.uint8))


def queries(case, mode):
    """[(updates of the call, source names, through names, connectivity)]: pairs and connectivities cycle with the calls from an
    offset the mode picks - six calls, so every mode meets all four pairs and all three connectivities."""
    off = aw.CASES[case]["modes"].index(mode)
    return [(n,) + MASK_PAIRS[(i + off) % 4] + (CONNS[(i + 2 * off) % 3],) for i, n in enumerate(CALLS)]


def draws_lines(case, mode):
    """The modes of a case with an odd index draw control lines between their calls (136x64_team has one mode: it draws)."""
    return aw.CASES[case]["modes"].index(mode) % 2 == 1 or len(aw.CASES[case]["modes"]) == 1


def line_rows(i, E, H, W, inits):
    """Control lines behind call i as ``apply_mitigation`` rows (env, column, row, type): a horizontal piece below and a diagonal piece
    beside every ignition, of the three types in turn - diagonals leak under 8-connectivity."""
    rows = []
    for e in range(E):
        x0, y0 = int(inits[e][0]), int(inits[e][1])
        t = FL + (i + e) % 3
        if i % 2 == 1:
            y = min(H - 1, y0 + 3 + i)
            rows += [(e, x, y, t) for x in range(max(0, x0 - 9), min(W, x0 + 10))]
        else:
            rows += [(e, x0 + 4 + i + d, y0 - 4 + d, t) for d in range(9) if 0 <= x0 + 4 + i + d < W and 0 <= y0 - 4 + d < H]
    return rows


def run_episode(case, mode, h, inits, on_query, H, W):
    """reset, then per call: ``h.step(n)``, ``on_query(i, n, source, through, connectivity)`` and - where the mode draws - lines."""
    h.reset(inits)
    for i, (n, src, thr, conn) in enumerate(queries(case, mode)):
        h.step(n)
        on_query(i, n, src, thr, conn)
        if draws_lines(case, mode) and i in (1, 2, 4):
            h.apply_mitigation(line_rows(i, h.n_envs, H, W, inits))


# ------------------------------------------------------------------------------------------------ hand-made scenes
def _serpentine(H, W, vertical):
    """Walls on every second row (column) with one gap at alternating ends: one corridor that visits every open cell."""
    m = np.zeros((W, H) if vertical else (H, W), dtype=np.uint8)
    for k, y in enumerate(range(1, m.shape[0], 2)):
        m[y, :] = FL
        m[y, -1 if k % 2 == 0 else 0] = U
    m[0, 0] = B
    return m.T.copy() if vertical else m


def _spiral(H, W):
    """Concentric wall rings two cells apart, each with one gap, the gaps at alternating ends: the way in winds round every ring."""
    m = np.zeros((H, W), dtype=np.uint8)
    k = 0
    while 2 * k + 1 < min(H, W) // 2:
        a = 2 * k + 1
        m[a, a:W - a] = FL
        m[H - 1 - a, a:W - a] = FL
        m[a:H - a, a] = FL
        m[a:H - a, W - 1 - a] = FL
        if k % 2 == 0:
            m[a, a + 1] = U
        else:
            m[H - 1 - a, W - 2 - a] = U
        k += 1
    m[0, 0] = B
    return m


def _ring(H, W, closed):
    m = np.zeros((H, W), dtype=np.uint8)
    cy, cx = H // 2, W // 2
    y0, y1, x0, x1 = max(cy - 3, 1), min(cy + 3, H - 2), max(cx - 3, 1), min(cx + 3, W - 2)
    m[y0, x0:x1 + 1] = FL
    m[y1, x0:x1 + 1] = FL
    m[y0:y1 + 1, x0] = FL
    m[y0:y1 + 1, x1] = FL
    m[cy, cx] = B
    if not closed:
        m[y0, x0 + 1] = U
    inside = (y1 - y0 - 1) * (x1 - x0 - 1) - 1
    ring = 2 * (y1 - y0 + 1) + 2 * (x1 - x0 + 1) - 4
    return m, inside, ring


def scenes(H, W):
    """[dict(name, map, source, through, conn, passable, expect, points)] for an H x W grid.  ``expect``: the count the scene claims
    (None: only equality with the oracle is claimed); ``passable``: None, a plane, or "per_env"; ``points``: [k, 3] or None."""
    burning, unburned = ("BURNING",), ("UNBURNED",)
    out = []

    def add(name, m, conn, expect=None, source=burning, through=unburned, passable=None, points=None):
        out.append(dict(name=name, map=np.ascontiguousarray(m, dtype=np.uint8), source=source, through=through, conn=conn,
                        passable=passable, expect=expect, points=points))
    long_paths = (H, W) in ((33, 17), (40, 130))           # (the oracle walks a corridor one cell per dilation: no longer ones)
    if long_paths:
        for vertical in (False, True):                                                                      # (a)
            m = _serpentine(H, W, vertical)
            for conn in (4, 8):
                add("serpentine_%s_%d" % ("v" if vertical else "h", conn), m, conn, int((m == U).sum()))
    if long_paths and W > 100:
        m = _spiral(H, W)                                                                                   # (b)
        add("spiral_4", m, 4, int((m == U).sum()))
        add("spiral_8", m, 8, int((m == U).sum()))
    if H == W:                                                                                              # (c)
        m = np.zeros((H, W), dtype=np.uint8)
        m[np.arange(H), W - 1 - np.arange(H)] = FL
        m[0, 0] = B
        add("diagonal_8", m, 8, H * W - H - 1)
        add("diagonal_4", m, 4, H * (H - 1) // 2 - 1)
    if H >= 9 and W >= 9:                                                                                   # (d)
        m, inside, ring = _ring(H, W, True)
        outside = np.array([(0, 0, 1), (W - 1, H - 1, 2), (W // 2, 0, 3), (W // 2, H // 2 - 1, 4)], dtype=np.int32)
        add("ring_closed", m, 8, inside, points=outside)
        m, inside, ring = _ring(H, W, False)
        add("ring_open", m, 4, H * W - ring - 1 + 1, points=outside)
    if W >= 130 and H >= 30:                                                                                # (e)
        for name, g64, g128 in (("gaps_a", ("h", 10), ("d", 21)), ("gaps_b", ("d", 12), ("h", 7)), ("gaps_c", ("u", 13), ("h", 8))):
            m = np.zeros((H, W), dtype=np.uint8)
            for col, (kind, row) in ((63, g64), (127, g128)):
                m[:, col] = FL
                m[:, col + 1] = FL
                m[row, col] = U
                m[row + {"h": 0, "d": 1, "u": -1}[kind], col + 1] = U
            m[5, 5] = B
            walls = int((m == FL).sum())
            diag_first = g64[0] != "h"
            add(name + "_8", m, 8, H * W - walls - 1)
            # without diagonals the fill stops in the first gap cell of the diagonal crossing
            left = 63 * H - 1 + 1
            mid = left + 1 + 62 * H + 1
            add(name + "_4", m, 4, left if diag_first else mid)
    wall = np.zeros((H, W), dtype=np.uint8)                                                                 # (f): the only way round is the padding
    if H >= 5:
        wall[H // 2, :] = FL
        wall[0, W - 1] = B
        add("wall_to_the_last_column_8", wall, 8, (H // 2) * W - 1)
        add("wall_to_the_last_column_4", wall, 4, (H // 2) * W - 1)
    m = np.zeros((H, W), dtype=np.uint8)                                                                    # (h)
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1)):
        m[y, x] = B
    add("borders", m, 4, H * W - int((m == B).sum()))
    add("no_seed", np.zeros((H, W), dtype=np.uint8), 8, 0)                                                   # (i)
    m = np.full((H, W), D, dtype=np.uint8)                                                                  # (j)
    m[H // 2, W // 2] = B
    m[0, W - 1] = B
    add("nothing_open", m, 8, 0)
    m = np.zeros((H, W), dtype=np.uint8)                                                                    # (k), also (g) on W = 64
    m[H - 1, W - 1] = B
    add("all_but_one", m, 4, H * W - 1)
    add("lines_are_seeds", np.where(wall == B, U, wall), 8, H * W - W, source=("FIRELINE",), through=("UNBURNED", "BURNED")) if H >= 5 else None
    if W >= 9:                                                                                              # (l)
        m = np.zeros((H, W), dtype=np.uint8)
        m[0, 0] = B
        p = np.full((H, W), 200, dtype=np.uint8)
        p[:, W // 2] = 0
        add("passable_shared", m, 8, H * (W // 2) - 1, passable=p)
        add("passable_per_env", m, 8, None, passable="per_env")
    rng = np.random.default_rng(H * 1000 + W)                                                               # (m)
    k = 11
    pts = np.stack([rng.integers(-2, W + 2, size=k), rng.integers(-2, H + 2, size=k), rng.integers(-1, 4, size=k)], axis=-1).astype(np.int32)
    pts[0] = (W - 1, H - 1, 1)
    pts[1] = pts[2] = (0, 0, 2)
    pts[3] = (0, 0, 0)
    pts[4] = (W, 0, 1)
    pts[5] = (0, -1, 1)
    m = np.zeros((H, W), dtype=np.uint8)
    m[0, 0] = B
    m[H // 2:, :] = D
    add("points", m, 8, None, points=pts)
    return [s for s in out if s is not None]


def per_env_passable(E, H, W):
    """uint8 [E, H, W]: environment e is cut by a closed column at x = 2 + e (mod W - 2)."""
    p = np.ones((E, H, W), dtype=np.uint8)
    for e in range(E):
        p[e, :, 2 + e % (W - 2)] = 0
    return p


def make_scene_world(H, W, diag):
    """(engine kwargs without n_envs, R table) for a grid of the scenes' shapes."""
    from test_env_state_gpu import _world
    rng = np.random.default_rng(9000 + H * 7 + W)
    kw, R8 = _world(rng, H, W, 4, False, diag)
    kw.update(max_time=None, update_rate=1.0)
    return kw, np.maximum(R8, 12.0)
