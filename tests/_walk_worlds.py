"""The scenes of ``tests/test_walk_gpu.py`` / ``tests/test_walk_cpu.py`` (``sf_walk``).  Most shapes come from
``_reach_worlds`` (serpentines, the spiral, the seam gaps, the wall to the last column, the borders): what was a seed there is a
target here, what was open is walkable.  The episode loops are ``_reach_worlds.run_episode`` with the mask pairs below."""
import numpy as np

import _reach_worlds as rw
import _walk_oracle as wo

U, B, D, FL, SL, WL = rw.U, rw.B, rw.D, rw.FL, rw.SL, rw.WL
SCENE_SHAPES = ((9, 9), (33, 17), (40, 130), (64, 64), (70, 1030))
EVERY = ("UNBURNED", "BURNING", "BURNED", "FIRELINE", "SCRATCHLINE", "WETLINE")
# (target, through): they may overlap
MASK_PAIRS = ((("BURNING",), ("UNBURNED",)),
              (("BURNING", "BURNED"), ("UNBURNED", "FIRELINE", "SCRATCHLINE", "WETLINE")),
              (("FIRELINE", "SCRATCHLINE", "WETLINE"), ("UNBURNED", "BURNED")),
              (("BURNING",), ("UNBURNED", "BURNING", "BURNED")))
CONNS = (4, 8, 4)


def queries(case, mode):
    """[(updates of the call, target names, through names, connectivity)] - the calls of ``_reach_worlds.queries`` with this
    feature's pairs and connectivities."""
    return [(n,) + MASK_PAIRS[(i + j) % 4] + (CONNS[(i + 2 * j) % 3],)
            for j in [rw.aw.CASES[case]["modes"].index(mode)] for i, n in enumerate(rw.CALLS)]


def run_episode(case, mode, h, inits, on_query, H, W):
    h.reset(inits)
    for i, (n, tgt, thr, conn) in enumerate(queries(case, mode)):
        h.step(n)
        on_query(i, n, tgt, thr, conn)
        if rw.draws_lines(case, mode) and i in (1, 2, 4):
            h.apply_mitigation(rw.line_rows(i, h.n_envs, H, W, inits))


def default_points(H, W, seed=0, k=13):
    """[k, 3] = (column, row, id): random cells, some off the grid, padding ids, a duplicate, the four corners."""
    rng = np.random.default_rng(H * 1000 + W + seed)
    pts = np.stack([rng.integers(-1, W + 1, size=k), rng.integers(-1, H + 1, size=k), rng.integers(0, 4, size=k)], axis=-1).astype(np.int32)
    pts[0] = (W - 1, H - 1, 1)
    pts[1] = pts[2] = (0, 0, 2)
    pts[3] = (0, 0, 0)
    pts[4] = (W, 0, 1)
    pts[5] = (0, -1, 1)
    pts[6] = (W - 1, 0, 5)
    pts[7] = (0, H - 1, 5)
    return pts


def per_env_targets(E, H, W):
    """uint8 [E, H, W]: environment e has one target cell of its own."""
    t = np.zeros((E, H, W), dtype=np.uint8)
    for e in range(E):
        t[e, (5 * e + 1) % H, (3 * e + 2) % W] = 1 + e % 200
    return t


def scenes(H, W):
    """[dict(name, map, target, through, conn, passable, targets, points, claim)].  ``passable`` / ``targets``: None, a plane, or
    "per_env" (``_reach_worlds.per_env_passable`` / ``per_env_targets``, indexed by the scene's environment number).  ``claim``: None
    or a function (moves plane, point_moves, point_step, reached, levels) -> None that asserts what the scene is there for."""
    out = []

    def add(name, m, conn=4, target=("BURNING",), through=("UNBURNED",), passable=None, targets=None, points=None, claim=None):
        out.append(dict(name=name, map=np.ascontiguousarray(m, dtype=np.uint8), target=target, through=through, conn=conn, passable=passable,
                        targets=targets, points=default_points(H, W, len(out)) if points is None else np.asarray(points, dtype=np.int32),
                        claim=claim))
    for s in rw.scenes(H, W):                       # serpentines, spirals, diagonals, rings, column seams, the wall, borders, ...
        claim = None
        if s["name"] == "serpentine_h_4":
            def claim(mv, pm, ps, reached, levels, n=int((s["map"] == U).sum())):
                assert levels == n == reached and mv.max() == n, (levels, n, reached)        # the corridor is the path
        if s["name"].startswith("wall_to_the_last_column"):
            def claim(mv, pm, ps, reached, levels):
                assert (mv[H // 2 + 1:] == wo.FAR).all() and (mv[:H // 2] < wo.FAR).all() and (mv[H // 2] == wo.BLOCKED).all()
        if s["name"] == "no_seed":
            def claim(mv, pm, ps, reached, levels):
                assert (mv == wo.FAR).all() and reached == 0 and levels == 0 and set(pm.tolist()) <= {-1, wo.FAR} and set(ps.tolist()) <= {-1, 0}
        if s["name"] == "nothing_open":
            def claim(mv, pm, ps, reached, levels):
                assert set(np.unique(mv).tolist()) == {wo.BLOCKED, 0} and reached == 0 and levels == 0
        if s["name"] == "borders":
            def claim(mv, pm, ps, reached, levels):
                assert mv.min() == 0 and mv.max() < wo.FAR and reached == H * W - 8
        add(s["name"], s["map"], s["conn"], s["source"], s["through"], s["passable"], None, s["points"], claim)
    if H >= 34:                                     # gaps exactly at the band seams: rows 15|16 and 31|32
        m = np.zeros((H, W), dtype=np.uint8)
        for row, col in ((15, 2), (31, W - 3)):
            m[row, :] = FL
            m[row + 1, :] = WL
            m[row, col] = m[row + 1, col] = U
        m[0, 0] = B

        def claim(mv, pm, ps, reached, levels):
            assert mv[16, 2] == 2 + 16 and mv[32, W - 3] == mv[16, 2] + (W - 5) + 16 and reached == H * W - 1 - 4 * W + 4
        add("row_seams_4", m, 4, claim=claim)
        add("row_seams_8", m, 8)
    cy, cx = H // 2, W // 2
    m = np.zeros((H, W), dtype=np.uint8)            # a target enclosed by blocked cells: nothing gets to it
    m[cy - 1:cy + 2, cx - 1:cx + 2] = SL
    m[cy, cx] = B

    def claim(mv, pm, ps, reached, levels):
        assert reached == 0 and levels == 0 and mv[cy, cx] == 0 and (mv[mv > 0] == wo.FAR).all() and pm[1] == wo.FAR and pm[0] == 1 and ps[0] == 2
    add("enclosed_target", m, 4, points=[(cx, cy - 1, 1), (cx, cy - 2, 1), (cx, cy, 1)], claim=claim)
    m = np.zeros((H, W), dtype=np.uint8)            # a four-way tie round a single target
    m[cy, cx] = B
    ring = [(cx, cy - 1), (cx, cy + 1), (cx - 1, cy), (cx + 1, cy), (cx - 1, cy - 1), (cx + 1, cy - 1), (cx - 1, cy + 1), (cx + 1, cy + 1), (cx, cy)]

    def claim(mv, pm, ps, reached, levels):
        assert pm.tolist() == [1, 1, 1, 1, 2, 2, 2, 2, 0] and ps.tolist() == [2, 1, 4, 3, 2, 2, 1, 1, 0], (pm, ps)
    add("tie", m, 4, points=[(x, y, 1) for x, y in ring], claim=claim)
    m = np.full((H, W), FL, dtype=np.uint8)         # a corridor through lines; walkers on the line beside it, and one cell further off
    m[cy, 1:W - 1] = U
    m[cy, 1] = B

    def claim(mv, pm, ps, reached, levels):
        assert reached == levels == W - 3 and pm.tolist() == [1 + 3, 1 + 3, wo.FAR, 1, 0, W - 3 + 1, -1] and ps.tolist() == [2, 1, 0, 2, 0, 3, -1], (pm, ps)
    add("on_the_line", m, 4, points=[(4, cy - 1, 1), (4, cy + 1, 2), (4, cy - 2, 1), (1, cy - 1, 1), (1, cy, 1), (W - 1, cy, 9), (4, cy, 0)], claim=claim)
    rng = np.random.default_rng(77 + H * W)         # a targets plane, target_mask = 0, every status walkable: the fire does not matter
    m = rng.integers(0, 6, size=(H, W)).astype(np.uint8)
    t = np.zeros((H, W), dtype=np.uint8)
    t[H - 1, W - 1] = 255

    def claim(mv, pm, ps, reached, levels):
        assert levels == H + W - 2 == mv[0, 0] and reached == H * W - 1
    add("targets_shared", m, 4, target=None, through=EVERY, targets=t, claim=claim)
    p = (rng.random((H, W)) < 0.8).astype(np.uint8) * 7
    add("targets_and_passable", m, 8, target=None, through=EVERY, targets=t, passable=p)
    add("targets_per_env", m, 4, target=("BURNING",), through=("UNBURNED", "BURNED", "FIRELINE"), targets="per_env")
    add("both_per_env", m, 4, target=None, through=EVERY, targets="per_env", passable="per_env")
    add("masks_overlap", m, 8, target=("BURNING", "WETLINE"), through=("UNBURNED", "BURNING", "BURNED"))
    return out


def planes_of(s, e, E, H, W):
    """(passable, targets) of scene ``s`` in environment ``e`` as host planes or None."""
    pas = rw.per_env_passable(E, H, W)[e] if isinstance(s["passable"], str) else s["passable"]
    tgt = per_env_targets(E, H, W)[e] if isinstance(s["targets"], str) else s["targets"]
    return pas, tgt


def corridor(H, W, length):
    """A map of lines with one straight corridor of ``length`` walkable cells in row 2 that starts right of a BURNING cell at
    column 1: cell (2, 1 + j) is j moves away."""
    m = np.full((H, W), FL, dtype=np.uint8)
    m[2, 1] = B
    m[2, 2:2 + length] = U
    return m
