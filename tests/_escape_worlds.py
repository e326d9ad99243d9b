"""Hand-made scenes for ``sf_escape``.  Unless a scene says otherwise ``minutes`` holds integers,
``minutes_per_move`` is 1 and the margin 0, so a cell's deadline D is its ``minutes`` value read off directly; walls are FIRELINE
(3), walkable cells UNBURNED (0) and targets BURNED (2).  A scene is a dict: ``name``, ``map`` uint8 [H, W], ``minutes`` float32
[H, W], ``target`` / ``through`` (status names), ``conn``, ``passable`` / ``targets`` (uint8 [H, W] or None), ``points`` int32
[k, 3] = (column, row, id), ``per_move``, ``margin``, ``horizon``, ``flag`` (unreached_safe) and ``claim``: a function of the
oracle-shaped answer (a dict of ``slack``, ``point_slack``, ``point_step``, ``safe``, ``escapable``, ``lost``, ``top``) that asserts
what the scene is there to show, or None."""
import numpy as np

SAFE, LOST, BLOCKED = 2 ** 31 - 1, -1, -2
TARGET, THROUGH = ("BURNED",), ("UNBURNED",)
WALL, OPEN, GOAL = 3, 0, 2
SCENE_SHAPES = [(9, 9), (33, 17), (40, 130), (64, 64), (70, 1030)]
HORIZON = 64.0
INF = np.float32(np.inf)


def _scene(name, m, mins, points=None, conn=4, claim=None, **more):
    H, W = m.shape
    if points is None:
        points = default_points(H, W)
    s = dict(name=name, map=np.ascontiguousarray(m, dtype=np.uint8), minutes=np.ascontiguousarray(mins, dtype=np.float32), target=TARGET,
             through=THROUGH, conn=conn, passable=None, targets=None, points=np.asarray(points, dtype=np.int32).reshape(-1, 3), per_move=1.0,
             margin=0.0, horizon=HORIZON, flag=False, claim=claim)
    s.update(more)
    return s


def default_points(H, W, seed=0):
    """A fixed set of points: corners, a duplicate, padding (id 0), a negative id, off the grid on every side, and random cells."""
    rng = np.random.default_rng(3100 + seed)
    pts = [(0, 0, 1), (W - 1, H - 1, 2), (W - 1, 0, 3), (0, H - 1, 4), (1, 1, 5), (1, 1, 5), (2, 1, 0), (2, 1, -3), (-1, 0, 1), (W, 0, 1), (0, -1, 1),
           (0, H, 1)]
    pts += [(int(rng.integers(0, W)), int(rng.integers(0, H)), 7) for _ in range(12)]
    return np.array(pts, dtype=np.int32)


def _walls(H, W, fill=50.0):
    return np.full((H, W), WALL, dtype=np.uint8), np.full((H, W), fill, dtype=np.float32)


def corridors(H, W):
    """Row 1: a corridor of L cells, target at column 0, whose cell next to the target closes exactly in time for a walker at the far
    end (D = L: it is stood on at index L - 1); row 3: the same, one move too early (D = L - 1)."""
    L = min(W - 2, 6)
    m, t = _walls(H, W)
    for row, d in ((1, L), (3, L - 1)):
        m[row, 0] = GOAL
        m[row, 1:L + 1] = OPEN
        t[row, 1] = d
    pts = [(L, 1, 1), (L, 3, 1), (1, 1, 1), (1, 3, 1), (L - 1, 3, 1)]

    def claim(r):
        assert r["point_slack"].tolist() == [0, LOST, L - 1, L - 2, 0] and r["point_step"].tolist() == [3, 0, 3, 3, 3]
        assert r["slack"][1, L] == 0 and r["slack"][3, L] == LOST and r["slack"][3, L - 1] == 0 and r["lost"] == 1 and r["top"] == 50
    return _scene("corridors", m, t, pts, claim=claim)


def late_opener(H, W):
    """A cell with D = 3 beside a cell that joined the safe set at level 29: it opens at level 2, long after its neighbour was the
    front - a search that dilates only the last front never reaches it."""
    m, t = _walls(H, W, 30.0)
    m[1, 0] = GOAL
    m[1, 1:3] = OPEN
    m[2, 1] = OPEN
    t[2, 1] = 3

    def claim(r):
        assert r["slack"][1, 1] == 29 and r["slack"][1, 2] == 28 and r["slack"][2, 1] == 2 and r["escapable"] == 3 and r["top"] == 30
    return _scene("late_opener", m, t, [(1, 2, 1), (1, 1, 1)], claim=claim)


def never_pocket(H, W, flag):
    """Cells the fire never closes, walled in, no target among them: LOST without the flag, SAFE (targets) with it.  Beside them a
    NEVER cell reached only through a finite one: its slack is finite."""
    m, t = _walls(H, W, 5.0)
    m[1, 1:4] = OPEN
    t[1, 1:4] = INF
    m[5, 0] = GOAL
    m[5, 1:3] = OPEN
    t[5, 2] = INF

    def claim(r):
        assert (r["slack"][1, 1:4] == (SAFE if flag else LOST)).all() and r["slack"][5, 1] == 4
        assert r["slack"][5, 2] == (SAFE if flag else 3)
        assert (r["safe"], r["escapable"], r["lost"], r["top"]) == ((0, 1, 0, 5) if flag else (0, 2, 3, 5))
    return _scene("never_pocket_flag" if flag else "never_pocket", m, t, [(2, 1, 1), (2, 5, 1), (1, 5, 1)], claim=claim, flag=flag)


def closed_under_walker(H, W):
    """D = 0 under a walker next to a target: nobody may stand there even now.  Beside it a blocked cell with its own deadline."""
    m, t = _walls(H, W, 9.0)
    m[1, 0] = GOAL
    m[1, 1] = OPEN
    t[1, 1] = 0
    m[3, 0] = GOAL
    t[3, 1] = 4                               # a wall cell next to a target: a point on it has D = 4
    m[5, 0] = GOAL
    m[5, 1] = OPEN
    t[5, 1] = 7
    t[5, 2] = 3                               # a wall cell behind a walkable one: min(3 - 1, 6 - 1)
    t[6, 1] = INF

    def claim(r):
        assert r["slack"][1, 1] == LOST and r["slack"][3, 1] == BLOCKED and r["slack"][5, 1] == 6
        assert r["point_slack"].tolist() == [LOST, 3, 2, 5, SAFE] and r["point_step"].tolist() == [0, 3, 3, 1, 0]
    return _scene("closed_under_walker", m, t, [(1, 1, 1), (1, 3, 1), (2, 5, 1), (1, 6, 1), (0, 5, 9)], claim=claim)


def borders(H, W, kind):
    """An open field under random deadlines with the targets on every border (a targets plane, no status), without any target, with
    nothing walkable, or with one target walled in."""
    rng = np.random.default_rng(3110)
    m = np.zeros((H, W), dtype=np.uint8)
    t = rng.integers(0, 12, size=(H, W)).astype(np.float32)
    more, claim = {}, None
    if kind == "borders":
        tg = np.zeros((H, W), dtype=np.uint8)
        tg[0, :] = tg[H - 1, :] = 1
        tg[:, 0] = tg[:, W - 1] = 1
        more = dict(targets=tg, target=())

        def claim(r):
            assert (r["slack"][0] == SAFE).all() and (r["slack"][:, W - 1] == SAFE).all() and r["safe"] == 0
    elif kind == "no_target":
        def claim(r):
            assert (r["slack"] == LOST).all() and (r["safe"], r["escapable"], r["lost"]) == (0, 0, H * W) and (r["point_slack"][:6] == LOST).all()
    elif kind == "nothing_walkable":
        m[:] = WALL
        m[H // 2, W // 2] = GOAL

        def claim(r):
            assert (r["slack"] == BLOCKED).sum() == H * W - 1 and (r["safe"], r["escapable"], r["lost"], r["top"]) == (0, 0, 0, 0)
            assert (r["point_slack"][:6] == LOST).all() and (r["point_step"][:6] == 0).all()
    else:
        m[3:6, 3:6] = WALL
        m[4, 4] = GOAL

        def claim(r):
            assert r["slack"][4, 4] == SAFE and (r["slack"][m == OPEN] == LOST).all() and r["escapable"] == 0
    return _scene(kind, m, t, claim=claim, **more)


def crossings(H, W, conn):
    """Corridors that cross the word boundaries 63|64 and 127|128 and the band boundaries 15|16 and 31|32 (where the grid has them),
    one cell wide (the diagonals cut the corner by one move), and - with the diagonals - a diagonal step over a word and a band boundary at once."""
    m, t = _walls(H, W, 60.0)
    m[1, 0] = GOAL
    m[1, 1:W] = OPEN                           # along row 1 over every word boundary
    m[1:H, W - 1] = OPEN                       # down the last column over every band boundary
    if conn == 8 and H > 17 and W > 65:
        m[12:16, 63] = OPEN                    # (15, 63) and (16, 64) touch at a corner only
        m[16:20, 64] = OPEN
        m[1:13, 63] = OPEN
    t[m == OPEN] = 1500                        # (a horizon of 2048 moves: every cell of the longest corridor has a finite slack)

    def claim(r):
        assert r["slack"][1, W - 1] == 1500 - (W - 1) and r["slack"][H - 1, W - 1] == 1500 - (W - 1) - (H - 2) + (conn == 8) and r["lost"] == 0
        if conn == 8 and H > 17 and W > 65:
            assert r["slack"][16, 64] == r["slack"][15, 63] - 1 >= 0
    return _scene("crossings%d" % conn, m, t, conn=conn, claim=claim, horizon=2048.0)


def serpentine(H, W):
    """A snake through the grid, every cell with the same deadline: the slack falls by one per cell from the target."""
    m, t = _walls(H, W, 63.0)
    cols = min(W, 12)
    path = []
    for i, y in enumerate(range(0, H, 2)):
        xs = range(cols) if i % 2 == 0 else range(cols - 1, -1, -1)
        path += [(y, x) for x in xs]
        if y + 2 < H:
            path.append((y + 1, xs[-1]))
    path = path[:80]
    for y, x in path:
        m[y, x] = OPEN
    m[path[0]] = GOAL

    def claim(r):
        for d, (y, x) in enumerate(path[1:], 1):
            assert r["slack"][y, x] == (63 - d if d <= 63 else LOST), (d, y, x)
    return _scene("serpentine", m, t, [(x, y, 1) for y, x in path[:12]], claim=claim)


def four_way_tie(H, W):
    """A cross whose four arms end in targets at equal distance: the centre may go any way and takes the lowest move code; a walker
    on an arm goes on outwards."""
    m, t = _walls(H, W, 20.0)
    m[4, 1:8] = OPEN
    m[1:8, 4] = OPEN
    for y, x in ((4, 0), (4, 8), (0, 4), (8, 4)):
        m[y, x] = GOAL
    pts = [(4, 4, 1), (4, 3, 1), (4, 5, 1), (3, 4, 1), (5, 4, 1), (4, 1, 1)]

    def claim(r):
        assert r["point_slack"].tolist() == [16, 17, 17, 17, 17, 19] and r["point_step"].tolist() == [1, 1, 2, 3, 4, 1]
    return _scene("four_way_tie", m, t, pts, claim=claim)


def safe_tie(H, W):
    """Two neighbours with slack SAFE, one a target and one a NEVER cell that the flood reaches from a target of its own: the step
    goes to the LOWER move code whichever of the two that is - vertically and horizontally, in both orders.  And a NEVER neighbour
    with a lower number that the flood does not reach loses against the target."""
    m, t = _walls(H, W, 5.0)
    goals = [(1, 0), (3, 1), (5, 1), (7, 0), (1, 4), (2, 6), (6, 4), (7, 6), (4, 8)]
    never = [(1, 1), (7, 1), (2, 4), (6, 6), (4, 6)]          # above / below / left / right of a point, flooded; left, not flooded
    stand = [(2, 1), (6, 1), (2, 5), (6, 5), (4, 7)]          # the points' cells, D = 5: a target on the other side of each
    for y, x in goals:
        m[y, x] = GOAL
    for y, x in never + stand:
        m[y, x] = OPEN
    for y, x in never:
        t[y, x] = INF
    pts = [(1, 2, 1), (1, 6, 1), (5, 2, 1), (5, 6, 1), (7, 4, 1)]

    def claim(r):
        assert r["point_slack"].tolist() == [4, 4, 4, 4, 4] and r["point_step"].tolist() == [1, 1, 3, 3, 4]
        assert r["slack"][4, 6] == 3 and (r["safe"], r["escapable"], r["lost"], r["top"]) == (4, 6, 0, 5)
    return _scene("safe_tie", m, t, pts, claim=claim)


def odd_minutes(H, W, conn):
    """An open field whose closing times mix integers with +inf, NaN, -1 and the horizon itself (all NEVER), a few walls, and a
    passable plane: nothing is claimed but equality with the oracle."""
    rng = np.random.default_rng(3120 + conn)
    u = rng.random((H, W))
    m = np.where(u < 0.15, WALL, np.where(u < 0.17, GOAL, OPEN)).astype(np.uint8)
    t = rng.integers(0, 40, size=(H, W)).astype(np.float32)
    kind = rng.random((H, W))
    t[kind < 0.05] = INF
    t[(kind >= 0.05) & (kind < 0.10)] = np.nan
    t[(kind >= 0.10) & (kind < 0.15)] = -1.0
    t[(kind >= 0.15) & (kind < 0.20)] = HORIZON
    pas = (rng.random((H, W)) < 0.95).astype(np.uint8)
    return _scene("odd_minutes%d" % conn, m, t, conn=conn, passable=pas)


def fractions(H, W):
    """The ceil: T = 2.5 with a margin of 0.5 is two moves away exactly (D = 2); float32(0.3) / 0.1 is a hair above 3 (D = 4)."""
    m, t = _walls(H, W, 9.0)
    m[1, 0] = GOAL
    m[1, 1] = OPEN
    t[1, 1] = 2.5
    def claim_margin(r):
        assert (r["slack"][1, 1], r["top"], r["point_slack"].tolist()) == (1, 2, [1])

    def claim_quotient(r):
        assert (r["slack"][1, 1], r["top"], r["point_slack"].tolist()) == (3, 4, [3])
    t2 = t.copy()
    t2[1, 1] = np.float32(0.3)
    return [_scene("fraction_margin", m, t, [(1, 1, 1)], margin=0.5, claim=claim_margin),
            _scene("fraction_quotient", m, t2, [(1, 1, 1)], per_move=0.1, horizon=6.0, claim=claim_quotient)]


def scenes(H, W):
    """Every scene that fits an H x W grid (the hand-made ones need 9 x 9)."""
    out = [corridors(H, W), late_opener(H, W), never_pocket(H, W, False), never_pocket(H, W, True), closed_under_walker(H, W)]
    out += [borders(H, W, k) for k in ("borders", "no_target", "nothing_walkable", "enclosed_target")]
    out += [crossings(H, W, 4), crossings(H, W, 8), serpentine(H, W), four_way_tie(H, W), safe_tie(H, W), odd_minutes(H, W, 4), odd_minutes(H, W, 8)]
    out += fractions(H, W)
    return out


def per_env_targets(E, H, W, seed=3130):
    """uint8 [E, H, W]: a few target cells per environment."""
    rng = np.random.default_rng(seed)
    return (rng.random((E, H, W)) < 0.01).astype(np.uint8)
