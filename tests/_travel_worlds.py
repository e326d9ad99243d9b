"""Hand-made worlds for ``sf_travel``: a fire map, an R table and a request per scene, and what the scene claims
about the answer.  Shared by ``tests/test_travel_cpu.py`` (the oracle alone) and ``tests/test_travel_gpu.py`` (the engine against it).
The shapes cross every boundary the kernel has: one partial tile (9 x 9), W % 4 != 0 (33 x 17), several tile columns (40 x 130), whole
tiles (64 x 64) and more than 32 tile columns, so that the tile bitmap has several words (70 x 1030)."""
import numpy as np

import _reach_worlds as rw

U, B, D, FL, SL, WL = 0, 1, 2, 3, 4, 5
SCENE_SHAPES = ((9, 9), (33, 17), (40, 130), (64, 64), (70, 1030))
PIXEL_SCALE = 30.0
RATES = (3.0, 7.5, 12.0, 30.0, 400.0, 1200.0)
EVERY = ("UNBURNED", "BURNING", "BURNED", "FIRELINE", "SCRATCHLINE", "WETLINE")
# (source, through): the default, lines passable, two pairs that overlap
MASK_PAIRS = ((("BURNING",), ("UNBURNED",)),
              (("BURNING", "BURNED"), ("UNBURNED", "FIRELINE", "SCRATCHLINE", "WETLINE")),
              (("BURNING",), ("UNBURNED", "BURNING", "BURNED")),
              (("BURNING", "FIRELINE"), EVERY))


def engine_kwargs(H, W, diag=True, update_rate=1.0, md=4):
    return dict(shape=(H, W), max_fire_duration=md, pixel_scale=PIXEL_SCALE, update_rate=update_rate, max_time=None,
                attenuate_line_ros=False, diagonal_spread=diag)


def random_rates(rng, H, W, dead=0.1, holes=0.05):
    """float64 [8, H, W]: rates from ``RATES``, a share ``dead`` of cells unburnable (all eight 0) and ``holes`` of single entries 0."""
    R8 = rng.choice(RATES, size=(8, H, W))
    R8[rng.random((8, H, W)) < holes] = 0.0
    R8[:, rng.random((H, W)) < dead] = 0.0
    return R8


def random_map(rng, H, W, lines=0.1, fires=3):
    m = np.where(rng.random((H, W)) < lines, rng.integers(3, 6, size=(H, W)), U).astype(np.uint8)
    m[rng.random((H, W)) < 0.02] = D
    for _ in range(fires):
        m[rng.integers(H), rng.integers(W)] = B
    return m


def corridor(H, W, length):
    """A corridor of ``length`` unburned cells along row 2, from column 2 on, walled in by fireline; the fire stands at its head
    (1, 2).  With a uniform table of rate R the cell j cells along is reached after the j-fold float32 sum of w."""
    m = np.full((H, W), FL, dtype=np.uint8)
    m[2, 1] = B
    m[2, 2:2 + length] = U
    return m


def fold(w, n):
    """The n-fold float32 sum 0 + w + w + ... in path order."""
    t, w = np.float32(0.0), np.float32(w)
    for _ in range(n):
        t = t + w
    return t


def default_points(H, W, seed=0, k=12):
    """int32 [k, 3]: random points, some off the grid or padding (id <= 0), a duplicate pair, the corners."""
    rng = np.random.default_rng(4100 + seed)
    pts = np.stack([rng.integers(-2, W + 2, size=k), rng.integers(-2, H + 2, size=k), rng.integers(-1, 4, size=k)], axis=-1).astype(np.int32)
    pts[0] = (W - 1, H - 1, 1)
    pts[1] = pts[2] = (W // 2, H // 2, 2)
    pts[3] = (0, 0, 0)
    pts[4] = (W, 0, 1)
    pts[5] = (0, -1, 1)
    return pts


def per_env_sources(E, H, W):
    """uint8 [E, H, W]: environment e starts from the cell (e mod H, (3 e) mod W) - and a second one in the far corner."""
    s = np.zeros((E, H, W), dtype=np.uint8)
    for e in range(E):
        s[e, e % H, (3 * e) % W] = 1 + e % 200
        s[e, H - 1, W - 1 - e % W] = 255
    return s


def scenes(H, W):
    """[dict(name, map, R8, source, through, conn, passable, sources, points, max_minutes, claim)] for an H x W grid.  ``passable`` /
    ``sources``: None, a plane [H, W], or "per_env"; ``claim(answer)``: what the scene asserts about an oracle-shaped answer (a dict
    with minutes, pred, reached, last, point_minutes), or None - equality with the oracle is always claimed."""
    rng = np.random.default_rng(H * 1000 + W + 26)
    burning, unburned = ("BURNING",), ("UNBURNED",)
    out = []
    uniform = np.full((8, H, W), 12.0)
    w12 = np.float32(PIXEL_SCALE / 12.0)

    def add(name, m, R8, conn=8, source=burning, through=unburned, passable=None, sources=None, points=None, max_minutes=0.0, claim=None):
        out.append(dict(name=name, map=np.ascontiguousarray(m, dtype=np.uint8), R8=np.ascontiguousarray(R8, dtype=np.float64), source=source,
                        through=through, conn=conn, passable=passable, sources=sources,
                        points=default_points(H, W, len(out)) if points is None else points, max_minutes=max_minutes, claim=claim))

    # (a) random worlds: every mask pair, the three connectivities
    for i, (src, thr) in enumerate(MASK_PAIRS):
        add("random_%d" % i, random_map(rng, H, W), random_rates(rng, H, W), conn=(8, 4, 0, 8)[i], source=src, through=thr)
    # (b) corridors that cross tile borders again and again
    if (H, W) in ((33, 17), (40, 130), (70, 1030)):
        for vertical in (False, True):
            m = rw._serpentine(H, W, vertical)
            add("serpentine_%s" % ("v" if vertical else "h"), m, random_rates(rng, H, W, dead=0.0, holes=0.0), conn=4,
                claim=lambda a, n=int((m == U).sum()): _is(a["reached"], n))
    if W > 100 and H >= 40:
        m = rw._spiral(H, W)
        add("spiral", m, random_rates(rng, H, W, dead=0.0, holes=0.0), conn=4, claim=lambda a, n=int((m == U).sum()): _is(a["reached"], n))
    # (c) a fast strip beside a slow field: the best route to the far cells of the first rows leaves their tile and comes back
    if H >= 9 and W >= 9:
        R8 = np.full((8, H, W), 3.0)
        ys = min(33, H - 2)
        R8[:, ys, :] = 1200.0
        m = np.zeros((H, W), dtype=np.uint8)
        m[1, 1] = B

        def strip_claim(a, ys=ys):
            far = a["minutes"][1, W - 2]
            direct = fold(PIXEL_SCALE / 3.0, W - 3)
            assert far < direct and a["pred"][1, W - 2] in (0, 1, 2)       # it comes up from the strip's side, not along the row
        add("fast_strip", m, R8, conn=8, claim=strip_claim if W > 2 * ys + 8 else None)
    # (d) unburnable blocks
    R8 = random_rates(rng, H, W, dead=0.0)
    for _ in range(max(2, H * W // 400)):
        y, x = int(rng.integers(H)), int(rng.integers(W))
        R8[:, y:y + 5, x:x + 7] = 0.0
    m = np.zeros((H, W), dtype=np.uint8)
    m[H // 2, W // 2] = B
    m[0, 0] = B

    def dead_claim(a, dead=(R8.sum(axis=0) == 0.0), m=m):
        assert np.isinf(a["minutes"][dead & (m == U)]).all() and (a["pred"][dead] == -1).all()
    add("unburnable_blocks", m, R8, conn=8, claim=dead_claim)
    # (e) a cell that can be entered from one direction only (from below: k = 1), behind a ring of cells that cannot be entered at all
    if H >= 9 and W >= 9:
        R8 = uniform.copy()
        cy, cx = H // 2, W // 2
        R8[:, cy - 1:cy + 2, cx - 1:cx + 2] = 0.0
        R8[:, cy + 1, cx] = 12.0                       # the gate below the cell is open from every side
        R8[1, cy, cx] = 30.0                           # the cell itself: from (cy + 1, cx) only
        m = np.zeros((H, W), dtype=np.uint8)
        m[0, 0] = B

        def gate_claim(a, cy=cy, cx=cx):
            assert a["pred"][cy, cx] == 1 and a["minutes"][cy, cx] == a["minutes"][cy + 1, cx] + np.float32(PIXEL_SCALE / 30.0)
            assert np.isinf(a["minutes"][cy - 1, cx - 1:cx + 2]).all()
        add("one_way", m, R8, conn=8, claim=gate_claim)
    # (f) a wall whose only gaps lie at rows / columns 31 | 32: the fire crosses exactly where four tiles meet
    if H >= 64 and W >= 64:
        m = np.zeros((H, W), dtype=np.uint8)
        m[:, 31] = FL
        m[:, 32] = FL
        m[31, 31] = U
        m[32, 32] = U
        m[5, 5] = B
        add("corner_gap_8", m, random_rates(rng, H, W, dead=0.0, holes=0.0), conn=8,
            claim=lambda a: _is(bool(np.isfinite(a["minutes"][32, 32]) and a["pred"][32, 32] == 7 and np.isfinite(a["minutes"][5, W - 1])), True))
        add("corner_gap_4", m, random_rates(rng, H, W, dead=0.0, holes=0.0), conn=4,
            claim=lambda a: _is(bool(np.isinf(a["minutes"][32, 32]) and np.isinf(a["minutes"][5, W - 1])), True))
        m2 = m.copy()
        m2[32, 31] = U                                  # now a way for the four moves too: through (31, 31), (32, 31), (32, 32)
        add("border_gap_4", m2, random_rates(rng, H, W, dead=0.0, holes=0.0), conn=4,
            claim=lambda a: _is(bool(np.isfinite(a["minutes"][5, W - 1]) and a["pred"][32, 32] == 4), True))
        # sources ON a tile border whose neighbours beyond it are all that the tile beyond holds: nothing but the source wakes that tile
        m = np.full((H, W), FL, dtype=np.uint8)
        m[5, 32] = m[32, 40] = m[32, 32] = B
        m[5, 20:32] = U                                 # to the left of (5, 32)
        m[20:32, 40] = U                                # above (32, 40)
        m[31, 31] = U                                   # the corner cell of (32, 32)
        m[50, 31] = B
        m[50, 32:44] = U                                # to the right of (50, 31)
        add("source_on_a_tile_border", m, uniform, conn=8,
            claim=lambda a: _is((a["reached"], float(a["minutes"][5, 20]), float(a["minutes"][31, 31]), float(a["minutes"][50, 43])),
                                (12 + 12 + 1 + 12, float(fold(w12, 12)), float(w12), float(fold(w12, 12)))))
    # (g) planes: shared and per environment, with and without a source mask
    m = np.zeros((H, W), dtype=np.uint8)
    m[H - 1, 0] = B
    s = np.zeros((H, W), dtype=np.uint8)
    s[0, W - 1] = 7
    p = np.full((H, W), 200, dtype=np.uint8)
    p[:, W // 2] = 0
    p[H // 2, W // 2] = 1
    add("sources_shared", m, random_rates(rng, H, W), source=None, sources=s,
        claim=lambda a: _is((float(a["minutes"][0, W - 1]), float(a["minutes"][H - 1, 0]), int(a["pred"][0, W - 1])), (0.0, -1.0, -1)))
    add("sources_and_mask", m, random_rates(rng, H, W), sources=s,
        claim=lambda a: _is((float(a["minutes"][0, W - 1]), float(a["minutes"][H - 1, 0])), (0.0, 0.0)))
    add("passable_shared", m, uniform, passable=p, conn=4,
        claim=lambda a: _is(bool((a["minutes"][:, W // 2] == -1).sum() == H - 1 and a["minutes"][H // 2, W // 2] > 0), True))
    add("sources_per_env", m, random_rates(rng, H, W), source=None, sources="per_env")
    add("both_per_env", m, random_rates(rng, H, W), source=None, sources="per_env", passable="per_env", through=EVERY)
    # (h) nothing to do
    add("no_source", np.zeros((H, W), dtype=np.uint8), uniform,
        claim=lambda a: _is((a["reached"], float(a["last"]), bool(np.isinf(a["minutes"]).all()), bool((a["pred"] == -1).all())), (0, 0.0, True, True)))
    if H >= 5 and W >= 5:
        m = np.zeros((H, W), dtype=np.uint8)
        m[H // 2 - 1:H // 2 + 2, W // 2 - 1:W // 2 + 2] = WL
        m[H // 2, W // 2] = B
        add("walled_in", m, uniform, claim=lambda a: _is((a["reached"], int(np.isinf(a["minutes"]).sum())), (0, H * W - 9)))
    # (i) points on every kind of cell, and a cap
    m = np.zeros((H, W), dtype=np.uint8)
    m[0, 0] = B
    m[H // 2, :] = SL
    m[H // 2, W - 1] = U
    pts = default_points(H, W, 99)
    pts[6] = (W // 2, H // 2, 1)                        # on the line
    pts[7] = (0, 0, 1)                                  # on the source
    pts[8] = (W // 2, H - 1, 1)                         # beyond the line

    def line_claim(a, cap=0.0):
        pm = a["point_minutes"]
        assert pm[3] == -1 and pm[4] == -1 and pm[5] == -1 and pm[1] == pm[2] and pm[7] == 0
        assert pm[6] == a["minutes"][H // 2 - 1, W // 2 - 1:W // 2 + 2].min() + w12 or (cap and pm[6] == np.float32(cap))
        assert a["minutes"][H // 2, W // 2] == -1
    add("points_on_the_line", m, uniform, points=pts, claim=line_claim)
    cap = float(fold(w12, max(2, min(H, W) // 3)))
    add("points_capped", m, uniform, points=pts, max_minutes=cap,
        claim=lambda a: (line_claim(a, cap), _is(float(a["minutes"].max()), float(np.float32(cap))), _is(float(a["last"]), float(np.float32(cap)))))
    return out


def _is(got, want):
    assert got == want, (got, want)


def planes_of(s, e, E, H, W):
    """(passable, sources) of scene ``s`` living in environment ``e`` of ``E``: the plane that environment reads, or None."""
    pas = rw.per_env_passable(E, H, W)[e] if isinstance(s["passable"], str) else s["passable"]
    src = per_env_sources(E, H, W)[e] if isinstance(s["sources"], str) else s["sources"]
    return pas, src
