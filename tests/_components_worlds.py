"""The scenes of ``tests/test_components_cpu.py`` and ``tests/test_components_gpu.py``: hand-made maps at the shapes of
``_reach_worlds`` (9 x 9 and 33 x 17: no full word; 64 x 64: exact words; 40 x 130: runs across a word boundary; 70 x 1030: a row scan
over many words with a ragged end), each with the claim it makes.  The corridors, the ring and the points are ``_reach_worlds``'."""
import numpy as np

import _reach_worlds as rw

U, B, D, FL, SL, WL = rw.U, rw.B, rw.D, rw.FL, rw.SL, rw.WL
SHAPES = rw.SCENE_SHAPES
OPEN = ("UNBURNED", "BURNING")
CAP = 64


def scenes(H, W):
    """[dict(name, map, select, conn, member, points, count, claim)]: ``count`` is the number of components the scene claims (None:
    only equality with the oracle), ``claim`` a function of the oracle-shaped result that asserts what else the scene says;
    ``member``: None, a plane, or "per_env"."""
    out = []

    def add(name, m, select, conn, count=None, member=None, points=None, claim=None):
        out.append(dict(name="%s_%d" % (name, conn), map=np.ascontiguousarray(m, dtype=np.uint8), select=select, conn=conn, member=member,
                        points=points, count=count, claim=claim))

    def nothing(r):
        assert r["largest"].tolist() == [0, 0] and (r["first"] == -1).all() and (r["bbox"] == -1).all() and not r["cells"].any()

    def whole(r):
        assert int(r["touch"][0]) == 64 and r["largest"].tolist() == [1, H * W] and r["bbox"][0].tolist() == [0, 0, W - 1, H - 1]

    zeros = np.zeros((H, W), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for conn in (4, 8):
        add("empty_selection", zeros, ("BURNING",), conn, 0, claim=nothing)
        add("everything_selected", zeros, ("UNBURNED",), conn, 1, claim=whole)
        board = np.where((yy + xx) % 2 == 0, B, U).astype(np.uint8)                    # far above the cap without diagonals
        add("checkerboard", board, ("BURNING",), conn, (H * W + 1) // 2 if conn == 4 else 1)
        for vertical in (False, True):                                                 # long union chains
            add("serpentine_%s" % ("v" if vertical else "h"), rw._serpentine(H, W, vertical), OPEN, conn, 1)
        if min(H, W) >= 9:
            add("spiral", rw._spiral(H, W), OPEN, conn, 1)
        comb = np.full((H, W), FL, dtype=np.uint8)                                     # numbers collapse in the last row only
        comb[:, ::2] = U
        comb[H - 1, :] = U
        add("comb", comb, ("UNBURNED",), conn, 1)
        up = comb[::-1].copy()                                                         # the same with the joining row first
        add("comb_upside_down", up, ("UNBURNED",), conn, 1)
        if W >= 130 and H >= 30:                                                       # walls at the word boundaries, one gap each
            for name, g64, g128 in (("gaps_a", ("h", 10), ("d", 21)), ("gaps_b", ("d", 12), ("h", 7)), ("gaps_c", ("u", 13), ("h", 8))):
                m = zeros.copy()
                for col, (kind, row) in ((63, g64), (127, g128)):
                    m[:, col] = FL
                    m[:, col + 1] = FL
                    m[row, col] = U
                    m[row + {"h": 0, "d": 1, "u": -1}[kind], col + 1] = U
                m[5, 5] = B
                add(name, m, OPEN, conn, 2 if conn == 4 else 1)                        # the diagonal gap joins only with diagonals
        if H >= 5:                                                                     # the only way round is the padding
            wall = zeros.copy()
            wall[H // 2, :] = FL
            wall[0, W - 1] = B
            add("wall_to_the_last_column", wall, OPEN, conn, 2)
        m = zeros.copy()
        m[1, 1] = m[2, 2] = m[2, 3] = m[3, 4] = B
        m[H - 2, W - 1] = m[H - 1, W - 2] = B                                          # and at the far corner
        add("diagonal_touch", m, ("BURNING",), conn, 5 if conn == 4 else 2)
        ring, inside, _ = rw._ring(H, W, True)                                         # the hole sees the ring and nothing else

        def hole(r, inside=inside):
            assert int(r["touch"][1]) == 1 << FL and int(r["cells"][1]) == inside + 1 and int(r["touch"][0]) == 64 | 1 << FL
        add("ring", ring, OPEN, conn, 2, claim=hole)
        rng = np.random.default_rng(H * 1000 + W)                                      # points: scene (m) of _reach_worlds
        k = 11
        pts = np.stack([rng.integers(-2, W + 2, size=k), rng.integers(-2, H + 2, size=k), rng.integers(-1, 4, size=k)], axis=-1).astype(np.int32)
        pts[0] = (W - 1, H - 1, 1)
        pts[1] = pts[2] = (0, 0, 2)
        pts[3] = (0, 0, 0)
        pts[4] = (W, 0, 1)
        pts[5] = (0, -1, 1)
        m = zeros.copy()
        m[0, 1] = B
        m[H // 2:, :] = D
        m[H // 2, ::3] = U

        def pointed(r):
            assert r["point_label"][:6].tolist() == [0, 1, 1, -1, -1, -1]
        add("points", m, ("UNBURNED",), conn, points=pts, claim=pointed)
        member = np.full((H, W), 200, dtype=np.uint8)
        member[:, W // 2] = 0
        add("member_shared", zeros, ("UNBURNED",), conn, 2, member=member)
        add("member_per_env", zeros, ("UNBURNED",), conn, None, member="per_env")
        u = rng.random((H, W))                                                         # every status, every touch bit
        mixed = np.select([u < 0.45, u < 0.6, u < 0.7, u < 0.8, u < 0.9], [U, B, D, FL, SL], WL).astype(np.uint8)
        add("mixed", mixed, ("UNBURNED", "BURNED"), conn)
    return out


def variant(m, j):
    """The map environment j of a scene's handle holds: the scene's own (j = 0, 2, 3) or its mirror image (j = 1)."""
    return np.ascontiguousarray(m[:, ::-1]) if j == 1 else m


per_env_member = rw.per_env_passable
make_scene_world = rw.make_scene_world
