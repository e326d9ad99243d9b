"""Walking distance without a device (``sf_walk``): the NumPy oracle against scipy's shortest paths, what the
hand-made scenes of ``tests/_walk_worlds.py`` claim, the ABI as the header and the binding state it, and the Python argument errors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _reach_oracle as ro
import _walk_oracle as wo
import _walk_worlds as ww

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- 1. the oracle
def _random_map(rng, H, W, lines):
    u = rng.random((H, W))
    m = np.where(u < lines, rng.integers(3, 6, size=(H, W)), 0)
    m = np.where((u >= lines) & (u < lines + 0.01), 1, m)
    m = np.where((u >= lines + 0.01) & (u < lines + 0.04), 2, m)
    return m.astype(np.uint8)


def test_oracle_equals_scipy_shortest_paths():
    """A directed graph with an edge a -> b of weight 1 for neighbours a, b with b a target or walkable, searched from every target
    at once over the reversed edges (``a`` may be any cell: that is the point rule; on walkable cells it is the plane)."""
    sp = pytest.importorskip("scipy.sparse")
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    rng = np.random.default_rng(2401)
    H, W = 24, 40
    seen_far = seen_near = 0
    for lines in (0.1, 0.3, 0.45):
        for tgt, thr in ((2, 1), (2 | 4, 1 | 56), (8, 1 | 4), (2, 1 | 2)):
            for conn in (4, 8):
                m = _random_map(rng, H, W, lines)
                target, walk = wo.cells(m, tgt, thr)
                ok = target | walk
                idx = np.arange(H * W).reshape(H, W)
                rows, cols = [], []
                for dy, dx in wo.MOVES + (wo.DIAGONALS if conn == 8 else ()):
                    ys, xs = np.mgrid[max(0, -dy):H - max(0, dy), max(0, -dx):W - max(0, dx)]
                    into = ok[ys + dy, xs + dx]
                    rows.append(idx[ys, xs][into])
                    cols.append(idx[ys + dy, xs + dx][into])
                rows, cols = np.concatenate(rows), np.concatenate(cols)
                # reversed, so that one search from all targets gives every cell's distance TO a target.  An edge a -> b exists only
                # where b may be entered, so the search never continues through a cell that is neither a target nor walkable - but it
                # ends on one: dist is the point rule for every cell, and the plane on the walkable ones
                g = sp.csr_matrix((np.ones(len(rows)), (cols, rows)), shape=(H * W, H * W))
                if target.any():
                    dist = csgraph.dijkstra(g, directed=True, indices=np.flatnonzero(target), unweighted=True, min_only=True).reshape(H, W)
                else:
                    dist = np.full((H, W), np.inf)
                d, L = wo.true_moves(m, tgt, thr, conn)
                want = np.where(target, 0, np.where(walk, np.where(np.isinf(dist), wo.FAR, dist), wo.BLOCKED)).astype(np.int64)
                assert (d == want).all(), (lines, tgt, thr, conn)
                assert L == int(dist[walk & np.isfinite(dist)].max(initial=0))
                pts = np.stack([idx % W, idx // W, np.ones_like(idx)], axis=-1).reshape(-1, 3)
                pm, ps = wo.points_of(d, pts, conn)
                assert (pm == np.where(np.isinf(dist), wo.FAR, dist).astype(np.int64).ravel()).all(), (lines, tgt, thr, conn)
                assert (pm.reshape(H, W)[walk & ~target] == d[walk & ~target]).all()             # on a walkable point: the plane value
                if conn == 4:                       # the step leads to a neighbour one move nearer, and no lower code does
                    for (x, y, _), v, s in zip(pts.tolist(), pm.tolist(), ps.tolist()):
                        if 0 < v < wo.FAR:
                            near = [c for c, (dy, dx) in enumerate(wo.MOVES, start=1)
                                    if 0 <= y + dy < H and 0 <= x + dx < W and 0 <= d[y + dy, x + dx] == v - 1]
                            assert s == near[0], (x, y, v, s, near)
                        else:
                            assert s == 0
                seen_far += int((d == wo.FAR).any())
                seen_near += int(((d > 3) & (d < wo.FAR)).any())
    assert seen_far >= 6 and seen_near >= 12


def test_oracle_by_hand():
    m = np.array([[1, 0, 3, 0],
                  [0, 3, 0, 0],
                  [3, 0, 0, 2]], dtype=np.uint8)
    F, X = wo.FAR, wo.BLOCKED
    assert wo.moves(m, 2, 1, 4).tolist() == [[0, 1, X, F], [1, X, F, F], [X, F, F, X]]
    assert wo.moves(m, 2, 1, 8).tolist() == [[0, 1, X, 3], [1, X, 2, 3], [X, 2, 3, X]]
    assert wo.moves(m, 2, 1, 8, max_moves=2).tolist() == [[0, 1, X, 2], [1, X, 2, 2], [X, 2, 2, X]]
    assert wo.moves(m | 0xF8, 2, 1, 8).tolist() == wo.moves(m, 2, 1, 8).tolist()              # only status & 7 counts
    assert wo.moves(m, 2 | 4, 1 | 2, 4).tolist() == [[0, 1, X, 2], [1, X, 2, 1], [X, 2, 1, 0]]   # overlap: a cell that is both is a target
    t = np.zeros((3, 4), dtype=np.uint8)
    t[0, 3] = 9
    assert wo.moves(m, 0, 1 | 2 | 8, 4, targets=t).tolist() == [[3, 2, 1, 0], [4, 3, 2, 1], [5, 4, 3, X]]
    p = np.ones((3, 4), dtype=np.uint8)
    p[1, 2] = 0
    assert wo.moves(m, 0, 1 | 2 | 8, 4, passable=p, targets=t).tolist() == [[3, 2, 1, 0], [4, 3, X, 1], [5, 4, 5, X]]
    a = wo.answer(m, 2, 1, 8, pts=np.array([[0, 0, 1], [2, 0, 1], [3, 2, 1], [1, 1, 0], [4, 0, 1], [3, 0, 2]]), max_moves=0)
    assert a["reached"] == 7 and a["levels"] == 3
    assert a["point_moves"].tolist() == [0, 2, 3, -1, -1, 3] and a["point_step"].tolist() == [0, 0, 0, -1, -1, 0]
    pm, ps = wo.points(m, np.array([[2, 0, 1], [1, 1, 1], [1, 2, 1]]), 2, 1, 4)
    assert pm.tolist() == [2, 2, F] and ps.tolist() == [3, 1, 0]                                # a line cell beside the route; ties: lowest code
    pm, ps = wo.points(m, np.array([[2, 0, 1], [1, 1, 1]]), 2, 1, 4, max_moves=1)
    assert pm.tolist() == [1, 1] and ps.tolist() == [0, 0]
    assert wo.reached(m, 2, 1, 8, max_moves=2) == 4 and wo.levels(m, 2, 1, 8, max_moves=2) == 2 and wo.levels(m, 2, 1, 8, max_moves=9) == 3


# ---------------------------------------------------------------------------------------------- 2. the scenes
def test_scenes_claim_what_the_oracle_says():
    names, claimed = set(), 0
    for H, W in ww.SCENE_SHAPES:
        sc = ww.scenes(H, W)
        for e, s in enumerate(sc):
            pas, tgt = ww.planes_of(s, e, len(sc), H, W)
            a = wo.answer(s["map"], ro.mask_of(s["target"]) if s["target"] else 0, ro.mask_of(s["through"]), s["conn"], pas, tgt, s["points"])
            if s["claim"] is not None:
                s["claim"](a["moves"], a["point_moves"], a["point_step"], a["reached"], a["levels"])
                claimed += 1
            names.add(s["name"])
            if s["name"] == "serpentine_h_4" and (H, W) == (40, 130):
                assert a["levels"] > 2000                                                   # a corridor of a few thousand cells
    assert {"serpentine_h_4", "spiral_4", "gaps_a_4", "gaps_b_4", "gaps_c_4", "row_seams_4", "row_seams_8", "wall_to_the_last_column_4",
            "borders", "no_seed", "nothing_open", "enclosed_target", "on_the_line", "tie", "targets_shared", "targets_and_passable",
            "targets_per_env", "both_per_env", "points", "masks_overlap"} <= names
    assert claimed >= 40


def test_corridor_and_caps():
    m = ww.corridor(9, 40, 30)
    a = wo.answer(m, 2, 1, 4)
    assert a["levels"] == 30 == a["reached"] and a["moves"][2, 2:32].tolist() == list(range(1, 31))
    for M in (1, 17, 30):
        pts = np.array([[1 + M, 2, 1], [2 + M, 2, 1], [M, 1, 1], [1 + M, 1, 1]])       # at the cap; one cell on; beside the route, twice
        c = wo.answer(m, 2, 1, 4, pts=pts, max_moves=M)
        assert c["levels"] == M == c["reached"] and c["moves"].max() == M
        assert c["point_moves"].tolist() == [M, M, M, M]
        assert c["point_step"].tolist() == [3, 0, 2, 0]         # at the cap the step is still given; one more cell along it is 0


# ---------------------------------------------------------------------------------------------- 3. the ABI
def test_header_declares_and_lib_binds_walk():
    from simfire_amd import _lib
    text = open(os.path.join(ROOT, "include", "simfire_hip.h")).read()
    assert re.search(r"int\s+sf_walk\s*\(\s*sf_sim\s*\*\s*sim\s*,\s*const\s+sf_walk_params\s*\*\s*params\s*,\s*int32_t\s+n\s*,\s*"
                     r"const\s+int32_t\s*\*\s*envs[^,)]*,\s*const\s+sf_walk_out\s*\*\s*out\s*\)\s*;", text)
    assert re.search(r"typedef\s+struct\s+sf_walk_params\s*\{[^}]*int32_t\s+target_mask\s*,\s*through_mask\s*;[^}]*int32_t\s+connectivity\s*;"
                     r"[^}]*int32_t\s+k\s*;[^}]*int32_t\s+max_moves\s*;[^}]*int32_t\s+passable_per_env\s*;[^}]*int32_t\s+targets_per_env\s*;"
                     r"[^}]*const\s+uint8_t\s*\*\s*passable\s*;[^}]*const\s+uint8_t\s*\*\s*targets\s*;[^}]*const\s+int32_t\s*\*\s*points\s*;"
                     r"[^}]*int64_t\s+scratch_bytes\s*;[^}]*int32_t\s+reserved\s*\[\s*2\s*\]\s*;[^}]*\}\s*sf_walk_params\s*;", text)
    assert re.search(r"typedef\s+struct\s+sf_walk_out\s*\{[^}]*int32_t\s*\*\s*moves\s*;[^}]*int32_t\s*\*\s*point_moves\s*;[^}]*int32_t\s*\*\s*point_step\s*;"
                     r"[^}]*int32_t\s*\*\s*reached\s*;[^}]*int32_t\s*\*\s*levels\s*;[^}]*\}\s*sf_walk_out\s*;", text)
    assert re.search(r"#define\s+SF_WALK_FAR\s+2147483647\b", text) and re.search(r"#define\s+SF_WALK_BLOCKED\s+\(-1\)", text)
    assert text.index("int sf_reach(") < text.index("Walking distance") < text.index("int sf_walk(") < text.index("Agents on the device")
    section = text[text.index("Walking distance"):text.index("int sf_walk(")]
    assert "no counterpart" in section and "LOWEST-numbered" in section and "hipMalloc" in section
    assert "Reach of the fire" not in section and "Agents on the device" not in section
    P, O = _lib.SfWalkParams, _lib.SfWalkOut
    assert C.sizeof(P) == 72
    assert [(f[0], getattr(P, f[0]).offset) for f in P._fields_] == [
        ("target_mask", 0), ("through_mask", 4), ("connectivity", 8), ("k", 12), ("max_moves", 16), ("passable_per_env", 20),
        ("targets_per_env", 24), ("passable", 32), ("targets", 40), ("points", 48), ("scratch_bytes", 56), ("reserved", 64)]
    assert C.sizeof(O) == 5 * C.sizeof(C.c_void_p) and [f[0] for f in O._fields_] == ["moves", "point_moves", "point_step", "reached", "levels"]
    assert "sf_walk" in _lib.SIGNATURES and len(_lib.SIGNATURES["sf_walk"]) == 5
    assert (_lib.SF_WALK_FAR, _lib.SF_WALK_BLOCKED) == (2 ** 31 - 1, -1) == (wo.FAR, wo.BLOCKED)
    csrc = os.path.join(ROOT, "simfire_amd", "csrc")
    assert open(os.path.join(csrc, "simfire_hip.hip")).read().count('#include "sf_walk_kernels.h"') == 1
    # the step kernels and the other features do not know the new kernel
    for unit in sorted(os.listdir(csrc)):
        if unit.endswith((".hip", ".h")) and unit not in ("simfire_hip.hip", "sf_host_query.h", "sf_walk_kernels.h"):
            assert "k_walk" not in open(os.path.join(csrc, unit)).read(), unit
    kernels = open(os.path.join(csrc, "sf_walk_kernels.h")).read()
    assert "asm" not in re.sub(r"//[^\n]*", "", kernels)        # plain C++ only


def test_built_library_exports_sf_walk():
    from simfire_amd import _lib
    L = _lib.load()                        # (raises if the library has not been built)
    assert L.sf_walk.argtypes == _lib.SIGNATURES["sf_walk"]
    p = _lib.SfWalkParams(target_mask=2, through_mask=1)
    o = _lib.SfWalkOut(reached=16)
    e = np.zeros(1, dtype=np.int32)
    assert L.sf_walk(None, C.byref(p), 1, e.ctypes.data_as(C.c_void_p), C.byref(o)) == _lib.SF_EINVAL
    assert b"sf_walk" in L.sf_last_error()


# ------------------------------------------------------------------------- 4. errors before any library call
class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called: {name}")


def _bare_engine(E=4, H=24, W=40):
    from simfire_amd.engine import FireEngine
    eng = FireEngine.__new__(FireEngine)
    eng._L, eng._h = _NoDevice(), None
    eng.n_envs, eng.H, eng.W = E, H, W
    eng.async_mode, eng._blobs_in_flight = False, []
    return eng


@pytest.mark.parametrize("kw", [
    dict(target=0), dict(target=None), dict(target=()), dict(target=64), dict(target=("SMOULDERING",)), dict(target=(6,)), dict(target=True),
    dict(through=0), dict(through=64), dict(through=(1.0,)), dict(through=None), dict(through=()),
    dict(connectivity=6), dict(connectivity=-4), dict(connectivity=8.0), dict(connectivity=True), dict(connectivity="8"),
    dict(max_moves=-1), dict(max_moves=1.5), dict(max_moves=2 ** 31), dict(max_moves=True),
    dict(scratch_bytes=-1), dict(scratch_bytes=1.5), dict(scratch_bytes=1),
    dict(envs=[4]), dict(envs=[-1]), dict(envs=[[0, 1]]), dict(envs=[0.0]),
    dict(), dict(plane=1), dict(reached="yes"), dict(levels=0), dict(plane=True, step=True), dict(step=True),
    dict(plane=True, points=np.zeros((4, 2, 3), dtype=np.int32)), dict(plane=True, passable=np.ones((24, 40), dtype=np.uint8)),
    dict(plane=True, targets=np.ones((24, 40), dtype=np.uint8)),
])
def test_python_argument_errors(kw):
    eng = _bare_engine()
    kw = dict(kw)
    if set(kw) - {"plane", "reached", "levels", "step"}:
        kw.setdefault("plane", True)
    with pytest.raises(ValueError, match="walk"):
        eng.walk(**kw)


def test_request_forms_and_scratch_need():
    from simfire_amd import walk
    from simfire_amd.enums import BurnStatus
    assert walk.request() == (2, 1, 4, 0, 0)
    assert walk.request(("BURNING", "BURNED"), ("UNBURNED", "BURNING"), 8, 3, 4096) == (6, 3, 8, 3, 4096)
    assert walk.request(BurnStatus.FIRELINE, [BurnStatus.UNBURNED, 2], connectivity=0)[:3] == (8, 5, 4)
    assert walk.request(None, 63, targets=True)[:2] == (0, 63) and walk.request((), 1, targets=True)[0] == 0
    assert walk.request(np.int64(2), 57, None, None)[:4] == (2, 57, 4, 0)
    for tgt, thr in ww.MASK_PAIRS:
        assert walk.request(tgt, thr)[:2] == (ro.mask_of(tgt), ro.mask_of(thr))
    with pytest.raises(ValueError, match="^walk: "):
        walk.request(("EMBERS",))
    with pytest.raises(ValueError, match="step needs connectivity 4"):
        walk.WalkSpec(2, 24, 40, connectivity=8, step=True, points=_FakePoints())
    # three bit planes (24 bytes per band row) and two halos (40 bytes per band), rounded up to 256 - as the header states it
    assert walk.scratch_need(1024, 1024) == 64 * 16 * (16 * 24 + 40) == _bare_engine(H=1024, W=1024).walk_scratch_bytes()
    assert walk.scratch_need(33, 17) == (3 * (16 * 24 + 40) + 255) // 256 * 256
    assert walk.scratch_need(977, 1030) == (1054 * (16 * 24 + 40) + 255) // 256 * 256
    assert walk.MOVES == {c: mv for c, mv in enumerate(wo.MOVES, start=1)}
    text = open(os.path.join(ROOT, "include", "simfire_hip.h")).read()
    assert "16 * ceil(height / 16) * ceil(pitch / 64) * 24 bytes + 40" in text


class _FakePoints:
    """Stops ``WalkSpec`` before it looks at a tensor: the connectivity check comes first."""


def test_batched_fire_env_refuses_a_bad_moves_to_option():
    from simfire_amd.vecenv import BatchedFireEnv

    class _Sim:
        n_envs = 2
        _engine = _bare_engine(E=2)
    for bad in (dict(radius=3), dict(target=("EMBERS",)), dict(target=None), dict(through=()), dict(max_moves=-2), dict(connectivity=8), "on"):
        with pytest.raises(ValueError, match="moves_to"):
            BatchedFireEnv(_Sim(), 1, np.zeros((1, 2), dtype=np.int32), moves_to=bad)
