"""Fire travel time without a device (``sf_travel``): the float32 heap Dijkstra of ``tests/_travel_oracle.py``
against a relaxation to the fixed point (equality) and scipy's float64 Dijkstra (within the rounding of the route), what the hand-made
scenes of ``tests/_travel_worlds.py`` claim, the link to the automaton on a uniform world, the ABI as the header and the binding state
it, and the Python argument errors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _reach_oracle as ro
import _travel_oracle as to
import _travel_worlds as tw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- 1. the oracle
def test_heap_equals_relaxation_in_any_order():
    """Twelve random 24 x 40 worlds, 15 % unburnable cells, some zero entries, three sources each, both connectivities: the heap
    Dijkstra, whole-grid sweeps and a chaotic order of partial sweeps agree in every bit - float32 addition is monotone and the weights
    are >= 0, so the greatest solution is unique and no result depends on the order of the relaxations."""
    rng = np.random.default_rng(2601)
    H, W = 24, 40
    inf_seen = 0
    for i in range(12):
        conn = (8, 4)[i % 2]
        m = tw.random_map(rng, H, W, lines=0.08)
        R8 = tw.random_rates(rng, H, W, dead=0.15, holes=0.08) * rng.choice([1.0, 0.37, 1.9])
        src, opn = to.cells(m, 2, 1)
        w = to.weights(R8, tw.PIXEL_SCALE, conn)
        assert w.dtype == np.float32 and (w >= 0).all() and np.isinf(w[:, R8.sum(axis=0) == 0]).all()
        T = to.dijkstra(src, opn, w)
        assert T.dtype == np.float32
        assert (T == to.relax_to_fixpoint(src, opn, w)).all(), i
        assert (T == to.relax_to_fixpoint(src, opn, w, order=np.random.default_rng(i))).all(), i
        cap = np.float32(np.median(T[np.isfinite(T) & opn])) if (np.isfinite(T) & opn).any() else np.float32(1.0)
        Tc = to.dijkstra(src, opn, w, cap)
        assert (Tc == to.relax_to_fixpoint(src, opn, w, cap, order=np.random.default_rng(100 + i))).all(), i
        assert (Tc == np.where(T <= cap, T, np.inf)).all(), i          # every value within the cap stays exact, nothing else survives
        inf_seen += int(np.isinf(T[opn]).any())
    assert inf_seen >= 3


@pytest.mark.parametrize("conn", [4, 8])
def test_oracle_against_scipy_float64(conn):
    """scipy's Dijkstra in float64 over the same float32 weights: the two minima differ by the rounding of the additions on a route
    at most - (additions on the longer of the two routes) x 2^-24, relative."""
    sp = pytest.importorskip("scipy.sparse")
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    rng = np.random.default_rng(2602 + conn)
    H, W = 24, 40
    idx = np.arange(H * W).reshape(H, W)
    for i in range(4):
        m = tw.random_map(rng, H, W, lines=0.1)
        R8 = tw.random_rates(rng, H, W, dead=0.15, holes=0.08)
        a = to.answer(m, R8, tw.PIXEL_SCALE, 2, 1, conn)
        src, opn = to.cells(m, 2, 1)
        w = to.weights(R8, tw.PIXEL_SCALE, conn)
        rows, cols, vals = [], [], []
        for k in range(8):
            nb_ok = to._neighbour((src | opn).astype(np.uint8), k, 0).astype(bool)    # the neighbour is on the grid and source or open
            edge = opn & np.isfinite(w[k]) & nb_ok
            rows.append(to._neighbour(idx, k, -1)[edge])                              # from the neighbour ...
            cols.append(idx[edge])                                                    # ... into the cell
            vals.append(w[k][edge].astype(np.float64))
        g = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(H * W, H * W))
        d64, pr = csgraph.dijkstra(g, directed=True, indices=np.flatnonzero(src), min_only=True, return_predecessors=True)[:2]
        d64 = d64.reshape(H, W)
        T = a["T"]
        assert (np.isinf(T[opn]) == np.isinf(d64[opn])).all()
        hops32 = to.hops_of(a["pred"])
        hops64 = np.zeros(H * W, dtype=np.int64)
        for c in np.argsort(d64.ravel(), kind="stable"):
            if pr[c] >= 0:
                hops64[c] = hops64[pr[c]] + 1
        fin = opn & np.isfinite(T)
        T64 = T.astype(np.float64)[fin]
        tol = np.maximum(hops32, hops64.reshape(H, W))[fin] * 2.0 ** -24 * np.maximum(T64, d64[fin]) * 1.01
        assert (np.abs(T64 - d64[fin]) <= tol).all(), (conn, i)
        assert fin.sum() > 200 and hops32.max() > 5


def test_two_routes_and_the_tie():
    """A short slow way and a long fast way to the same cell: the faster wins; and where two neighbours give the same float32 the
    lowest k is the pred."""
    H, W = 5, 9
    m = np.full((H, W), 3, dtype=np.uint8)
    m[2, 0] = 1
    m[2, 1:8] = 0                                  # the short way: 7 cells along row 2 ...
    m[0, 0:9] = 0                                  # ... the long way: up, along row 0, down the last column (4-moves)
    m[1, 0] = m[1, 8] = m[2, 8] = 0
    m[2, 7] = 0
    R8 = np.zeros((8, H, W))
    R8[:, 2, 1:8] = 3.0                            # slow: 10 minutes a cell
    R8[:, 0, :] = R8[:, 1, 0] = R8[:, 1, 8] = R8[:, 2, 8] = 300.0
    a = to.answer(m, R8, 30.0, 2, 1, 4)
    w_slow, w_fast = np.float32(10.0), np.float32(30.0 / 300.0)
    assert a["minutes"][2, 8] == tw.fold(w_fast, 12)                                  # 12 fast cells: up 2, along 8, down 2
    assert a["minutes"][2, 7] == tw.fold(w_fast, 12) + w_slow and a["pred"][2, 7] == 3    # entered from (2, 8): offset (+1, 0)
    assert a["minutes"][2, 1] == w_slow and a["pred"][2, 1] == 4                      # the slow way still wins near the fire
    meet = [x for x in range(1, 8) if a["pred"][2, x] == 4][-1]
    assert a["minutes"][2, meet] == tw.fold(w_slow, meet) and a["pred"][2, meet + 1] == 3
    # the tie: a cell with two neighbours at the same time and equal weights - k = 1 (from below) beats k = 6 (from above)
    m = np.zeros((3, 3), dtype=np.uint8)
    m[0, :] = m[2, :] = 1
    b = to.answer(m, np.full((8, 3, 3), 6.0), 30.0, 2, 1, 4)
    assert b["pred"][1].tolist() == [1, 1, 1] and (b["minutes"][1] == np.float32(5.0)).all()
    b = to.answer(m, np.full((8, 3, 3), 6.0), 30.0, 2, 1, 8)
    assert b["pred"][1].tolist() == [0, 0, 1]                                         # with diagonals: k = 0 where (x + 1, y + 1) is on the grid
    assert b["reached"] == 3 and b["last"] == np.float32(5.0)


# ---------------------------------------------------------------------------------------------- 2. the scenes
@pytest.mark.parametrize("shape", tw.SCENE_SHAPES[:4], ids=["%dx%d" % s for s in tw.SCENE_SHAPES[:4]])
def test_scenes_claim_what_the_oracle_says(shape):
    H, W = shape
    sc = tw.scenes(H, W)
    names, claimed = set(), 0
    for e, s in enumerate(sc):
        pas, src = tw.planes_of(s, e, len(sc), H, W)
        a = to.answer(s["map"], s["R8"], tw.PIXEL_SCALE, ro.mask_of(s["source"]) if s["source"] else 0, ro.mask_of(s["through"]),
                      s["conn"] or 8, pas, src, s["points"], s["max_minutes"])
        assert a["minutes"].dtype == np.float32 and a["pred"].dtype == np.int8 and a["point_minutes"].dtype == np.float32
        if s["claim"] is not None:
            s["claim"](a)
            claimed += 1
        names.add(s["name"])
    assert {"random_0", "random_3", "unburnable_blocks", "sources_shared", "sources_per_env", "both_per_env", "no_source", "walled_in",
            "points_on_the_line", "points_capped"} <= names
    if shape == (40, 130):
        assert {"serpentine_h", "serpentine_v", "spiral", "fast_strip", "one_way"} <= names
    if shape == (64, 64):
        assert {"corner_gap_8", "corner_gap_4", "border_gap_4", "source_on_a_tile_border"} <= names
    assert claimed >= 8


def test_corridor_and_caps():
    m = tw.corridor(9, 40, 30)
    R8 = np.full((8, 9, 40), 7.0)
    w = np.float32(30.0 / 7.0)
    a = to.answer(m, R8, 30.0, 2, 1, 4)
    assert a["reached"] == 30 and a["last"] == tw.fold(w, 30) and [a["minutes"][2, 1 + j] for j in (1, 17, 30)] == [tw.fold(w, j) for j in (1, 17, 30)]
    end = float(tw.fold(w, 30))
    for M, n in ((float(np.nextafter(np.float32(end), np.float32(0))), 29), (end, 30), (float(tw.fold(w, 17)) + 0.5, 17)):
        pts = np.array([[31, 2, 1], [1 + n, 2, 1], [2 + n, 1, 1]])                   # the last cell; the last one within the cap; the wall beside the next
        c = to.answer(m, R8, 30.0, 2, 1, 4, pts=pts, max_minutes=M)
        cap = np.float32(M)
        assert c["reached"] == n and c["last"] == tw.fold(w, n) and c["minutes"].max() == cap
        assert c["point_minutes"].tolist() == [float(tw.fold(w, 30)) if n == 30 else float(cap), float(tw.fold(w, n)), float(cap)]
        assert (c["pred"][2, 2:2 + n] == 4).all() and (c["pred"][2, 2 + n:] == -1).all()


# ---------------------------------------------------------------------------------------------- 3. the automaton
@pytest.mark.parametrize("R,rate,md", [(7.0, 1.0, 8), (13.0, 0.5, 7)])
def test_uniform_world_links_travel_time_to_the_automaton(R, rate, md):
    """Flat, windless, uniform: every cell takes q = pixel_scale / (R * update_rate) updates of burn, and burns when the sum EXCEEDS
    pixel_scale - floor(q) + 1 updates for a q that is no integer.  A cell h Chebyshev cells from the ignition burns at update
    h * (floor(q) + 1) (the project's arrival oracle over the dense automaton), while the travel time is the h-fold float32 sum of
    w = float32(pixel_scale / R): the forecast is continuous, the automaton rounds every cell up to whole updates."""
    from _arrival_oracle import arrival_from_maps
    from oracle import fire_dense
    H, W, ps = 17, 19, 30.0
    q = ps / (R * rate)
    per_cell = int(np.floor(q)) + 1
    assert abs(q - round(q)) > 0.05 and per_cell < md
    o = fire_dense.DenseOracle(n_envs=1, **tw.engine_kwargs(H, W, update_rate=rate, md=md))
    R8 = np.full((8, H, W), R)
    o.set_rtable(R8)
    y0, x0 = 8, 9
    o.reset([(x0, y0)])
    maps = [o.fire_map(0).copy()]
    for _ in range(per_cell * 9 + 2):
        o.step(1)
        maps.append(o.fire_map(0).copy())
    arr = arrival_from_maps(maps)
    h = np.maximum(np.abs(np.arange(H)[:, None] - y0), np.abs(np.arange(W)[None, :] - x0))
    assert (arr == h * per_cell).all()
    m = np.zeros((H, W), dtype=np.uint8)
    m[y0, x0] = 1
    a = to.answer(m, R8, ps, 2, 1, 8)
    w = np.float32(ps / R)
    folds = np.array([tw.fold(w, n) for n in range(max(H, W))], dtype=np.float32)
    assert (a["minutes"] == folds[h]).all()
    # in updates the forecast runs ahead of the automaton by the rounding up of every cell: q against floor(q) + 1
    ahead = arr[h > 0] / (a["minutes"][h > 0] / np.float32(rate))
    assert np.allclose(ahead, per_cell / q, rtol=1e-5)


# ---------------------------------------------------------------------------------------------- 4. the ABI
def test_header_declares_and_lib_binds_travel():
    from simfire_amd import _lib
    text = open(os.path.join(ROOT, "include", "simfire_hip.h")).read()
    assert re.search(r"int\s+sf_travel\s*\(\s*sf_sim\s*\*\s*sim\s*,\s*const\s+sf_travel_params\s*\*\s*params\s*,\s*int32_t\s+n\s*,\s*"
                     r"const\s+int32_t\s*\*\s*envs[^,)]*,\s*const\s+sf_travel_out\s*\*\s*out\s*\)\s*;", text)
    assert re.search(r"typedef\s+struct\s+sf_travel_params\s*\{[^}]*int32_t\s+source_mask\s*,\s*through_mask\s*;[^}]*int32_t\s+connectivity\s*;"
                     r"[^}]*int32_t\s+k\s*;[^}]*float\s+max_minutes\s*;[^}]*int32_t\s+passable_per_env\s*;[^}]*int32_t\s+sources_per_env\s*;"
                     r"[^}]*const\s+uint8_t\s*\*\s*passable\s*;[^}]*const\s+uint8_t\s*\*\s*sources\s*;[^}]*const\s+int32_t\s*\*\s*points\s*;"
                     r"[^}]*int64_t\s+scratch_bytes\s*;[^}]*int32_t\s+reserved\s*\[\s*2\s*\]\s*;[^}]*\}\s*sf_travel_params\s*;", text)
    assert re.search(r"typedef\s+struct\s+sf_travel_out\s*\{[^}]*float\s*\*\s*minutes\s*;[^}]*int8_t\s*\*\s*pred\s*;[^}]*float\s*\*\s*point_minutes\s*;"
                     r"[^}]*int32_t\s*\*\s*reached\s*;[^}]*float\s*\*\s*last\s*;[^}]*int32_t\s*\*\s*activations\s*;[^}]*\}\s*sf_travel_out\s*;", text)
    assert re.search(r"#define\s+SF_TRAVEL_BLOCKED\s+\(-1\.0f\)", text)
    assert text.index("int sf_walk(") < text.index("Fire travel time") < text.index("int sf_travel(") < text.index("Fire behaviour per cell")
    section = text[text.index("Fire travel time"):text.index("int sf_travel(")]
    assert "NOT the automaton" in section and "LOWEST k" in section and "no counterpart" in section and "hipMalloc" in section
    assert "attenuate_line_ros is not modelled" in section and "Walking distance" not in section
    P, O = _lib.SfTravelParams, _lib.SfTravelOut
    assert C.sizeof(P) == 72
    assert [(f[0], getattr(P, f[0]).offset) for f in P._fields_] == [
        ("source_mask", 0), ("through_mask", 4), ("connectivity", 8), ("k", 12), ("max_minutes", 16), ("passable_per_env", 20),
        ("sources_per_env", 24), ("passable", 32), ("sources", 40), ("points", 48), ("scratch_bytes", 56), ("reserved", 64)]
    assert dict(P._fields_)["max_minutes"] is C.c_float
    assert C.sizeof(O) == 6 * C.sizeof(C.c_void_p)
    assert [f[0] for f in O._fields_] == ["minutes", "pred", "point_minutes", "reached", "last", "activations"]
    assert "sf_travel" in _lib.SIGNATURES and len(_lib.SIGNATURES["sf_travel"]) == 5
    assert _lib.SF_TRAVEL_BLOCKED == -1.0 == float(to.BLOCKED)
    from simfire_amd import travel
    from oracle import rothermel_np
    assert travel.SRC_OFFSETS == tuple(rothermel_np.SRC_OFFSETS) == to.SRC_OFFSETS


def test_kernel_is_included_once_and_named_by_nobody_else():
    csrc = os.path.join(ROOT, "simfire_amd", "csrc")
    assert open(os.path.join(csrc, "simfire_hip.hip")).read().count('#include "sf_travel_kernels.h"') == 1
    # the step path, the enqueue layer and the other features do not know the new kernel
    for unit in sorted(os.listdir(csrc)):
        if unit.endswith((".hip", ".h")) and unit not in ("sf_host_query.h", "sf_travel_kernels.h"):
            assert "k_travel" not in open(os.path.join(csrc, unit)).read(), unit
    kernels = open(os.path.join(csrc, "sf_travel_kernels.h")).read()
    assert "__global__" in kernels and "k_travel" in kernels
    assert "asm" not in re.sub(r"//[^\n]*", "", kernels)        # plain C++ only
    for other in ("k_walk", "k_reach", "k_dist_", "k_ensemble"):
        assert other not in kernels
    host = open(os.path.join(csrc, "sf_host_query.h")).read()
    assert host.count("k_travel") >= 1 and 'extern "C" int sf_travel(' in host
    assert "sf_travel" in open(os.path.join(csrc, "sf_handle.h")).read()


def test_built_library_exports_sf_travel():
    from simfire_amd import _lib
    L = _lib.load()                        # (raises if the library has not been built)
    assert L.sf_travel.argtypes == _lib.SIGNATURES["sf_travel"]
    p = _lib.SfTravelParams(source_mask=2, through_mask=1)
    o = _lib.SfTravelOut(reached=16)
    e = np.zeros(1, dtype=np.int32)
    assert L.sf_travel(None, C.byref(p), 1, e.ctypes.data_as(C.c_void_p), C.byref(o)) == _lib.SF_EINVAL
    assert b"sf_travel" in L.sf_last_error()


# ------------------------------------------------------------------------- 5. errors before any library call
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
    dict(source=0), dict(source=None), dict(source=()), dict(source=64), dict(source=("SMOULDERING",)), dict(source=(6,)), dict(source=True),
    dict(through=0), dict(through=64), dict(through=(1.0,)), dict(through=None), dict(through=()),
    dict(connectivity=6), dict(connectivity=-4), dict(connectivity=8.0), dict(connectivity=True), dict(connectivity="8"),
    dict(max_minutes=-1), dict(max_minutes=-0.5), dict(max_minutes=float("nan")), dict(max_minutes=True), dict(max_minutes="10"),
    dict(scratch_bytes=-1), dict(scratch_bytes=1.5), dict(scratch_bytes=1),
    dict(envs=[4]), dict(envs=[-1]), dict(envs=[[0, 1]]), dict(envs=[0.0]),
    dict(plane=False), dict(plane=1), dict(pred="yes"), dict(reached=0), dict(last=None), dict(activations=2),
    dict(points=np.zeros((4, 2, 3), dtype=np.int32)), dict(passable=np.ones((24, 40), dtype=np.uint8)),
    dict(sources=np.ones((24, 40), dtype=np.uint8)),
])
def test_python_argument_errors(kw):
    eng = _bare_engine()
    with pytest.raises(ValueError, match="travel"):
        eng.travel(**kw)


def test_request_forms_and_scratch_need():
    from simfire_amd import travel
    from simfire_amd.enums import BurnStatus
    assert travel.request() == (2, 1, 0, 0.0, 0)
    assert travel.request(("BURNING", "BURNED"), ("UNBURNED", "BURNING"), 8, 3, 4096) == (6, 3, 8, 3.0, 4096)
    assert travel.request(BurnStatus.FIRELINE, [BurnStatus.UNBURNED, 2], connectivity=4)[:3] == (8, 5, 4)
    assert travel.request(None, 63, sources=True)[:2] == (0, 63) and travel.request((), 1, sources=True)[0] == 0
    assert travel.request(np.int64(2), 57, None, None)[:4] == (2, 57, 0, 0.0)
    assert travel.request(max_minutes=0.1)[3] == float(np.float32(0.1)) and travel.request(max_minutes=np.float32(2.5))[3] == 2.5
    for src, thr in tw.MASK_PAIRS:
        assert travel.request(src, thr)[:2] == (ro.mask_of(src), ro.mask_of(thr))
    with pytest.raises(ValueError, match="^travel: "):
        travel.request(("EMBERS",))
    # the working array, rounded up to 256 - as the header states it
    assert travel.scratch_need(1024, 1024) == 4 << 20 == _bare_engine(H=1024, W=1024).travel_scratch_bytes()
    assert travel.scratch_need(33, 17) == (4 * 33 * 17 + 255) // 256 * 256 == 2304
    text = open(os.path.join(ROOT, "include", "simfire_hip.h")).read()
    assert "4 * height * width\n * bytes rounded up to 256" in text or "4 * height * width bytes rounded up to 256" in text


def test_simulation_classes_refuse_a_bad_unit_before_anything_else():
    from simfire_amd.simulation import BatchedFireSimulation, FireSimulation, _travel_unit
    for cls in (FireSimulation, BatchedFireSimulation):
        sim = cls.__new__(cls)
        sim._engine = _bare_engine()
        with pytest.raises(ValueError, match="unit"):
            sim.time_to_fire(unit="hours")
    assert _travel_unit(dict(a=1), "minutes", 2.0) == dict(a=1)


def test_batched_fire_env_refuses_a_bad_time_to_fire_option():
    from simfire_amd.vecenv import BatchedFireEnv

    class _Sim:
        n_envs = 2
        _engine = _bare_engine(E=2)
    for bad in (dict(radius=3), dict(source=("EMBERS",)), dict(source=None), dict(through=()), dict(max_minutes=-2.0), dict(connectivity=8), "on"):
        with pytest.raises(ValueError, match="time_to_fire"):
            BatchedFireEnv(_Sim(), 1, np.zeros((1, 2), dtype=np.int32), time_to_fire=bad)
