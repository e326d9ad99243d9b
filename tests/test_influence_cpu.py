"""Fire influence without a device (``sf_influence``): the oracle of ``tests/_influence_oracle.py`` against its
own leaf-peeling restatement and ``networkx``, what the hand-made forests of ``tests/_influence_worlds.py`` are there for, the history
rule, the committed trajectories, the ABI as the header and the binding state it, and the Python argument errors."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

import _influence_oracle as io
import _influence_worlds as iw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- 1. the oracle
def _same(a, b, tag):
    assert set(a) == set(b), tag
    for k in a:
        assert np.array_equal(a[k], b[k]), (tag, k)


def test_walk_up_against_leaf_peeling():
    """Random 24 x 40 planes - forests, and raw random bytes with cycles and bad codes -, with and without weights and include."""
    rng = np.random.default_rng(2801)
    cyclic = 0
    for i in range(12):
        pred = iw.random_forest(24, 40, 100 + i) if i % 2 else rng.integers(-3, 10, size=(24, 40)).astype(np.int8)
        w = iw.weights(24, 40, i) if i % 3 else None
        inc = iw.include(24, 40, i) if i % 4 < 2 else None
        for inclusive in (False, True):
            a, b = io.answer(pred, inc, w, inclusive), io.answer_peel(pred, inc, w, inclusive)
            _same(a, b, (i, inclusive))
        cyclic += a["cyclic"] > 0
        assert ("value" in a) == (w is not None)
    assert cyclic >= 3                                        # the raw planes do hold cycles


def test_tree_case_against_networkx():
    nx = pytest.importorskip("networkx")
    for seed in range(3):
        pred = iw.random_forest(12, 15, 200 + seed)
        a = io.answer(pred)
        par = io.parents(a["pred"])
        g = nx.DiGraph()
        g.add_nodes_from(range(par.size))
        g.add_edges_from((int(p), c) for c, p in enumerate(par) if p >= 0)
        want = np.array([len(nx.descendants(g, c)) for c in range(par.size)]).reshape(12, 15)
        assert np.array_equal(a["cells"], want) and a["cyclic"] == 0


def test_the_smallest_answers_by_hand():
    p = np.array([[-1, 4, 4], [6, -1, 6]], dtype=np.int8)        # (1,0) -> (0,0) <- (0,1); (2,0) -> (1,0) <- ... (2,1) -> (2,0)
    a = io.answer(p, weights=np.array([[1, 10, 100], [1000, 5, -7]]))
    assert a["cells"].tolist() == [[4, 2, 1], [0, 0, 0]] and a["value"].tolist() == [[1103, 93, -7], [0, 0, 0]]
    assert (a["forest"], a["roots"], a["cyclic"]) == (4, 1, 0)
    assert io.answer(p, inclusive=True)["cells"].tolist() == [[5, 3, 2], [1, 1, 1]]
    inc = np.array([[1, 0, 1], [1, 1, 1]])
    assert io.answer(p, include=inc)["cells"].tolist() == [[3, 2, 1], [0, 0, 0]]           # (1,0) counts for nobody, and still links
    assert io.answer(p, include=inc, inclusive=True)["cells"].tolist() == [[4, 2, 2], [1, 1, 1]]
    r = io.points(a, [(2, 1, 1), (2, 1, 0), (3, 0, 1), (0, 0, 2)], max_route=3)
    assert r["point_cells"].tolist() == [0, -1, -1, 4] and r["point_value"].tolist() == [0, 0, 0, 1103]
    assert r["point_route"].tolist() == [[5, 2, 1], [-1, -1, -1], [-1, -1, -1], [0, -1, -1]] and r["point_hops"].tolist() == [-2, -1, -1, 0]
    assert io.points(a, [(2, 1, 1)], max_route=4)["point_hops"].tolist() == [3]            # exactly at the route's length
    assert io.points(a, [(2, 1, 1)], max_route=9)["point_route"][0].tolist() == [5, 2, 1, 0, -1, -1, -1, -1, -1]


def test_scenes_are_what_they_are_there_for():
    H, W = 9, 11
    sc = {s["name"]: s["pred"] for s in iw.scenes(H, W)}
    assert {"serpentine", "star", "comb", "one_tree", "random_0", "random_1", "two_cycle", "fed_cycle", "off_grid", "bad_bytes", "all_none"} == set(sc)
    a = {k: io.answer(p) for k, p in sc.items()}
    n = H * W
    s = a["serpentine"]
    assert (s["forest"], s["roots"], s["cyclic"]) == (n - 1, 1, 0) and s["cells"][0, 0] == n - 1
    assert sorted(s["cells"].ravel().tolist()) == list(range(n))                       # a chain: every height once
    assert io.points(s, [(W - 1, H - 1, 1)], max_route=n)["point_hops"].tolist() == [n - 1]        # (H - 1 is even: the last row ends at its last column)
    st = a["star"]
    assert (st["forest"], st["roots"]) == (8, 1) and st["cells"][H // 2, W // 2] == 8 and st["cells"].sum() == 8
    c = a["comb"]
    assert c["roots"] == 1 and c["cells"][0, 0] == n - 1 and c["cells"][0, W - 1] == H - 1 and c["cells"][H - 1].tolist() == [0] * W
    t = a["one_tree"]
    assert (t["forest"], t["roots"]) == (n - 1, 1) and t["cells"][0, 0] == n - 1
    for k in ("random_0", "random_1"):
        assert a[k]["cyclic"] == 0 and a[k]["roots"] > 3 and a[k]["cells"].max() > 3
    assert a["two_cycle"]["cyclic"] == 2 and a["two_cycle"]["cells"][1, 1] == a["two_cycle"]["cells"][1, 2] == io.CYCLE
    assert (a["two_cycle"]["forest"], a["two_cycle"]["roots"]) == (2, 0)
    f = a["fed_cycle"]
    assert f["cyclic"] == 4 and (f["cells"] == io.CYCLE).sum() == 4 and f["cells"][4, 2] == H - 5 and f["cells"][1, 2] == 0 and f["cells"][0, 2] == 1
    assert io.points(f, [(2, H - 1, 1)], max_route=50)["point_hops"].tolist() == [-2]   # a route into the cycle never ends
    o = a["off_grid"]
    assert (o["pred"][0] == -1).all() and (o["pred"][H - 1] == -1).all() and (o["pred"][:, W - 1] == -1).all() and o["roots"] == H - 2
    assert o["cells"][1, 0] == W - 2 and o["cells"][2, 0] == W - 2                      # nothing leaks over the right border into the next row
    b = a["bad_bytes"]
    assert {8, -2, 127} <= set(sc["bad_bytes"].ravel().tolist()) and set(b["pred"].ravel().tolist()) <= set(range(-1, 8))
    e = a["all_none"]
    assert (e["forest"], e["roots"], e["cyclic"]) == (0, 0, 0) and not e["cells"].any()
    w = iw.weights(H, W)
    assert w.min() < 0 and abs(io.answer(sc["serpentine"], weights=w)["value"]).max() > 2 ** 31
    inc = iw.include(H, W)
    knocked = io.answer(sc["comb"], include=inc)
    assert 0 < (inc == 0).sum() < n and knocked["cells"][0, 0] == int((inc != 0).sum()) - int(inc[0, 0] != 0)
    pts = iw.default_points(H, W)
    assert (pts[:, 2] <= 0).any() and (pts[:, 0] >= W).any() and (pts[1] == pts[2]).all()


# ---------------------------------------------------------------------------------------------- 2. the history rule
def _mask(*offsets):
    m = 0
    for o in offsets:
        m |= 1 << io.GRAPH_OFFSETS.index(o)
    return m


def test_history_rule_by_hand():
    arr = np.full((3, 4), -1, dtype=np.int32)
    msk = np.zeros((3, 4), dtype=np.uint8)
    arr[1, 0] = 0                                             # the ignition
    arr[1, 1], msk[1, 1] = 2, _mask((-1, 0))
    # re-ignition: (2,1) burned at 3 from (1,1); a line drawn on it and a second ignition ORed (3,1), which burned LATER, into its mask
    arr[1, 2], msk[1, 2] = 3, _mask((-1, 0), (+1, 0))
    arr[1, 3], msk[1, 3] = 5, _mask((-1, 0))
    # a parent without arrival (a cell painted by load_fire_map): (0,0) names (1,0), which never arrived -> a root
    arr[0, 0], msk[0, 0] = 4, _mask((+1, 0))
    # the tie: (2,2) names (1,1) [code 7] and (1,2) [code 4], both of arrival 2
    arr[2, 1] = 2
    arr[2, 2], msk[2, 2] = 6, _mask((-1, -1), (-1, 0))
    codes = io.history_codes(msk, arr)
    assert codes[1, 0] == -1 and codes[1, 1] == 4 and codes[1, 2] == 4 and codes[1, 3] == 4
    assert codes[0, 0] == -1                                  # its only candidate never arrived
    assert codes[2, 2] == 4                                   # (1,2) at 2 via code 4 and (1,1) at 2 via code 7: the lowest code
    assert codes[2, 1] == -1 and codes[0, 3] == -1
    # equal arrivals are no candidates (strict), so no two cells can be each other's parent
    arr2 = np.array([[3, 3]], dtype=np.int32)
    assert io.history_codes(np.array([[_mask((+1, 0)), _mask((-1, 0))]], dtype=np.uint8), arr2).tolist() == [[-1, -1]]
    # a bit that names a neighbour off the grid is ignored
    assert io.history_codes(np.array([[_mask((-1, 0), (0, -1))]], dtype=np.uint8), np.array([[1]], dtype=np.int32)).tolist() == [[-1]]


@pytest.mark.parametrize("name", sorted(os.path.basename(f) for f in glob.glob(os.path.join(ROOT, "tests", "golden", "traj_g*.npz"))))
def test_history_tree_on_golden_trajectory(name):
    """The fixtures hold the reference's spread-graph edges and the map after every update.  The ignition tree keeps one of a cell's
    graph parents, so its ``cells`` is at most the graph's descendant count, everywhere - and equal on every cell all of whose
    descendants have exactly one parent in the graph."""
    from _arrival_oracle import arrival_from_maps
    d = np.load(os.path.join(ROOT, "tests", "golden", name))
    H, W = (int(v) for v in d["shape"])
    x0, y0 = (int(v) for v in d["init_pos"])
    start = np.zeros((H, W), dtype=np.uint8)
    start[y0, x0] = 1
    arrival = arrival_from_maps([start] + list(d["fire_maps"]))
    edges = d["edges"]
    masks = io.masks_from_edges(edges, H, W)
    codes = io.history_codes(masks, arrival)
    a = io.answer_peel(codes)
    assert a["cyclic"] == 0 and a["forest"] > 10
    dag = io.dag_descendants(edges, H, W)
    assert (a["cells"] <= dag).all(), name
    indeg = np.zeros(H * W, dtype=np.int64)
    for sx, sy, x, y in edges.tolist():
        indeg[y * W + x] += 1
    kids = {}
    for sx, sy, x, y in edges.tolist():
        kids.setdefault(sy * W + sx, []).append(y * W + x)
    checked = 0
    for c in range(H * W):
        seen, stack = {c}, [c]
        while stack:
            for k in kids.get(stack.pop(), ()):
                if k not in seen:
                    seen.add(k)
                    stack.append(k)
        seen.discard(c)
        if seen and all(indeg[k] == 1 for k in seen):
            assert a["cells"].ravel()[c] == dag.ravel()[c], (name, c)
            checked += 1
    # such cells are few on an open front (every ignition there has several BURNING neighbours): g1, g5, g6 and g7 hold none, the mixed
    # fuels and the line fixtures hold one to seven each - a property of the fixtures' own edge lists - and there the clause must bite
    if name.startswith(("traj_g2", "traj_g3", "traj_g4")):
        assert checked > 0, name


def test_history_tree_equals_the_graph_in_a_corridor():
    """A corridor one cell wide: every ignition has exactly one BURNING neighbour, the tree is the graph."""
    H, W, n = 3, 12, 10
    edges = np.array([(x, 1, x + 1, 1) for x in range(1, n)], dtype=np.int32)
    arrival = np.full((H, W), -1, dtype=np.int32)
    arrival[1, 1:n + 1] = np.arange(n) * 3
    a = io.answer(io.history_codes(io.masks_from_edges(edges, H, W), arrival))
    dag = io.dag_descendants(edges, H, W)
    assert np.array_equal(a["cells"], dag) and a["cells"][1, 1:n + 1].tolist() == list(range(n - 1, -1, -1)) and (a["forest"], a["roots"]) == (n - 1, 1)


def test_bit_to_code_table():
    """graph.py's neighbour order as the header writes it, against SRC_OFFSETS."""
    from simfire_amd import influence, travel
    from simfire_amd.engine import FireEngine
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "simfire_hip.h")).read())
    m = re.search(r"adj_locs order ((?:\(x(?:[+-]1)?,y(?:[+-]1)?\) ?){8})", text)
    order = []
    for gx, gy in re.findall(r"\(x([+-]1)?,y([+-]1)?\)", m.group(1)):
        order.append((int(gx or 0), int(gy or 0)))
    assert tuple(order) == influence.GRAPH_OFFSETS == io.GRAPH_OFFSETS == tuple(zip(FireEngine.GRAPH_DX, FireEngine.GRAPH_DY))
    assert influence.SRC_OFFSETS is travel.SRC_OFFSETS and tuple(travel.SRC_OFFSETS) == io.SRC_OFFSETS == iw.SRC_OFFSETS
    assert influence.BIT_TO_CODE == tuple(travel.SRC_OFFSETS.index(o) for o in order) == (3, 0, 1, 2, 4, 7, 6, 5)


# ---------------------------------------------------------------------------------------------- 3. the ABI
def test_header_declares_and_lib_binds_influence():
    from simfire_amd import _lib, influence
    text = open(os.path.join(ROOT, "include", "simfire_hip.h")).read()
    assert re.search(r"int\s+sf_influence\s*\(\s*sf_sim\s*\*\s*sim\s*,\s*const\s+sf_influence_params\s*\*\s*params\s*,\s*int32_t\s+n\s*,\s*"
                     r"const\s+int32_t\s*\*\s*envs[^,)]*,\s*const\s+sf_influence_out\s*\*\s*out\s*\)\s*;", text)
    assert re.search(r"typedef\s+struct\s+sf_influence_params\s*\{[^}]*int32_t\s+pred_source\s*;[^}]*int32_t\s+pred_per_env\s*;[^}]*int32_t\s+weight_mode\s*;"
                     r"[^}]*int32_t\s+weights_per_env\s*;[^}]*int32_t\s+include_per_env\s*;[^}]*int32_t\s+inclusive\s*;[^}]*int32_t\s+k\s*;[^}]*int32_t\s+max_route\s*;"
                     r"[^}]*const\s+int8_t\s*\*\s*pred\s*;[^}]*const\s+int32_t\s*\*\s*weights\s*;[^}]*const\s+uint8_t\s*\*\s*include\s*;"
                     r"[^}]*const\s+int32_t\s*\*\s*points\s*;[^}]*int64_t\s+scratch_bytes\s*;[^}]*int32_t\s+reserved\s*\[\s*2\s*\]\s*;[^}]*\}\s*sf_influence_params\s*;", text)
    assert re.search(r"typedef\s+struct\s+sf_influence_out\s*\{[^}]*int32_t\s*\*\s*cells\s*;[^}]*int64_t\s*\*\s*value\s*;[^}]*int8_t\s*\*\s*pred\s*;"
                     r"[^}]*int32_t\s*\*\s*forest\s*,\s*\*\s*roots\s*,\s*\*\s*cyclic\s*;[^}]*int32_t\s*\*\s*point_cells\s*;[^}]*int64_t\s*\*\s*point_value\s*;"
                     r"[^}]*int32_t\s*\*\s*point_route\s*;[^}]*int32_t\s*\*\s*point_hops\s*;[^}]*\}\s*sf_influence_out\s*;", text)
    for name, v in (("SF_INFLUENCE_PRED_PLANE", "0"), ("SF_INFLUENCE_PRED_HISTORY", "1"), ("SF_INFLUENCE_CYCLE", r"\(-2\)")):
        assert re.search(r"#define\s+%s\s+%s\s" % (name, v), text), name
    assert (_lib.SF_INFLUENCE_PRED_PLANE, _lib.SF_INFLUENCE_PRED_HISTORY, _lib.SF_INFLUENCE_CYCLE) == (0, 1, -2) and influence.MAX_ROUTE == 1 << 20
    # the section stands directly behind sf_perimeter's, in front of the agents, and uses none of the other sections' titles
    assert text.index("int sf_perimeter(") < text.index("Influence of a cell on the fire") < text.index("int sf_influence(") < text.index("Agents on the device")
    between = text[text.index("int sf_perimeter("):text.index("Influence of a cell on the fire")]
    assert between.count(";") == 1 and "typedef" not in between
    section = text[text.index("Influence of a cell on the fire"):text.index("int sf_influence(")]
    for title in ("Fire travel time", "Walking distance", "Fire behaviour per cell", "Reach of the fire", "Distance fields", "Perimeters of the fire"):
        assert title not in section, title
    for words in ("graph.py:53-82", "a(n_j) < a(c)", "ties go to the lowest code", "SF_INFLUENCE_CYCLE on C", "no bit depends on scheduling", "hipMalloc",
                  "N + 4 * N bytes (codes, counters) + 4 * N where cells is not asked for + 8 * N where there are weights and value is not asked for"):
        assert words in re.sub(r"\s*\n \* ", " ", section), words
    P, O = _lib.SfInfluenceParams, _lib.SfInfluenceOut
    assert C.sizeof(P) == 80
    assert [(f[0], getattr(P, f[0]).offset) for f in P._fields_] == [
        ("pred_source", 0), ("pred_per_env", 4), ("weight_mode", 8), ("weights_per_env", 12), ("include_per_env", 16), ("inclusive", 20), ("k", 24),
        ("max_route", 28), ("pred", 32), ("weights", 40), ("include", 48), ("points", 56), ("scratch_bytes", 64), ("reserved", 72)]
    assert C.sizeof(O) == 10 * C.sizeof(C.c_void_p)
    assert [f[0] for f in O._fields_] == ["cells", "value", "pred", "forest", "roots", "cyclic", "point_cells", "point_value", "point_route", "point_hops"]
    assert "sf_influence" in _lib.SIGNATURES and len(_lib.SIGNATURES["sf_influence"]) == 5


def test_kernels_are_included_once_and_named_by_nobody_else():
    csrc = os.path.join(ROOT, "simfire_amd", "csrc")
    assert open(os.path.join(csrc, "simfire_hip.hip")).read().count('#include "sf_influence_kernels.h"') == 1
    for unit in sorted(os.listdir(csrc)):
        if unit.endswith((".hip", ".h")) and unit not in ("sf_host_query.h", "sf_influence_kernels.h"):
            assert "k_infl" not in open(os.path.join(csrc, unit)).read(), unit
    kernels = open(os.path.join(csrc, "sf_influence_kernels.h")).read()
    names = re.findall(r"__global__[^\n]*void\s+(\w+)\s*\(", kernels)
    assert names == ["k_infl_stage", "k_infl_walk", "k_infl_finish", "k_infl_points"]
    assert "asm" not in re.sub(r"//[^\n]*", "", kernels)        # plain C++ only
    for other in ("k_walk", "k_reach", "k_dist_", "k_travel", "k_behavior", "k_ensemble", "k_perim", "k_run", "k_step"):
        assert other not in kernels, other
    walk = kernels[kernels.index("void k_infl_walk"):kernels.index("void k_infl_finish")]
    assert "__HIP_MEMORY_SCOPE_AGENT" in walk and "__ATOMIC_ACQ_REL" in walk and "__syncthreads" not in walk and "while" not in walk
    host = open(os.path.join(csrc, "sf_host_query.h")).read()
    assert 'extern "C" int sf_influence(' in host and all(n in host for n in names)
    body = host[host.index('extern "C" int sf_influence('):]
    for helper in ("check_points(", "check_reserved(", "check_aligned(", "check_scratch(", "check_envs(", "query_chunk(", "scratch_reserve("):
        assert helper in body, helper
    assert re.search(r"QueryState [^;]*\binfluence\b[^;]*;", open(os.path.join(csrc, "sf_handle.h")).read())


def test_built_library_exports_sf_influence():
    """Fails on a library built without the feature."""
    from simfire_amd import _lib
    L = _lib.load()                        # (raises if the library has not been built)
    assert L.sf_influence.argtypes == _lib.SIGNATURES["sf_influence"]
    p = _lib.SfInfluenceParams(pred_source=1)
    o = _lib.SfInfluenceOut(cells=16)
    e = np.zeros(1, dtype=np.int32)
    assert L.sf_influence(None, C.byref(p), 1, e.ctypes.data_as(C.c_void_p), C.byref(o)) == _lib.SF_EINVAL
    assert b"sf_influence" in L.sf_last_error()


# ------------------------------------------------------------------------- 4. errors before any library call
class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called: {name}")


def _bare_engine(E=4, H=24, W=40, graph=False, arrival=False, values=False):
    from simfire_amd.engine import FireEngine
    eng = FireEngine.__new__(FireEngine)
    eng._L, eng._h = _NoDevice(), None
    eng.n_envs, eng.H, eng.W = E, H, W
    eng.async_mode, eng._blobs_in_flight = False, []
    eng.spread_graph = eng.spread_graph_on = graph
    eng.arrival_on, eng.values_on = arrival, values
    return eng


_HOST = np.zeros((24, 40), dtype=np.int8)


@pytest.mark.parametrize("kw", [
    dict(), dict(pred=_HOST), dict(pred=[[1]]), dict(pred=_HOST, history=True), dict(history=1), dict(history=None),
    dict(history=True),                                                             # (neither graph nor arrival is on)
    dict(history=True, weights="values"), dict(history=True, weights="value"), dict(history=True, weights=np.ones((24, 40), dtype=np.int32)),
    dict(history=True, value=True), dict(history=True, include=np.ones((24, 40), dtype=np.uint8)), dict(history=True, inclusive=1),
    dict(history=True, cells=0), dict(history=True, value="yes"), dict(history=True, pred_out=None), dict(history=True, counts=2),
    dict(history=True, cells=False), dict(history=True, max_route=-1), dict(history=True, max_route=(1 << 20) + 1), dict(history=True, max_route=1.5),
    dict(history=True, max_route=True), dict(history=True, max_route=8), dict(history=True, points=np.zeros((4, 2, 3), dtype=np.int32)),
    dict(history=True, scratch_bytes=-1), dict(history=True, scratch_bytes=1.5), dict(history=True, scratch_bytes=1),
    dict(history=True, envs=[4]), dict(history=True, envs=[-1]), dict(history=True, envs=[[0, 1]]), dict(history=True, envs=[0.0]),
])
def test_python_argument_errors(kw):
    on = "history" in kw and kw["history"] is True and len(kw) > 1
    eng = _bare_engine(graph=on, arrival=on)                  # (the switches are on where the case is about another argument)
    with pytest.raises(ValueError, match="influence"):
        eng.influence(**kw)


def test_python_history_needs_both_switches_and_a_wide_grid_is_refused():
    from simfire_amd.influence import InfluenceSpec
    for g, a in ((False, False), (True, False), (False, True)):
        with pytest.raises(ValueError, match="spread graph and arrival"):
            InfluenceSpec(4, 24, 40, history=True, graph_on=g, arrival_on=a)
    with pytest.raises(ValueError, match="8192"):
        _bare_engine(W=8200, graph=True, arrival=True).influence(history=True)
    with pytest.raises(ValueError, match="value plane"):
        InfluenceSpec(4, 24, 40, history=True, graph_on=True, arrival_on=True, weights="values")
    s = InfluenceSpec(4, 24, 40, history=True, graph_on=True, arrival_on=True, weights="values", values_on=True, value=True, counts=True,
                      pred_out=True, envs=[3, 0, 3])
    assert s.outputs == dict(cells=((3, 24, 40), "int32"), value=((3, 24, 40), "int64"), pred=((3, 24, 40), "int8"), forest=((3,), "int32"),
                             roots=((3,), "int32"), cyclic=((3,), "int32"))
    p = s.params()
    assert (p.pred_source, p.pred_per_env, p.weight_mode, p.weights_per_env, p.include_per_env, p.inclusive, p.k, p.max_route, p.pred, p.weights,
            p.include, p.points, p.scratch_bytes) == (1, 0, 1, 0, 0, 0, 0, 0, None, None, None, None, 0)
    assert list(InfluenceSpec(4, 24, 40, history=True, graph_on=True, arrival_on=True, cells=False, counts=True).outputs) == ["forest", "roots", "cyclic"]


def test_scratch_need_is_the_headers_formula():
    from simfire_amd import influence
    r = lambda b: (b + 255) // 256 * 256      # noqa: E731
    n = 33 * 130
    assert influence.scratch_need(33, 130) == r(n) + r(4 * n)
    assert influence.scratch_need(33, 130, cells=False) == r(n) + 2 * r(4 * n)
    assert influence.scratch_need(33, 130, weighted=True) == r(n) + r(4 * n) + r(8 * n)
    assert influence.scratch_need(33, 130, weighted=True, value=True) == r(n) + r(4 * n)
    assert influence.scratch_need(33, 130, cells=False, weighted=True) == r(n) + 2 * r(4 * n) + r(8 * n)
    assert influence.scratch_need(1, 1) == 512 and influence.scratch_need(1024, 1024) == 5 << 20 == _bare_engine(H=1024, W=1024).influence_scratch_bytes()
    s = influence.InfluenceSpec(4, 33, 130, history=True, graph_on=True, arrival_on=True, cells=False, counts=True)
    assert s.need == influence.scratch_need(33, 130, cells=False)


def test_simulation_classes_refuse_bad_sources_before_anything_else():
    from simfire_amd.simulation import BatchedFireSimulation, _fire_influence
    eng = _bare_engine()
    for bad in (dict(source="graph"), dict(source="history", horizon=3.0), dict(source="history", max_minutes=5.0), dict(source="forecast", horizon=-1.0),
                dict(source="forecast", horizon=True), dict(source="forecast", pred=True), dict(source="forecast", envs=[0])):
        src = bad.pop("source")
        hor = bad.pop("horizon", None)
        with pytest.raises(ValueError, match="fire_influence"):
            _fire_influence(eng, src, None, None, None, False, None, 0, True, False, False, False, 0, hor, bad)
    for bad_inc in (np.ones((24, 40), dtype=np.uint8), [[1]]):       # (a host plane with a horizon: refused before the forecast is asked for)
        with pytest.raises(ValueError, match="fire_influence: include"):
            _fire_influence(eng, "forecast", None, None, bad_inc, False, None, 0, True, False, False, False, 0, 5.0, {})
    sim = BatchedFireSimulation.__new__(BatchedFireSimulation)
    sim._engine = eng
    with pytest.raises(ValueError, match="points or agents"):
        sim.fire_influence(points=np.zeros((4, 1, 3)), agents=True)
