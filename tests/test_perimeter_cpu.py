"""Fire perimeters without a device (``sf_perimeter``): the tracer of ``tests/_perimeter_oracle.py`` against
``scipy.ndimage.label`` and its own invariants, what the hand-made scenes of ``tests/_perimeter_worlds.py`` are there for, the ABI as
the header and the binding state it, the Python argument errors, and ``rings``."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _perimeter_oracle as po
import _perimeter_worlds as pw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- 1. the oracle
def test_oracle_against_scipy_label():
    """400 random masks up to 11 x 11, both connectivities: the outer loops are the c-connected components of the set, the holes the
    (12 - c)-connected components of the padded complement minus the outside.  (Every edge in exactly one loop, the areas adding up
    to |S| and the edge count are the oracle's own assertions: they run on every call.)"""
    pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(2701)
    differ = 0
    for i in range(400):
        H, W = int(rng.integers(1, 12)), int(rng.integers(1, 12))
        S = rng.random((H, W)) < rng.choice([0.2, 0.5, 0.8])
        got = {}
        for conn in (4, 8):
            a = po.answer(S, conn)
            outer, holes = po.components(S, conn)
            assert (a["loops"] - a["holes"], a["holes"]) == (outer, holes), (i, conn, S.astype(int).tolist())
            assert a["cells"] == int(S.sum()) and int(a["loop_area"].sum()) == a["cells"] and int(a["loop_edges"].sum()) == a["edges"]
            assert a["loop_start"][0] == 0 and a["loop_start"][-1] == a["n_vertices"] == len(a["vertices"])
            full = po.answer(S, conn, simplify=False)
            assert full["n_vertices"] == full["edges"] and (np.diff(full["loop_start"]) == full["loop_edges"]).all()
            assert (full["loop_area"] == a["loop_area"]).all() and full["loops"] == a["loops"]
            got[conn] = a
        differ += got[4]["loops"] != got[8]["loops"]
        assert got[4]["edges"] == got[8]["edges"] and (got[4]["front"] == got[8]["front"]).all()
    assert differ > 50                                        # the two successor rules really differ


def test_the_smallest_answers_by_hand():
    a = po.answer(np.ones((1, 1), dtype=bool), 4)
    assert a["vertices"].tolist() == [[0, 0], [1, 0], [1, 1], [0, 1]] and a["loop_area"].tolist() == [1]      # E, S, W, N: clockwise on the screen
    assert (a["edges"], a["cells"], a["loops"], a["holes"], a["front"].tolist()) == (4, 1, 1, 0, [[1]])
    ring = pw.one_cell_hole(3, 3)
    a = po.answer(ring, 4)
    assert a["loop_area"].tolist() == [9, -1] and a["holes"] == 1 and a["loop_edges"].tolist() == [12, 4]
    assert a["vertices"][4:].tolist() == [[1, 1], [1, 2], [2, 2], [2, 1]]                                      # the hole runs the other way round
    assert a["front"].sum() == 8
    # a saddle: two cells that touch at a corner are two loops under 4 and one loop under 8
    S = np.array([[1, 0], [0, 1]], dtype=bool)
    a4, a8 = po.answer(S, 4), po.answer(S, 8)
    assert (a4["loops"], a8["loops"]) == (2, 1) and a8["loop_edges"].tolist() == [8] and a8["n_vertices"] == 8
    assert a8["vertices"].tolist() == [[0, 0], [1, 0], [1, 1], [2, 1], [2, 2], [1, 2], [1, 1], [0, 1]]
    # ... and a hole whose corner touches the outside is cut off from it under 4 only when the set's cells are joined diagonally
    e = po.answer(np.zeros((3, 4), dtype=bool), 8)
    assert (e["edges"], e["loops"], e["n_vertices"]) == (0, 0, 0) and e["loop_start"].tolist() == [0] and e["vertices"].shape == (0, 2)


def test_scenes_are_what_they_are_there_for():
    H, W = 17, 65
    sc = {s["name"]: s["mask"] for s in pw.scenes(H, W)}
    assert {"empty", "full", "corner_cell", "one_cell_hole", "nested_rings", "saddle_pair", "checkerboard", "serpentine", "spiral", "four_borders",
            "run_to_word_boundary", "band_rows", "random_0", "random_1", "random_2"} == set(sc)
    a = {k: (po.answer(m, 4), po.answer(m, 8)) for k, m in sc.items()}
    assert a["empty"][0]["edges"] == 0 and a["full"][0]["edges"] == 2 * (H + W) and a["full"][0]["n_vertices"] == 4
    assert a["corner_cell"][0]["vertices"].tolist() == [[W - 1, H - 1], [W, H - 1], [W, H], [W - 1, H]]
    assert a["nested_rings"][0]["holes"] >= 4 and a["nested_rings"][0]["loops"] == a["nested_rings"][0]["holes"] * 2 + 1
    assert a["saddle_pair"][0]["loops"] > a["saddle_pair"][1]["loops"] and a["saddle_pair"][1]["holes"] == 1
    assert a["checkerboard"][0]["holes"] == 0 and a["checkerboard"][1]["loops"] - a["checkerboard"][1]["holes"] == 1
    for k in ("serpentine", "spiral"):
        assert a[k][0]["loops"] == a[k][1]["loops"] == 1 and a[k][0]["edges"] > 1000
    m = sc["four_borders"]
    assert m[0].any() and m[-1].any() and m[:, 0].any() and m[:, -1].any()
    m = sc["run_to_word_boundary"]
    assert m[0, 63] and not m[0, 64] and m[2, 64] and not m[2, 63] and m[4, 63] and m[4, 64]
    m = sc["band_rows"]
    assert m[15, 1] and not m[16, 1] and m[16, W // 2] and not m[17:, W // 2].any() and (a["band_rows"][0]["loops"], a["band_rows"][1]["loops"]) == (3, 2)
    assert [round(float(sc["random_%d" % k].mean()), 1) for k in range(3)] == [0.1, 0.5, 0.9]
    assert po.answer(pw.checkerboard(64, 64), 4)["loops"] == 2048
    # the map a scene is loaded as: BURNING | BURNED is the mask, both occur, and there are lines among the rest
    fm = pw.fire_map(sc["random_1"])
    assert (po.mask_of_status(fm, 6) == sc["random_1"]).all() and {0, 1, 2, 3} == set(np.unique(fm).tolist())
    arr = np.array([[-1, 0, 3], [5, 12, -1]])
    assert po.mask_of_arrival(arr, 3).tolist() == [[False, True, True], [False, False, False]]


# ---------------------------------------------------------------------------------------------- 2. the ABI
def test_header_declares_and_lib_binds_perimeter():
    from simfire_amd import _lib
    text = open(os.path.join(ROOT, "include", "simfire_hip.h")).read()
    assert re.search(r"int\s+sf_perimeter\s*\(\s*sf_sim\s*\*\s*sim\s*,\s*const\s+sf_perimeter_params\s*\*\s*params\s*,\s*int32_t\s+n\s*,\s*"
                     r"const\s+int32_t\s*\*\s*envs[^,)]*,\s*const\s+sf_perimeter_out\s*\*\s*out\s*\)\s*;", text)
    assert re.search(r"typedef\s+struct\s+sf_perimeter_params\s*\{[^}]*int32_t\s+status_mask\s*;[^}]*int32_t\s+at_update\s*;[^}]*int32_t\s+connectivity\s*;"
                     r"[^}]*int32_t\s+simplify\s*;[^}]*int32_t\s+member_per_env\s*;[^}]*int32_t\s+max_edges\s*,\s*max_vertices\s*,\s*max_loops\s*;"
                     r"[^}]*const\s+uint8_t\s*\*\s*member\s*;[^}]*int64_t\s+scratch_bytes\s*;[^}]*int32_t\s+reserved\s*\[\s*2\s*\]\s*;[^}]*\}\s*sf_perimeter_params\s*;", text)
    assert re.search(r"typedef\s+struct\s+sf_perimeter_out\s*\{[^}]*int32_t\s*\*\s*edges\s*,\s*\*\s*cells\s*;[^}]*uint8_t\s*\*\s*front\s*;"
                     r"[^}]*int32_t\s*\*\s*loops\s*,\s*\*\s*holes\s*,\s*\*\s*n_vertices\s*;[^}]*int32_t\s*\*\s*vertices\s*;[^}]*int32_t\s*\*\s*loop_start\s*;"
                     r"[^}]*int32_t\s*\*\s*loop_area\s*,\s*\*\s*loop_edges\s*;[^}]*\}\s*sf_perimeter_out\s*;", text)
    # the new section stands behind sf_behavior and uses none of the other sections' titles
    assert text.index("int sf_behavior(") < text.index("Perimeters of the fire") < text.index("int sf_perimeter(") < text.index("Agents on the device")
    section = text[text.index("Perimeters of the fire"):text.index("int sf_perimeter(")]
    for title in ("Fire travel time", "Walking distance", "Fire behaviour per cell", "Reach of the fire", "Distance fields"):
        assert title not in section, title
    for words in ("right cell is in S and its left cell is not", "smallest-id edge", "never by a failure of the call", "hipMalloc",
                  "8 * height * ceil(width / 64) + 12 * (height + 1) * ceil((width + 1) / 16)"):
        assert words in re.sub(r"\s*\n \* ", " ", section), words
    P, O = _lib.SfPerimeterParams, _lib.SfPerimeterOut
    assert C.sizeof(P) == 56
    assert [(f[0], getattr(P, f[0]).offset) for f in P._fields_] == [
        ("status_mask", 0), ("at_update", 4), ("connectivity", 8), ("simplify", 12), ("member_per_env", 16), ("max_edges", 20),
        ("max_vertices", 24), ("max_loops", 28), ("member", 32), ("scratch_bytes", 40), ("reserved", 48)]
    assert C.sizeof(O) == 10 * C.sizeof(C.c_void_p)
    assert [f[0] for f in O._fields_] == ["edges", "cells", "front", "loops", "holes", "n_vertices", "vertices", "loop_start", "loop_area", "loop_edges"]
    assert "sf_perimeter" in _lib.SIGNATURES and len(_lib.SIGNATURES["sf_perimeter"]) == 5
    from simfire_amd import perimeter
    assert perimeter.TRACED == tuple(f[0] for f in O._fields_[3:])


def test_kernels_are_included_once_and_named_by_nobody_else():
    csrc = os.path.join(ROOT, "simfire_amd", "csrc")
    assert open(os.path.join(csrc, "simfire_hip.hip")).read().count('#include "sf_perimeter_kernels.h"') == 1
    for unit in sorted(os.listdir(csrc)):
        if unit.endswith((".hip", ".h")) and unit not in ("sf_host_query.h", "sf_perimeter_kernels.h"):
            assert "k_perim" not in open(os.path.join(csrc, unit)).read(), unit
    kernels = open(os.path.join(csrc, "sf_perimeter_kernels.h")).read()
    assert kernels.count("__global__") == 2 and "k_perim_summary" in kernels and "k_perim_trace" in kernels
    assert "asm" not in re.sub(r"//[^\n]*", "", kernels)        # plain C++ only
    for other in ("k_walk", "k_reach", "k_dist_", "k_travel", "k_behavior", "k_ensemble", "k_run", "k_step"):
        assert other not in kernels, other
    host = open(os.path.join(csrc, "sf_host_query.h")).read()
    assert 'extern "C" int sf_perimeter(' in host and "k_perim_summary" in host and "k_perim_trace" in host
    assert re.search(r"QueryState [^;]*\bperimeter\b[^;]*;", open(os.path.join(csrc, "sf_handle.h")).read())


def test_built_library_exports_sf_perimeter():
    """Fails on a library built without the feature."""
    from simfire_amd import _lib
    L = _lib.load()                        # (raises if the library has not been built)
    assert L.sf_perimeter.argtypes == _lib.SIGNATURES["sf_perimeter"]
    p = _lib.SfPerimeterParams(status_mask=6, at_update=-1)
    o = _lib.SfPerimeterOut(edges=16)
    e = np.zeros(1, dtype=np.int32)
    assert L.sf_perimeter(None, C.byref(p), 1, e.ctypes.data_as(C.c_void_p), C.byref(o)) == _lib.SF_EINVAL
    assert b"sf_perimeter" in L.sf_last_error()


# ------------------------------------------------------------------------- 3. errors before any library call
class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called: {name}")


def _bare_engine(E=4, H=24, W=40, arrival=False):
    from simfire_amd.engine import FireEngine
    eng = FireEngine.__new__(FireEngine)
    eng._L, eng._h = _NoDevice(), None
    eng.n_envs, eng.H, eng.W = E, H, W
    eng.async_mode, eng._blobs_in_flight = False, []
    eng.arrival_on = arrival
    return eng


@pytest.mark.parametrize("kw", [
    dict(status=0), dict(status=64), dict(status=()), dict(status=("SMOULDERING",)), dict(status=(6,)), dict(status=True), dict(status=(1.0,)),
    dict(at_update=-1), dict(at_update=1.5), dict(at_update=True), dict(at_update="3"), dict(at_update=3),      # (3: recording is off)
    dict(status=6, at_update=3), dict(status=("BURNING",), member=np.ones((24, 40), dtype=np.uint8)),
    dict(member=np.ones((24, 40), dtype=np.uint8)), dict(member=[[1]]),
    dict(connectivity=6), dict(connectivity=-4), dict(connectivity=8.0), dict(connectivity=True), dict(connectivity="8"),
    dict(simplify=1), dict(simplify=None), dict(counts=0), dict(front="yes"), dict(trace=1), dict(counts=False),
    dict(max_edges=-1), dict(max_edges=1.5), dict(max_vertices=-2), dict(max_loops=-1), dict(max_loops=True),
    dict(trace=True, max_vertices=0), dict(trace=True, max_loops=0), dict(trace=True, max_edges=3),      # (3 // 4 loops: none)
    dict(scratch_bytes=-1), dict(scratch_bytes=1.5), dict(trace=True, scratch_bytes=1),
    dict(envs=[4]), dict(envs=[-1]), dict(envs=[[0, 1]]), dict(envs=[0.0]),
])
def test_python_argument_errors(kw):
    eng = _bare_engine()
    with pytest.raises(ValueError, match="perimeter"):
        eng.perimeter(**kw)


def test_python_refuses_a_grid_too_wide_and_at_update_passes_with_recording():
    from simfire_amd.perimeter import PerimeterSpec
    with pytest.raises(ValueError, match="8192"):
        _bare_engine(W=8200).perimeter()
    s = PerimeterSpec(4, 24, 40, at_update=3, arrival_on=True)
    assert (s.status, s.at_update) == (0, 3) and list(s.outputs) == ["edges", "cells"]
    with pytest.raises(ValueError, match="arrival"):
        PerimeterSpec(4, 24, 40, at_update=3, arrival_on=False)


def test_request_forms_capacities_and_scratch_need():
    from simfire_amd import perimeter
    from simfire_amd.enums import BurnStatus
    assert perimeter.request() == (6, -1, 0, 1, 0)
    assert perimeter.request(("BURNING",), None, 8, False, 4096) == (2, -1, 8, 0, 4096)
    assert perimeter.request([BurnStatus.BURNED, 3], connectivity=4)[:3] == (12, -1, 4)
    assert perimeter.request(at_update=0)[:2] == (0, 0) and perimeter.request(member=True)[:2] == (0, -1)
    assert perimeter.request(np.int64(63))[0] == 63
    with pytest.raises(ValueError, match="^perimeter: "):
        perimeter.request(("EMBERS",))
    assert perimeter.default_capacities(1024, 1024) == (1 << 18, 1 << 18, 1 << 16)
    assert perimeter.default_capacities(3, 5) == (32, 32, 8) and perimeter.default_capacities(3, 5, 100, None, 7) == (100, 100, 7)
    # the formula as the header states it
    assert perimeter.scratch_need(33, 130, 1000) == (8 * 33 * 3 + 12 * 34 * 9 + 32 * 1000 + 255) // 256 * 256
    assert perimeter.scratch_need(1024, 1024, 1 << 18) == 8 * 1024 * 16 + 12 * 1025 * 65 + 32 * (1 << 18) + 244 == 9319424 == _bare_engine(H=1024, W=1024).perimeter_scratch_bytes()
    assert perimeter.scratch_need(1, 1, 0) == 256
    spec = perimeter.PerimeterSpec(4, 24, 40, envs=[3, 0, 3], front=True, trace=True, max_edges=500, max_loops=9)
    assert spec.outputs == dict(edges=((3,), "int32"), cells=((3,), "int32"), front=((3, 24, 40), "uint8"), loops=((3,), "int32"), holes=((3,), "int32"),
                                n_vertices=((3,), "int32"), vertices=((3, 500, 2), "int32"), loop_start=((3, 10), "int32"),
                                loop_area=((3, 9), "int32"), loop_edges=((3, 9), "int32"))
    p = spec.params()
    assert (p.status_mask, p.at_update, p.connectivity, p.simplify, p.member_per_env, p.max_edges, p.max_vertices, p.max_loops, p.member, p.scratch_bytes) == \
        (6, -1, 0, 1, 0, 500, 500, 9, None, 0) and spec.need == perimeter.scratch_need(24, 40, 500)
    assert list(perimeter.PerimeterSpec(4, 24, 40, counts=False, front=True).outputs) == ["front"]


def test_rings():
    from simfire_amd.perimeter import rings
    S = np.zeros((4, 6), dtype=bool)
    S[0:3, 0:3] = True
    S[1, 1] = False
    S[3, 5] = True
    a = po.answer(S, 4)
    cap_v, cap_l = 20, 5
    v = np.full((cap_v, 2), -9, dtype=np.int32)
    v[:a["n_vertices"]] = a["vertices"]
    st = np.zeros(cap_l + 1, dtype=np.int32)
    st[:a["loops"] + 1] = a["loop_start"]
    ar = np.full(cap_l, 7, dtype=np.int32)
    ar[:a["loops"]] = a["loop_area"]
    got = rings(v, st, ar)
    assert len(got) == 3 and [hole for _, hole in got] == [False, True, False]
    assert got[0][0].tolist() == [[0, 0], [3, 0], [3, 3], [0, 3]] and got[1][0].tolist() == [[1, 1], [1, 2], [2, 2], [2, 1]]
    assert got[2][0].tolist() == [[5, 3], [6, 3], [6, 4], [5, 4]]
    assert [g[0].tolist() for g in rings(v, st, ar, loops=2)] == [g[0].tolist() for g in got[:2]]
    assert rings(v, np.zeros(cap_l + 1, dtype=np.int32), ar) == [] and rings(v, st, ar, loops=0) == []      # an answer that did not fit
    got[0][0][0, 0] = 99
    assert v[0, 0] == 0                                       # copies, not views
    for bad in ((v[:, :1], st, ar), (v, st[:-1], ar), (v.ravel(), st, ar)):
        with pytest.raises(ValueError, match="rings"):
            rings(*bad)


def test_simulation_classes_refuse_a_bad_unit_before_anything_else():
    from simfire_amd.simulation import FireSimulation, _perimeter_unit
    sim = FireSimulation.__new__(FireSimulation)
    sim._engine = _bare_engine()
    with pytest.raises(ValueError, match="unit"):
        sim.perimeter(unit="m")
    assert _perimeter_unit("cells", 30.0) == 1.0 and _perimeter_unit("ft", 30.0) == 30.0


def test_batched_fire_env_refuses_a_bad_perimeter_option():
    from simfire_amd.vecenv import BatchedFireEnv

    class _Sim:
        n_envs = 2
        _engine = _bare_engine(E=2)
    for bad in (dict(radius=3), dict(status=("EMBERS",)), dict(status=()), dict(status=0), "on"):
        with pytest.raises(ValueError, match="perimeter"):
            BatchedFireEnv(_Sim(), 1, np.zeros((1, 2), dtype=np.int32), perimeter=bad)
