"""Reach of the fire without a device (``sf_reach``): the NumPy oracle against scipy's labelling, what the
hand-made scenes of ``tests/_reach_worlds.py`` claim, the superset property on the episode worlds with ``oracle/fire_dense`` standing in
for an engine, the ABI as the header and the binding state it, and the Python argument errors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _arrival_worlds as aw
import _reach_oracle as ro
import _reach_worlds as rw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((24, 40), (33, 17), (70, 1030), (72, 80), (136, 64))


# ---------------------------------------------------------------------------------------------- 1. the oracle
def _random_map(rng, H, W, lines):
    u = rng.random((H, W))
    m = np.where(u < lines, rng.integers(3, 6, size=(H, W)), 0)
    m = np.where((u >= lines) & (u < lines + 0.01), 1, m)
    m = np.where((u >= lines + 0.01) & (u < lines + 0.04), 2, m)
    return m.astype(np.uint8)


def test_oracle_equals_scipy_labelling():
    """R = the open cells of every connected component of the open cells that touches a seed (or a seed's neighbourhood)."""
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(2301)
    checked = 0
    for H, W in SHAPES:
        for lines in (0.1, 0.35, 0.55):
            m = _random_map(rng, H, W, lines)
            for src, thr in ((2, 1), (2, 1 | 56), (6, 1), (8, 1 | 4)):
                for conn in (4, 8):
                    got = ro.reach(m, src, thr, conn)
                    open_ = ro.selected(m, thr)
                    structure = np.ones((3, 3), dtype=bool) if conn == 8 else ndi.generate_binary_structure(2, 1)
                    lab, _ = ndi.label(open_, structure=structure)
                    touched = ndi.binary_dilation(ro.selected(m, src), structure=structure) & open_
                    want = np.isin(lab, np.unique(lab[touched])) & open_
                    assert (got == want).all(), (H, W, lines, src, thr, conn)
                    assert (ro.first_round(m, src, thr, conn) <= got).all()
                    checked += int(got.any() and not got.all())
    assert checked >= 100


def test_oracle_by_hand():
    m = np.array([[1, 0, 3, 0],
                  [0, 3, 0, 0],
                  [3, 0, 0, 2]], dtype=np.uint8)
    assert ro.reach(m, 2, 1, 4).astype(int).tolist() == [[0, 1, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0]]
    assert ro.reach(m, 2, 1, 8).astype(int).tolist() == [[0, 1, 0, 1], [1, 0, 1, 1], [0, 1, 1, 0]]
    assert ro.reach(m, 2, 1 | 8, 4).astype(int).tolist() == [[0, 1, 1, 1], [1, 1, 1, 1], [1, 1, 1, 0]]
    assert (ro.reach(m | 0xF8, 2, 1, 8) == ro.reach(m, 2, 1, 8)).all()               # only status & 7 counts
    p = np.ones((3, 4), dtype=np.uint8)
    p[1, 2] = 0
    assert ro.reach(m, 2, 1, 8, p).astype(int).tolist() == [[0, 1, 0, 1], [1, 0, 0, 1], [0, 1, 1, 0]]      # (round by (2, 1))
    p[2, 1] = 0
    assert ro.reach(m, 2, 1, 8, p).astype(int).tolist() == [[0, 1, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0]]
    r = ro.reach(m, 2, 1, 8)
    assert ro.count(r) == 7 and ro.seeds(m, 2) == 1 and ro.seeds(m, 8) == 3
    assert ro.value(r, np.arange(12).reshape(3, 4) - 5) == sum(v - 5 for v in (1, 3, 4, 6, 7, 9, 10))
    pts = np.array([[1, 0, 1], [0, 0, 1], [3, 2, 7], [1, 0, 0], [4, 0, 1], [0, -1, 1], [1, 0, -2], [1, 0, 1]])
    assert ro.point_in(r, pts).tolist() == [1, 0, 0, -1, -1, -1, -1, 1]


# ---------------------------------------------------------------------------------------------- 2. the scenes
def test_scenes_claim_what_the_oracle_says():
    names = set()
    for H, W in rw.SCENE_SHAPES:
        for s in rw.scenes(H, W):
            passable = rw.per_env_passable(3, H, W)[1] if isinstance(s["passable"], str) else s["passable"]
            r = ro.reach(s["map"], ro.mask_of(s["source"]), ro.mask_of(s["through"]), s["conn"], passable)
            if s["expect"] is not None:
                assert ro.count(r) == s["expect"], (H, W, s["name"], ro.count(r), s["expect"])
            names.add(s["name"])
            if s["name"] == "ring_closed":
                assert ro.point_in(r, s["points"]).tolist() == [0, 0, 0, 1]
            if s["name"] == "ring_open":
                assert ro.point_in(r, s["points"]).tolist() == [1, 1, 1, 1] and r.sum() == (s["map"] == 0).sum()
            if s["name"] == "no_seed":
                assert ro.seeds(s["map"], 2) == 0 and not r.any()
            if s["name"] == "nothing_open":
                assert ro.seeds(s["map"], 2) == 2 and not r.any()
            if s["name"].startswith("wall_to_the_last_column"):
                assert not r[H // 2:].any() and r[:H // 2].sum() == (H // 2) * W - 1
            if s["name"] == "points":
                assert {-1, 0, 1} <= set(ro.point_in(r, s["points"]).tolist()) | {0, 1}
    assert {"serpentine_h_4", "serpentine_v_8", "spiral_4", "diagonal_8", "diagonal_4", "ring_closed", "ring_open", "gaps_a_8", "gaps_b_4",
            "gaps_c_4", "wall_to_the_last_column_8", "borders", "no_seed", "nothing_open", "all_but_one", "passable_shared",
            "passable_per_env", "points", "lines_are_seeds"} <= names
    d = {s["name"]: s["expect"] for s in rw.scenes(9, 9)}
    assert (d["diagonal_8"], d["diagonal_4"]) == (71, 35)


# ---------------------------------------------------------------------------------------------- 3. the superset property
@pytest.mark.parametrize("case", rw.EPISODE_CASES)
def test_reach_is_a_superset_of_every_later_fire(case):
    """At every query point of the case's line-drawing mode: the reach through UNBURNED and the three lines, with the world's own
    connectivity, holds every cell that burns later (lines drawn after the query only shrink what burns).  Through UNBURNED alone
    the same is asserted where no line cell ever ignites - and the world is asserted to be one of those, or known to be one of the
    others: none is skipped silently."""
    kw, R8, E, inits = aw.make_world(case)
    H, W = kw["shape"]
    h = rw.StandIn(kw, R8, E)
    modes = aw.CASES[case]["modes"]
    mode = next(m for m in modes if rw.draws_lines(case, m))
    conn = 8 if kw["diagonal_spread"] else 4
    recorded = []

    def on_query(i, n, src, thr, c):
        for e in range(E):
            m = h.fire_map(e).copy()
            recorded.append((e, m, ro.reach(m, 2, 1 | 56, conn), ro.reach(m, 2, 1, conn)))
    # every UNBURNED cell that became a control line (a line written over a burning cell is no line that ignites: that cell turns
    # BURNED when its fire is pruned)
    line_cells = [np.zeros((H, W), dtype=bool) for _ in range(E)]
    draw = h.apply_mitigation

    def draw_and_note(rows):
        before = [h.fire_map(e).copy() for e in range(E)]
        draw(rows)
        for e in range(E):
            line_cells[e] |= (h.fire_map(e) >= 3) & (before[e] == 0)
    h.apply_mitigation = draw_and_note
    rw.run_episode(case, mode, h, inits, on_query, H, W)
    final = [h.fire_map(e).copy() for e in range(E)]
    for _ in range(400):                                        # to burn-out (or to the world's max_time: the maps stand still then)
        h.step(25)
        last, final = final, [h.fire_map(e).copy() for e in range(E)]
        if all((a == b).all() for a, b in zip(last, final)):
            break
    else:
        raise AssertionError((case, "still changing"))
    lines_held = all((final[e][line_cells[e]] >= 3).all() for e in range(E))
    assert lines_held == (not kw["attenuate_line_ros"] or case in LINES_HOLD_WITH_ATTENUATION), (case, kw["attenuate_line_ros"], lines_held)
    later = grew = 0
    for e, m, with_lines, unburned_only in recorded:
        burned_later = ((final[e] == 1) | (final[e] == 2)) & ~((m == 1) | (m == 2))
        assert (burned_later <= with_lines).all(), (case, e)
        if lines_held:
            assert (burned_later <= unburned_only).all(), (case, e)
        later += int(burned_later.sum())
        grew += int((with_lines & ~burned_later).sum())
    assert later > 0 and any(line_cells[e].any() for e in range(E))
    print(case, "lines held:", lines_held, "burned later:", later, "reach beyond the fire:", grew)


LINES_HOLD_WITH_ATTENUATION = ()       # worlds with attenuate_line_ros in which no line cell ignites all the same (none)


# ---------------------------------------------------------------------------------------------- 4. the ABI
def test_header_declares_and_lib_binds_reach():
    from simfire_amd import _lib
    text = open(os.path.join(ROOT, "include", "simfire_hip.h")).read()
    assert re.search(r"int\s+sf_reach\s*\(\s*sf_sim\s*\*\s*sim\s*,\s*const\s+sf_reach_params\s*\*\s*params\s*,\s*int32_t\s+n\s*,\s*"
                     r"const\s+int32_t\s*\*\s*envs[^,)]*,\s*const\s+sf_reach_out\s*\*\s*out\s*\)\s*;", text)
    assert re.search(r"typedef\s+struct\s+sf_reach_params\s*\{[^}]*int32_t\s+source_mask\s*,\s*through_mask\s*;[^}]*int32_t\s+connectivity\s*;"
                     r"[^}]*int32_t\s+k\s*;[^}]*int32_t\s+max_rounds\s*;[^}]*int32_t\s+passable_per_env\s*;[^}]*const\s+uint8_t\s*\*\s*passable\s*;"
                     r"[^}]*const\s+int32_t\s*\*\s*points\s*;[^}]*int64_t\s+scratch_bytes\s*;[^}]*int32_t\s+reserved\s*\[\s*2\s*\]\s*;[^}]*\}"
                     r"\s*sf_reach_params\s*;", text)
    assert re.search(r"typedef\s+struct\s+sf_reach_out\s*\{[^}]*int32_t\s*\*\s*count\s*;[^}]*int64_t\s*\*\s*value\s*;[^}]*uint8_t\s*\*\s*mask\s*;"
                     r"[^}]*int32_t\s*\*\s*seeds\s*;[^}]*int32_t\s*\*\s*point_in\s*;[^}]*int32_t\s*\*\s*rounds\s*;[^}]*\}\s*sf_reach_out\s*;", text)
    assert text.index("int sf_distance(") < text.index("Reach of the fire") < text.index("int sf_reach(") < text.index("Agents on the device")
    section = text[text.index("Reach of the fire"):text.index("int sf_reach(")]
    assert "no counterpart" in section and "upper bound, not a forecast" in section and "hipMalloc" in section
    P, O = _lib.SfReachParams, _lib.SfReachOut
    assert C.sizeof(P) == 56
    assert [(f[0], getattr(P, f[0]).offset) for f in P._fields_] == [
        ("source_mask", 0), ("through_mask", 4), ("connectivity", 8), ("k", 12), ("max_rounds", 16), ("passable_per_env", 20),
        ("passable", 24), ("points", 32), ("scratch_bytes", 40), ("reserved", 48)]
    assert C.sizeof(O) == 6 * C.sizeof(C.c_void_p) and [f[0] for f in O._fields_] == ["count", "value", "mask", "seeds", "point_in", "rounds"]
    assert "sf_reach" in _lib.SIGNATURES and len(_lib.SIGNATURES["sf_reach"]) == 5
    csrc = os.path.join(ROOT, "simfire_amd", "csrc")
    assert open(os.path.join(csrc, "simfire_hip.hip")).read().count('#include "sf_reach_kernels.h"') == 1
    # the step kernels and the other features do not know the new kernel
    for unit in sorted(os.listdir(csrc)):
        if unit.endswith((".hip", ".h")) and unit not in ("simfire_hip.hip", "sf_host_query.h", "sf_reach_kernels.h"):
            assert "k_reach" not in open(os.path.join(csrc, unit)).read(), unit
    kernels = open(os.path.join(csrc, "sf_reach_kernels.h")).read()
    assert "asm" not in re.sub(r"//[^\n]*", "", kernels)        # plain C++ only


def test_built_library_exports_sf_reach():
    from simfire_amd import _lib
    L = _lib.load()                        # (raises if the library has not been built)
    assert L.sf_reach.argtypes == _lib.SIGNATURES["sf_reach"]
    p = _lib.SfReachParams(source_mask=2, through_mask=1)
    o = _lib.SfReachOut(count=16)
    e = np.zeros(1, dtype=np.int32)
    assert L.sf_reach(None, C.byref(p), 1, e.ctypes.data_as(C.c_void_p), C.byref(o)) == _lib.SF_EINVAL
    assert b"sf_reach" in L.sf_last_error()


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
    eng.values_on = False
    return eng


@pytest.mark.parametrize("kw", [
    dict(source=0), dict(source=64), dict(source=()), dict(source=("SMOULDERING",)), dict(source=(6,)), dict(source=None), dict(source=True),
    dict(through=0), dict(through=64), dict(through=(1.0,)), dict(through=None),
    dict(source=("BURNING",), through=("BURNING", "UNBURNED")), dict(source=3, through=1),
    dict(connectivity=6), dict(connectivity=-4), dict(connectivity=8.0), dict(connectivity=True), dict(connectivity="8"),
    dict(max_rounds=-1), dict(max_rounds=1.5), dict(max_rounds=2 ** 31), dict(scratch_bytes=-1), dict(scratch_bytes=1.5), dict(scratch_bytes=1),
    dict(envs=[4]), dict(envs=[-1]), dict(envs=[[0, 1]]), dict(envs=[0.0]),
    dict(count=False), dict(count=1), dict(mask="yes"), dict(value=True),
    dict(points=np.zeros((4, 2, 3), dtype=np.int32)), dict(passable=np.ones((24, 40), dtype=np.uint8)),
])
def test_python_argument_errors(kw):
    eng = _bare_engine()
    with pytest.raises(ValueError, match="reach"):
        eng.reach(**kw)


def test_request_forms_and_shared_mask_parsing():
    from simfire_amd.engine import FireEngine
    from simfire_amd.enums import BurnStatus
    req = FireEngine._reach_request
    assert req() == (2, 1, 0, 0, 0)
    assert req(("BURNING", "BURNED"), ("UNBURNED",) + ro.LINES, 8, 3, 4096) == (6, 1 | 56, 8, 3, 4096)
    assert req(BurnStatus.FIRELINE, [BurnStatus.UNBURNED, 2], connectivity=4)[:3] == (8, 5, 4)
    assert req(np.int64(2), 57)[:2] == (2, 57)
    for src, thr in rw.MASK_PAIRS:
        assert req(src, thr)[:2] == (ro.mask_of(src), ro.mask_of(thr))
    # distance and reach parse their masks with the same function
    assert FireEngine._status_mask("distance", ("BURNING", 2)) == 6 == FireEngine._distance_request(("BURNING", 2))[0]
    with pytest.raises(ValueError, match="^reach: "):
        FireEngine._status_mask("reach", ("EMBERS",))
    eng = _bare_engine(H=1024, W=1024)
    assert eng.reach_scratch_bytes() == 64 * 16 * (16 * 16 + 20)
    assert _bare_engine(H=33, W=17).reach_scratch_bytes() == (3 * (16 * 16 + 20) + 255) // 256 * 256


def test_batched_fire_env_refuses_a_bad_reach_option():
    from simfire_amd.vecenv import BatchedFireEnv

    class _Sim:
        n_envs = 2
        _engine = _bare_engine(E=2)
    for bad in (dict(radius=3), dict(source=("EMBERS",)), dict(source=("BURNING",), through=("BURNING",)), dict(connectivity=5), dict(value=1),
                dict(value=True), "on"):
        with pytest.raises(ValueError, match="reach"):
            BatchedFireEnv(_Sim(), 1, np.zeros((1, 2), dtype=np.int32), reach=bad)
