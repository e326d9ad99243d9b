"""Arrival times without a GPU: the mask decode against brute force, ``arrival_from_maps`` against the sprite oracle on the golden
trajectories, the inputs of every case of ``tests/test_arrival_gpu.py`` (run on ``oracle/fire_dense``), and the declared ABI."""
import glob
import os
import re

import numpy as np
import pytest

import _golden
from _arrival_oracle import arrival_from_maps, decode_masks, slot_of
from _arrival_worlds import CASES, PAIRS, DenseStandIn, drive, make_world
from oracle import fire_sprites

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------- 1. the decode
def _brute(md, T, every, rng, n_cells=40):
    """Sprites (cell, s) aged by hand: sprite s is in its cell's mask - bit slot_of(s, md + 3) - from update s until the update
    s + md + 2 recycles the slot (sf_common.h: set at s, live through s + md, pruned at s + md + 1, cleared at s + md + 2).  A pass
    every ``every`` updates.  Returns (true first arrival per cell, recorded arrival1)."""
    N = md + 3
    sprites = [(0, 0)]                                    # the reset's ignition: the sprite of update 0
    first = np.full(n_cells, -1, dtype=np.int64)
    first[0] = 0
    arrival1 = np.zeros(n_cells, dtype=np.int64)
    for t in range(0, T + 1):
        if t > 0:
            for c in rng.choice(n_cells, size=int(rng.integers(0, 4)), replace=False):
                # a cell ignites again only after a control line made it eligible: while its sprite lives or later
                sprites.append((int(c), t))
                if first[c] < 0:
                    first[c] = t
        masks = np.zeros(n_cells, dtype=np.int64)
        for c, s in sprites:
            if s <= t < s + md + 2:
                masks[c] |= 1 << slot_of(s, N)
        if t % every == 0 or t == T:
            # every sprite ignited in the last md updates is named exactly
            probe = np.zeros(n_cells, dtype=np.int64)
            decode_masks(masks, t, md, probe)
            for c, s in sprites:
                if t - md <= s <= t:
                    oldest = min(s2 for c2, s2 in sprites if c2 == c and t - md <= s2 <= t)
                    assert probe[c] == oldest + 1, (md, t, c, s, int(probe[c]))
            decode_masks(masks, t, md, arrival1)
    return first, arrival1


@pytest.mark.parametrize("md", [1, 2, 3, 4, 5, 8, 13, 28])
def test_decode_against_brute_force(md):
    rng = np.random.default_rng(500 + md)
    T = 3 * (md + 3)
    missed_late = 0
    for rep in range(6):
        first, got = _brute(md, T, md, rng)
        assert (got - 1 == first).all(), (md, rep, np.flatnonzero(got - 1 != first)[:5])
        # negative control: a pass every md + 3 updates comes back after the slots have been recycled (the closing pass at T is
        # the only other one)
        first, got = _brute(md, T, md + 3, rng)
        missed_late += int((got - 1 != first).sum())
    assert missed_late > 0, md


def test_decode_every_t_up_to_three_rounds():
    """every t up to 3 (md + 3): a single sprite per cell, one cell per update, a pass wherever t is a multiple of md"""
    for md in (1, 2, 3, 4, 5, 8, 13, 28):
        N, T = md + 3, 3 * (md + 3)
        arrival1 = np.zeros(T + 1, dtype=np.int64)
        for t in range(T + 1):
            masks = np.zeros(T + 1, dtype=np.int64)
            for s in range(t + 1):                              # cell s ignites at update s
                if t < s + md + 2:
                    masks[s] |= 1 << slot_of(s, N)
            if t % md == 0 or t == T:
                decode_masks(masks, t, md, arrival1)
        assert (arrival1 == np.arange(T + 1) + 1).all(), md


# ------------------------------------------------------------------------ 2. golden trajectories, sprite oracle
def _traj_files():
    return sorted(os.path.basename(f) for f in glob.glob(os.path.join(ROOT, "tests", "golden", "traj_g*.npz")))


@pytest.mark.parametrize("name", _traj_files())
def test_arrival_from_maps_on_golden_trajectory(name):
    """The fixtures hold the reference's map after every update (``fire_maps[s]`` = after update s + 1) and the control lines drawn in
    front of each (``schedule`` rows (s, x, y, type)), not the map after the reset: that one is the ignition cell alone."""
    d = _golden.load(name)
    kw = _golden.engine_kwargs(d)
    H, W = kw["shape"]
    x0, y0 = (int(v) for v in d["init_pos"])
    f = fire_sprites.SpriteFire(kw["shape"], d["init_pos"], kw["max_fire_duration"], kw["pixel_scale"], kw["update_rate"],
                                rtable=d["rtable"], max_time=kw["max_time"], attenuate_line_ros=kw["attenuate_line_ros"],
                                diagonal_spread=kw["diagonal_spread"])
    fm = np.zeros((H, W), dtype=np.int64)
    fm[y0, x0] = 1
    first = np.full((H, W), -1, dtype=np.int32)
    first[y0, x0] = 0
    created = {(x0, y0): [0]}
    running = True
    sched = d["schedule"]
    for s in range(len(d["status"])):
        pts = sched[sched[:, 0] == s]
        fire_sprites.apply_mitigation(fm, [(int(x), int(y), int(t)) for (_, x, y, t) in pts])
        if running:
            fm, st = f.update(fm)
            running = st == fire_sprites.RUNNING
            for (x, y), dur in zip(f.sprites, f.durations):          # the sprites this update created
                if dur == 0 and created.get((x, y), [None])[-1] != s + 1:
                    created.setdefault((x, y), []).append(s + 1)
                    if first[y, x] < 0:
                        first[y, x] = s + 1
        assert (fm == d["fire_maps"][s]).all(), (name, s)
    start = np.zeros((H, W), dtype=np.uint8)
    start[y0, x0] = 1
    got = arrival_from_maps([start] + list(d["fire_maps"]))
    assert (got == first).all(), name
    assert (got >= 0).sum() > 1, name
    if name == "traj_g4_lines_on_burning.npz":
        again = [(c, v) for c, v in created.items() if len(v) > 1]
        assert again, "no cell ignited twice"
        for (x, y), v in again:
            assert got[y, x] == v[0] < v[1]


# ------------------------------------------------------------------------------ 3. the inputs of the GPU cases
_seen = {}


def _see(case):
    if case not in _seen:
        kw, R8, E, _ = make_world(case)
        _seen[case] = drive(case, CASES[case]["modes"][0], DenseStandIn(kw, R8, E))
    return _seen[case]


@pytest.mark.parametrize("case", list(CASES))
def test_case_sees_what_it_claims(case):
    c = CASES[case]
    seen = _see(case)
    md = c.get("md", 4)
    assert seen["cells"] >= 50, seen["cells"]
    assert seen["span"] > 3 * md, seen["span"]
    ops = c.get("ops", {})
    if any(op[0].startswith("reset") for op in ops.values()):
        assert seen["reset_after_arrivals"] >= 1
        assert [o for o in seen["ops"] if isinstance(o, tuple) and o[0] == "not running" and o[1] >= 1], "reset_where() found every environment running"
    if c.get("lines"):
        assert seen["on_burning"] >= 1
    if c.get("late"):
        live = [o for o in seen["ops"] if isinstance(o, tuple) and o[0] == "live at enable"][0]
        assert live[1] >= 2 and live[3] >= 5, live          # sprites live at the moment of enabling, and cells burned out before it


def test_cases_cover_the_modes():
    from test_env_state_gpu import MODES
    assert {m for _, m in PAIRS} >= set(MODES)


# ---------------------------------------------------------------------------------------------- 4. the ABI
def test_header_declares_and_lib_binds_arrival():
    from simfire_amd import _lib
    text = open(os.path.join(ROOT, "include", "simfire_hip.h")).read()
    decl = {"sf_enable_arrival": r"int\s+sf_enable_arrival\s*\(\s*sf_sim\s*\*\s*sim\s*,\s*int32_t\s+on\s*\)\s*;",
            "sf_get_arrival": r"int\s+sf_get_arrival\s*\(\s*sf_sim\s*\*\s*sim\s*,\s*int32_t\s+env\s*,\s*int32_t\s*\*\s*out[^)]*\)\s*;",
            "sf_arrival_device": r"int\s+sf_arrival_device\s*\(\s*sf_sim\s*\*\s*sim\s*,\s*void\s*\*\*\s*ptr\s*,\s*int64_t\s*\*\s*row_pitch\s*,"
                                 r"\s*int64_t\s*\*\s*env_stride\s*\)\s*;"}
    for name, pat in decl.items():
        assert re.search(pat, text), f"include/simfire_hip.h does not declare {name}"
        assert name in _lib.SIGNATURES, f"simfire_amd/_lib.py does not bind {name}"
    assert len(_lib.SIGNATURES["sf_enable_arrival"]) == 2
    assert len(_lib.SIGNATURES["sf_get_arrival"]) == 3
    assert len(_lib.SIGNATURES["sf_arrival_device"]) == 4
    assert "fire.py:571-587" in text[text.index("Arrival times"):text.index("int sf_enable_arrival")]
