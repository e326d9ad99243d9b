"""New episodes drawn on the device, the parts that need no GPU: the draw pinned by known words in two
restatements, its uniformity on one fixed input, the header / binding / exports, and a run of every GPU case's driver over
``oracle/fire_dense`` to check that the case sees what it claims to cover."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _episode_oracle as eo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KNOWN = [((0, 0, 0, 0), 0x48218226ff3cd4bf), ((1, 0, 0, 0), 0xdce423fc82c0d5b8), ((12345, 3, 7, 1), 0x3eb55f854bd585af),
         ((2 ** 64 - 1, 65534, 2 ** 32 - 1, 255), 0x64e9403bb683e737), ((42, 5, 1, 128), 0x76d14a26e97a06a9),
         ((42, 5, 1, 129), 0xcd5ccc83e0feb23c)]


def test_known_words():
    for args, want in KNOWN:
        assert eo.word_int(*args) == want, args
        assert int(eo.word(*args)) == want, args
    # vectorised over the slot, as the agents' start cells use it
    got = eo.word(42, 5, 1, np.array([128, 129], dtype=np.uint64))
    assert [int(v) for v in got] == [KNOWN[4][1], KNOWN[5][1]]
    # the derived integers and doubles
    x, y = eo.cell(eo.word(12345, 3, 7, 1), (10, 4, 29, 19))
    assert (int(x), int(y)) == (14, 8)
    w = 0x3eb55f854bd585af
    assert 10 + (((w >> 32) * 20) >> 32) == 14 and 4 + (((w & 0xFFFFFFFF) * 16) >> 32) == 8
    assert float(eo.to_double(eo.word(42, 5, 1, 128), 0.0, 360.0)) == 167.08716241836697
    assert float(eo.to_double(eo.word(42, 5, 1, 129), 0.0, 360.0)) == 288.7910095128228
    assert eo.wind(42, 5, 1, (0.0, 360.0), (0.0, 360.0)) == (167.08716241836697, 288.7910095128228)
    # plain-integer restatement of the double: (w >> 11) * 2^-53 is exact, the product and the sum round once each
    for slot, want in ((128, 167.08716241836697), (129, 288.7910095128228)):
        u = (eo.word_int(42, 5, 1, slot) >> 11) * 2.0 ** -53
        assert 0.0 + 360.0 * u == want
    # the ends of an integer range are reached and never left
    assert int(eo.to_int(0, 3, 9)) == 3 and int(eo.to_int(0xFFFFFFFF, 3, 9)) == 9 and int(eo.to_int(0xFFFFFFFF, 5, 5)) == 5


def test_uniformity_pin():
    """Seed 7, environments 0..4095, episodes 0..7, slot 0, the high half over 20 columns: 32 768 distinct words, every column hit
    between 1555 and 1718 times (expected 1638) - the values of exactly this input: a pin, not a statistical bar."""
    env = np.repeat(np.arange(4096, dtype=np.uint64), 8)
    ep = np.tile(np.arange(8, dtype=np.uint64), 4096)
    ws = eo.word(7, env, ep, 0)
    assert len(np.unique(ws)) == 32768
    counts = np.bincount(eo.to_int(ws >> np.uint64(32), 0, 19), minlength=20)
    assert len(counts) == 20 and counts.sum() == 32768
    assert counts.min() == 1555 and counts.max() == 1718, (counts.min(), counts.max())
    assert int(ws[8 * 3 + 7]) == eo.word_int(7, 3, 7, 0)


def test_ignition_loop_against_a_table():
    """The sequential loop: dead cells are skipped in attempt order; an all-dead box falls through to attempt 63's cell."""
    H, W, box = 12, 12, (2, 2, 9, 9)
    cells = [tuple(int(v) for v in eo.cell(eo.word(5, 1, 0, a), box)) for a in range(64)]
    rt = np.ones((8, H, W))
    assert eo.ignition(5, 1, 0, box, rt) == cells[0] + (0, False)
    assert eo.ignition(5, 1, 0, box, None) == cells[0] + (0, False)
    first_other = next(a for a in range(64) if cells[a] != cells[0])
    rt[:, cells[0][1], cells[0][0]] = 0.0
    assert eo.ignition(5, 1, 0, box, rt) == cells[first_other] + (first_other, False)
    rt[3, cells[0][1], cells[0][0]] = 2.5                     # one live direction is enough
    assert eo.ignition(5, 1, 0, box, rt) == cells[0] + (0, False)
    rt[:] = 0.0
    assert eo.ignition(5, 1, 0, box, rt) == cells[63] + (64, True)
    starts = eo.agent_starts(5, 1, 0, box, 3)
    assert [tuple(int(v) for v in s) for s in starts] == [tuple(int(v) for v in eo.cell(eo.word_int(5, 1, 0, 64 + j), box)) for j in range(3)]


def test_header_binding_and_exports():
    from simfire_amd import _lib
    header = open(os.path.join(ROOT, "include", "simfire_hip.h")).read()
    lib = _lib.load()
    for name, n_args in (("sf_episodes_set", 2), ("sf_episodes_begin", 3), ("sf_episodes_device", 4)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert len(_lib.SIGNATURES[name]) == n_args
        assert hasattr(lib, name)
    for word, value in (("SF_EP_IGNITION", 1), ("SF_EP_LIVE_CELL", 2), ("SF_EP_WIND", 4), ("SF_EP_AGENTS", 8)):
        assert re.search(r"#define\s+%s\s+%d\b" % (word, value), header), word
        assert getattr(_lib, word) == value
    assert C.sizeof(_lib.SfEpisodeParams) == 80
    assert re.search(r"typedef\s+struct\s+sf_episode_params\s*\{", header)
    # what is refused without a handle needs no device
    p = _lib.SfEpisodeParams(seed=1, flags=_lib.SF_EP_IGNITION)
    rc = lib.sf_episodes_set(None, C.byref(p))
    assert rc == _lib.SF_EINVAL and b"sf_episodes_set" in lib.sf_last_error()
    with pytest.raises(ValueError):
        _lib.check(rc)
    rc = lib.sf_episodes_begin(None, None, 1)
    assert rc == _lib.SF_EINVAL and b"sf_episodes_begin" in lib.sf_last_error()
    ptrs = [C.c_void_p() for _ in range(3)]
    rc = lib.sf_episodes_device(None, *[C.byref(q) for q in ptrs])
    assert rc == _lib.SF_EINVAL and b"sf_episodes_device" in lib.sf_last_error()


@pytest.mark.parametrize("case", list(eo.CASES))
def test_gpu_cases_see_what_they_claim(case):
    """The driver of tests/test_episodes_gpu.py over ``oracle/fire_dense`` (no handle B): at least 3 restarts per environment on
    average; in the ``live`` cases an attempt rejected as dead; where the ignition is drawn, two distinct ignitions within one
    environment's episodes (where only the wind is, two distinct winds and one ignition); the all-dead case falls through."""
    c = eo.CASES[case]
    world = eo.make_world(case)
    a = eo.DenseHandle(world)
    a.reset(world["inits"])
    seen = eo.drive(case, a, world)
    E = c["E"]
    assert seen["restarts"] >= 3 * E, seen["restarts"]
    assert sum(len(v) for v in seen["episodes"]) == seen["restarts"] and min(len(v) for v in seen["episodes"]) >= 1
    if c.get("live"):
        assert seen["rejected"] >= 1
    if "all_dead" in case:
        assert seen["fell"] == seen["restarts"] and seen["rejected"] == 64 * seen["restarts"]
        x0, y0, x1, y1 = c["ign_box"]
        for e in range(E):
            for i, (x, y, _, _) in enumerate(seen["episodes"][e]):
                assert (x, y) == tuple(int(v) for v in eo.cell(eo.word(c["seed"], e, i, 63), c["ign_box"]))
                assert x0 <= x <= x1 and y0 <= y <= y1
    else:
        assert seen["fell"] == 0
    if c.get("ign_box"):
        assert max(len({v[:2] for v in eps}) for eps in seen["episodes"]) >= 2
        if c.get("live") and "all_dead" not in case:
            assert all(world["R8"][:, y, x].any() for eps in seen["episodes"] for (x, y, _, _) in eps)
    else:
        assert all({v[:2] for v in eps} == {tuple(int(q) for q in world["inits"][e])} for e, eps in enumerate(seen["episodes"]))
    if c.get("wind"):
        (u0, u1), (d0, d1) = c["wind"]
        assert max(len({v[2:] for v in eps}) for eps in seen["episodes"]) >= 2
        assert all(u0 <= v[2] < u1 and d0 <= v[3] < d1 for eps in seen["episodes"] for v in eps)
