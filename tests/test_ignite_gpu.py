"""Ignitions during an episode on the GPU (``sf_ignite`` / ``sf_ignite_device``).  The yardstick is the
sprite-list oracle with the canonical insertion (``tests/_ignite_oracle.py``, pinned against the real reference by
``tests/golden/ignite_*.npz``), one per environment, fed the device's own table (``get_rtable``): maps, status rows, elapsed times
and burn amounts are compared bit for bit.  Run with ``pytest -m gpu``."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

import _ignite_oracle
from test_ignite_cpu import FIXTURES, load

pytestmark = pytest.mark.gpu

CFG = os.path.join(os.path.dirname(__file__), "golden", "configs")
MODES = {
    "fused0": dict(fused=0, kind=0),
    "fused1": dict(fused=1, kind=1),
    "cells2": dict(fused=-1, md=7, kind=3),                                       # sprite masks of two bytes: the per-cell kernel
    "cells4": dict(fused=-1, md=14, kind=3),                                      # ... of four
    "run_win": dict(fused=2, tuning=dict(run_window=3), kind=2),                  # the resident launch with its window phase
    "run_loop": dict(fused=2, tuning=dict(run_window=0), kind=2),                 # the general loop alone
    "run_team": dict(fused=2, tuning=dict(run_team=2), kind=2),                   # every environment split into two workgroups
    "run_kwin": dict(fused=-1, tuning=dict(run_compact=2, run_window=1), kind=4),  # k_win in front of k_run (the automatic choice only)
}


def table(rng, H, W):
    """An R table whose fires go on for many updates around cells that never burn."""
    R8 = rng.choice([3.0, 7.5, 12.0, 30.0, 400.0, 1200.0], size=(8, H, W))
    R8 = np.maximum(R8, 12.0)
    R8[:, rng.random((H, W)) < 0.08] = 0.0
    return R8


class Pair:
    """A handle and, per environment (``protos``: per environment modulo that number - the others repeat them), the oracle."""

    def __init__(self, H, W, inits, mode="fused0", seed=1, md=None, att=True, diag=True, max_time=None, pixel_scale=20.0, protos=None,
                 R8=None, update_rate=1.0):
        from simfire_amd.engine import FireEngine
        m = MODES[mode]
        self.H, self.W, self.E, self.mode = H, W, len(inits), mode
        self.P = protos or self.E
        self.md = md if md is not None else m.get("md", 4)
        self.kw = dict(shape=(H, W), max_fire_duration=self.md, pixel_scale=pixel_scale, update_rate=update_rate, max_time=max_time,
                       attenuate_line_ros=att, diagonal_spread=diag)
        self.eng = FireEngine(n_envs=self.E, **self.kw)
        self.eng.set_fused(m["fused"])
        if m.get("tuning"):
            self.eng.set_tuning(**m["tuning"])
        self.eng.set_rtable(table(np.random.default_rng(seed), H, W) if R8 is None else R8)
        self.R8 = self.eng.get_rtable()                    # the common-table protocol: the oracle steps on the device's table
        self.inits = np.asarray(inits, dtype=np.int32)
        assert all((self.inits[e] == self.inits[e % self.P]).all() for e in range(self.E))
        self.eng.reset(self.inits)
        self.w = [self.fresh(e) for e in range(self.P)]

    def fresh(self, e):
        return _ignite_oracle.IgniteFire((self.H, self.W), tuple(int(v) for v in self.inits[e]), self.R8, self.md, self.kw["pixel_scale"],
                                         self.kw["update_rate"], max_time=self.kw["max_time"], attenuate_line_ros=self.kw["attenuate_line_ros"],
                                         diagonal_spread=self.kw["diagonal_spread"])

    def rows(self, cells, envs=None):
        """int32 [n, 4]: every (x, y) of ``cells`` in every environment of ``envs`` (default: all)."""
        envs = range(self.E) if envs is None else envs
        return np.array([(e, x, y, 0) for e in envs for (x, y) in cells], dtype=np.int32).reshape(-1, 4)

    def ignite(self, rows, form="host"):
        rows = np.asarray(rows, dtype=np.int32).reshape(-1, 4)
        if form == "host":
            self.eng.ignite(rows)
        else:
            import torch
            self.keep = torch.from_numpy(rows).cuda()
            self.eng.ignite_torch(self.keep)
        by_env = {}
        for (e, x, y, r) in rows.tolist():
            if r == 0 and 0 <= x < self.W and 0 <= y < self.H:
                by_env.setdefault(e, []).append((x, y))
        for p in range(self.P):
            for q in range(p + self.P, self.E, self.P):      # the environments that repeat p were given the same rows
                assert by_env.get(q, []) == by_env.get(p, [])
            self.w[p].ignite(by_env.get(p, []))

    def mitigate(self, rows):
        self.eng.apply_mitigation(rows)
        for p in range(self.P):
            self.w[p].apply_mitigation([(int(x), int(y), int(t)) for (e, x, y, t) in rows if e == p])

    def step(self, n, kind="mode"):
        self.eng.step(n)
        for w in self.w:
            for _ in range(n):
                w.update()
        if kind is not None:
            want = MODES[self.mode]["kind"] if kind == "mode" else kind
            got = self.eng.last_launch_kind()
            assert got == want or (isinstance(want, tuple) and got in want), (self.mode, got, want)

    def check(self, tag, burn=False):
        maps = self.eng.fire_maps()
        st, el = self.eng.status()
        for e in range(self.E):
            w = self.w[e % self.P]
            bad = np.argwhere(maps[e] != w.fire_map)
            assert not len(bad), (tag, e, "map", len(bad), bad[:4].tolist(), [(int(maps[e][tuple(i)]), int(w.fire_map[tuple(i)])) for i in bad[:4]])
            assert st[e].tolist() == w.counts(), (tag, e, "status row", st[e].tolist(), w.counts())
            assert el[e] == w.fire.elapsed_time, (tag, e, "elapsed", el[e], w.fire.elapsed_time)
        if burn:                                            # (last: fetching burn amounts converts the handle to the row-major planes)
            for e in range(self.E) if self.E <= 8 else (0, 1, self.E // 2, self.E - 1):
                assert (self.eng.burn(e) == self.w[e % self.P].fire.burn).all(), (tag, e, "burn")

    def to_layout(self, want):
        """Makes the blocked plane (1) or the row-major planes (0) the current layout: a burn_amounts transfer converts to the
        row-major planes, one update made by the resident launch (on the oracles too) to the blocked plane."""
        if self.eng.cell_layout() != want:
            if want == 0:
                self.eng.burn(0)
            else:
                self.eng.set_fused(2)
                self.step(1, kind=2)
                self.eng.set_fused(MODES[self.mode]["fused"])
        assert self.eng.cell_layout() == want


def near_and_far(w, H, W):
    """Cells for an ignition: beside the fire of oracle ``w`` (inside any window round it), and UNBURNED cells more than four
    16-cell vectors / many rows away from it."""
    ys, xs = np.nonzero(w.fire_map == 1)
    x0, x1, y0, y1 = int(xs.min()), int(xs.max()), int(ys.min()), int(ys.max())
    near = [(min(x1 + 2, W - 1), (y0 + y1) // 2), (max(x0 - 2, 0), y0), ((x0 + x1) // 2, min(y1 + 2, H - 1)), ((x0 + x1) // 2, min(y1 + 2, H - 1))]
    far_x = 0 if x0 > W - 1 - x1 else W - 1
    far = [(far_x, 0), (far_x, H - 1), (W - 1 - far_x, H - 1 if y0 > H - 1 - y1 else 0)]
    return near, far


# ------------------------------------------------------------------------------------------------ 1. the reference's fixtures
@pytest.mark.parametrize("mode", ["fused0", "run_win"])
@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_through_the_engine(name, mode):
    """The reference's maps, status and elapsed time update by update, its burn amounts at the end: the table is the fixture's."""
    from simfire_amd.engine import FireEngine
    d = load(name)
    H, W = (int(v) for v in d["shape"])
    eng = FireEngine((H, W), n_envs=2, max_fire_duration=int(d["max_fire_duration"]), pixel_scale=float(d["pixel_scale"]),
                     update_rate=float(d["update_rate"]), max_time=d["max_time"], attenuate_line_ros=bool(d["attenuate"]),
                     diagonal_spread=bool(d["diagonal"]))
    eng.set_fused(MODES[mode]["fused"])
    eng.set_rtable(d["rtable"])
    eng.reset(np.array([d["init_pos"], d["init_pos"]], dtype=np.int32))
    for s in range(len(d["status"])):
        pts = [(1, int(x), int(y), int(t)) for (u, x, y, t) in d["schedule"] if u == s]
        ign = [(1, int(x), int(y), 0) for (u, x, y) in d["ignite"] if u == s]
        if pts:
            eng.apply_mitigation(pts)
        if s % 2:
            eng.ignite(ign)
        elif ign:
            import torch
            t = torch.tensor(ign, dtype=torch.int32, device="cuda")
            eng.ignite_torch(t)
        eng.step(1)
        assert (eng.fire_map(1) == d["fire_maps"][s]).all(), (name, s)
        st, el = eng.status()
        assert int(st[1, 0]) == int(d["status"][s]) and el[1] == d["elapsed"][s], (name, s)
    assert (eng.burn(1) == d["burn"]).all()
    assert (eng.fire_map(0) != d["fire_maps"][-1]).any()      # (environment 0 had no ignitions: the fixture is about them)


# ------------------------------------------------------------------------------------------------ 2. every launch structure
STRUCT_SHAPES = {"fused0": (37, 101, 3), "fused1": (37, 101, 3), "cells2": (37, 101, 3), "cells4": (24, 40, 2), "run_win": (520, 80, 4),      # (the window has a sixteenth as many rows as the workgroup threads: 36 here)
                
                 "run_loop": (72, 80, 4), "run_team": (136, 64, 3), "run_kwin": (64, 64, 320)}      # (k_win: grids of 64 rows and four vectors at least, more environments than CUs)
STRUCTS = [(m, lay) for m in MODES for lay in ("bl", "rm") if not (m.startswith("cells") and lay == "bl")]      # (wide masks: there is no blocked plane)


@pytest.mark.parametrize("mode,layout", STRUCTS, ids=["%s-%s" % s for s in STRUCTS])
def test_step_ignite_step(mode, layout):
    """Step, ignite (host rows), step, ignite (device rows), step - with the ignitions arriving while the blocked plane / the
    row-major planes are current, beside the old fire and far from it, some rows twice; the structure named is the one that ran."""
    H, W, E = STRUCT_SHAPES[mode]
    P = 8 if E > 8 else None
    rng = np.random.default_rng(11)
    protos = np.stack([rng.integers(W // 3, W - W // 3, size=P or E), rng.integers(H // 3, H - H // 3, size=P or E)], axis=1)
    inits = protos[np.arange(E) % (P or E)]
    p = Pair(H, W, inits, mode, seed=21, protos=P)
    if mode in ("run_win", "run_loop"):
        p.eng.enable_counters(True)
    p.step(3)
    if mode == "run_team":
        assert int(p.eng.team_sizes().max()) >= 2
    p.check("before")
    want = 1 if layout == "bl" else 0
    for i, form in enumerate(("host", "device")):
        p.to_layout(want)
        rows = []
        for e in range(E):
            near, far = near_and_far(p.w[e % p.P], H, W)
            rows += [(e, x, y, 0) for (x, y) in (near + far if (e % p.P) % 2 == i else near)]
        p.ignite(rows, form)
        assert p.eng.cell_layout() == want                  # the call converts nothing
        p.check(("ignited", i))
        # (k_win goes in front only while every fire is known to be young: an ignition gives that bound up until the next reset)
        p.step(2 + i, kind=(2, 4) if mode == "run_kwin" else "mode")
        p.check(("stepped", i))
    p.step(4, kind=(2, 4) if mode == "run_kwin" else "mode")
    if mode in ("run_win", "run_loop"):                     # the lab's count of updates made in the window phase: it ran / it is switched off
        assert (p.eng.counters()["window_updates"] > 0) == (mode == "run_win")
    p.check("end", burn=True)


def test_the_window_phase_declines_a_far_ignition():
    """A fire that spreads a cell per update every way on 520 x 160 (a window of 36 rows).  An ignition two cells beside it leaves the fire inside a window:
    the updates of the next call are made in the window phase (the lab's count of them).  One more than four 16-cell vectors away
    does not: the phase declines, none of the call's updates is made there - and both equal the oracle."""
    H, W = 520, 160
    got = {}
    for where, cell in (("near", (26, 260)), ("far", (150, 260))):
        p = Pair(H, W, [(20, 260)], "run_win", R8=np.full((8, H, W), 1500.0))
        p.eng.set_tuning(run_window=1)
        p.eng.enable_counters(True)
        p.step(3)
        p.ignite([(0, cell[0], cell[1], 0)], "device")
        p.eng.counters(reset=True)
        p.step(4)
        got[where] = int(p.eng.counters()["window_updates"])
        p.check(where, burn=True)
    assert got["near"] > 0 and got["far"] == 0, got


# ------------------------------------------------------------------------------------------------ 3. shapes
def edge_cells(eng, H, W):
    """Cells at x % 16 == 0 and 15, either side of every chunk boundary, the four corners, the last row of a tile and the first of
    the next, two cells of one bitmap word and two of one status word."""
    g = eng.geometry()
    cw, th = max(g["tile_w"], 16), max(g["tile_h"], 1)
    xs = {0, 1, 15, 16, 31, 32, 4, 5, 6, W - 1, W - 2} | {b * cw + d for b in range(1, W // cw + 1) for d in (-1, 0)} | {1023, 1024, 1039, 1040}
    ys = {0, H - 1, th - 1, th, H // 2}
    xs, ys = sorted(x for x in xs if 0 <= x < W), sorted(y for y in ys if 0 <= y < H)
    return [(x, y) for y in ys for x in xs]


@pytest.mark.parametrize("mode", ["fused0", "run_win"])
@pytest.mark.parametrize("shape", [(37, 101), (19, 300), (12, 1100)], ids=lambda s: "%dx%d" % s)
def test_shapes(shape, mode):
    """37 x 101: pitch padding; 19 x 300: several chunks; 12 x 1100: a second bitmap word per row."""
    H, W = shape
    p = Pair(H, W, [(W // 2, H // 2), (3, 3)], mode, seed=31, pixel_scale=30.0)
    if W > 1024:
        assert p.eng.geometry()["pitch"] // 16 > 64
    p.step(2)
    cells = edge_cells(p.eng, H, W)
    assert len(cells) >= 40
    p.ignite(p.rows(cells[0::2], [0]).tolist() + p.rows(cells[1::2], [1]).tolist(), "device")
    p.check("ignited")
    p.step(2)
    p.check("stepped 2")
    p.ignite(p.rows(cells, [1]), "host")                    # the other half, and the first half again: BURNING by now, or BURNED
    p.step(3)
    p.check("stepped 5", burn=True)


# ------------------------------------------------------------------------------------------------ 4. rows that are skipped
@pytest.mark.parametrize("mode", ["fused0", "run_loop"])
def test_rows_on_other_statuses_are_skipped(mode):
    H, W = 24, 40
    p = Pair(H, W, [(20, 12), (20, 12)], mode, seed=41, md=2)
    lines = [(e, 5 + t, 3, t) for e in (0, 1) for t in (3, 4, 5)]
    p.mitigate(lines)
    p.step(5)
    m = p.w[0].fire_map
    assert (m == 1).any() and (m == 2).any()
    dead = [(8, 3), (9, 3), (10, 3)] + [(int(x), int(y)) for s in (1, 2) for (y, x) in np.argwhere(m == s)[:3]]
    before = p.eng.fire_maps()
    p.ignite(p.rows(dead), "host")
    p.ignite(p.rows(dead), "device")
    assert (p.eng.fire_maps() == before).all()
    p.check("dead rows")
    p.ignite(p.rows(dead + [(38, 22)], [1]).tolist() + p.rows([(38, 22)] * 64, [0]).tolist(), "device")      # one live row among them; a cell 64 times
    assert int((p.eng.fire_maps() != before).sum()) == 2
    p.step(4)
    p.check("end", burn=True)


def test_rows_in_environments_that_are_not_running_are_skipped():
    """Environment 0 burns out (a lone burnable cell), 1 QUITs on max_time, 2 QUITs on max_time and keeps pruning, 3 runs."""
    from simfire_amd.engine import FireEngine
    H, W = 20, 33
    R8 = np.full((8, H, W), 40.0)
    kw = dict(shape=(H, W), max_fire_duration=2, pixel_scale=30.0, update_rate=1.0, attenuate_line_ros=True, diagonal_spread=True)
    for prune in (False, True):
        eng = FireEngine(n_envs=2, max_time=3.0, **kw)
        eng.set_fused(0)
        eng.set_prune_after_quit(prune)
        eng.set_rtable(R8)
        eng.reset([(10, 10), (10, 10)])
        eng.step(4)
        assert eng.status()[0][:, 0].tolist() == [1, 1]
        eng.step(1)                                         # elapsed_time 4.0 > max_time: the fifth update QUITs, the sprites of updates 3, 4 live
        st, _ = eng.status()
        assert st[:, 0].tolist() == [0, 0], st[:, 0]           # (the row shows both kinds of QUIT as not running)
        before, row = eng.fire_maps(), st.copy()
        eng.ignite([(0, 30, 3), (1, 2, 17)])
        eng.step(2)
        after = eng.fire_maps()
        assert (after[:, 3, 30] == 0).all() and (after[:, 17, 2] == 0).all() and ((after == 1) <= (before == 1)).all()
        assert (eng.status()[0][:, 2] == row[:, 2]).all()
        assert (int((after == 1).sum()) < int((before == 1).sum())) == prune      # still pruning, or frozen
    Rz = np.zeros((8, H, W))
    p = Pair(H, W, [(10, 10), (10, 10)], "fused0", md=2, R8=Rz, pixel_scale=30.0)
    p.step(4)
    assert p.eng.status()[0][:, 0].tolist() == [0, 0] and not p.w[0].running      # burned out: finished
    before = p.eng.fire_maps()
    p.ignite(p.rows([(3, 3), (30, 15)]), "host")
    p.ignite(p.rows([(3, 3), (30, 15)]), "device")
    p.step(2, kind=None)
    assert (p.eng.fire_maps() == before).all()
    p.check("finished")


@pytest.mark.parametrize("mode", ["fused0", "run_loop"])
def test_a_fire_about_to_burn_out_goes_on(mode):
    """A table of zeros: the reset's sprite never spreads and is pruned by update 3.  After two updates the environment still
    counts as running; an ignition then keeps it alive, and again, while its twin without one finishes."""
    H, W = 20, 33
    p = Pair(H, W, [(10, 10), (10, 10)], mode, md=2, R8=np.zeros((8, H, W)), pixel_scale=30.0)
    p.step(2)
    assert p.eng.status()[0][:, 0].tolist() == [1, 1]
    p.ignite([(1, 25, 5, 0)], "device")
    p.step(2, kind=None)
    assert p.eng.status()[0][:, 0].tolist() == [0, 1]
    p.check("revived")
    p.ignite([(1, 2, 18, 0), (0, 2, 18, 0)], "host")        # (environment 0 has finished: skipped)
    p.step(2, kind=None)
    assert p.eng.status()[0][:, 0].tolist() == [0, 1]
    p.check("again", burn=True)


def test_device_rows_out_of_range_are_skipped():
    import torch
    H, W, E = 19, 45, 3
    p = Pair(H, W, [(20, 9)] * E, "fused0", seed=43)
    p.step(2)
    before = p.eng.fire_maps()
    bad = [(-1, 3, 3, 0), (E, 3, 3, 0), (0, -1, 3, 0), (0, W, 3, 0), (0, 3, -1, 0), (0, 3, H, 0), (0, 3, 3, 1), (0, 3, 3, -1),
           (2 ** 31 - 1, 3, 3, 0), (1, 2 ** 31 - 1, 3, 0), (1, 3, -2 ** 31, 0), (1, 46, 3, 0)]      # (46: in the pitch padding)
    p.eng.ignite_torch(torch.tensor(bad, dtype=torch.int32, device="cuda"))
    assert (p.eng.fire_maps() == before).all()
    p.ignite(bad + [(2, 3, 3, 0)], "device")
    assert int((p.eng.fire_maps() != before).sum()) == 1
    p.step(3)
    p.check("end", burn=True)


# ------------------------------------------------------------------------------------------------ 5. the two forms, async, the loop
def _bytes(eng):
    return eng.fire_maps().tobytes(), np.stack([eng.burn(e) for e in range(eng.n_envs)]).tobytes(), eng.status()[0].tobytes(), eng.status()[1].tobytes()


@pytest.mark.parametrize("mode", ["fused1", "run_win"])
def test_forms_async_and_the_closed_loop_agree(mode):
    H, W, E = 72, 80, 3
    inits = [(30, 30), (50, 40), (12, 60)]
    rows = [(e, x, y, 0) for e in range(E) for (x, y) in [(3, 3), (70, 65), (33, 30), (33, 30), (79, 0)]]
    got = []
    for how in ("host", "device", "async") + (("loop",) if mode == "run_win" else ()):      # (a closed loop needs the resident launch)
        p = Pair(H, W, inits, mode, seed=51)
        if how == "async":
            p.eng.set_async(True)
        p.step(2)
        if how == "loop":
            p.eng.loop_start(1)
            p.eng.loop_step(None)                           # the third update, made by the running loop
            for w in p.w:
                w.update()
        else:
            p.step(1)
        p.ignite(rows, "device" if how in ("device", "async") else "host")
        if how == "loop":
            with pytest.raises(RuntimeError):
                p.eng.loop_step(None)                       # the call has ended the loop
        p.step(3)
        if how == "async":
            p.eng.sync()
        got.append(_bytes(p.eng))
        p.check(how)
    assert all(g == got[0] for g in got)


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_change_nothing():
    from simfire_amd import _lib
    from simfire_amd.engine import FireEngine
    import torch
    H, W, E = 19, 45, 2
    eng = FireEngine((H, W), n_envs=E, max_fire_duration=4, pixel_scale=20.0)
    eng.set_rtable(table(np.random.default_rng(3), H, W))
    L, h = eng._L, eng._h
    ok = np.array([[0, 5, 5, 0]], dtype=np.int32)
    dev = torch.tensor([[0, 5, 5, 0], [1, 6, 6, 0]], dtype=torch.int32, device="cuda")
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.sf_ignite(h, ptr(ok), 1) == _lib.SF_ESTATE and L.sf_ignite_device(h, C.c_void_p(dev.data_ptr()), 2) == _lib.SF_ESTATE
    with pytest.raises(RuntimeError):
        eng.ignite(ok)
    eng.reset([(20, 9), (20, 9)])
    eng.step(2)
    before = _bytes(eng)
    for bad in ([E, 5, 5, 0], [-1, 5, 5, 0], [0, W, 5, 0], [0, -1, 5, 0], [0, 5, H, 0], [0, 5, -1, 0], [0, 5, 5, 7]):
        rows = np.array([[0, 7, 7, 0], bad, [1, 8, 8, 0]], dtype=np.int32)
        assert L.sf_ignite(h, ptr(rows), 3) == _lib.SF_EINVAL
        assert b"row 1" in L.sf_last_error()
    assert L.sf_ignite(h, ptr(ok), -1) == _lib.SF_EINVAL and L.sf_ignite(h, None, 1) == _lib.SF_EINVAL
    assert L.sf_ignite_device(h, C.c_void_p(dev.data_ptr()), -1) == _lib.SF_EINVAL and L.sf_ignite_device(h, None, 2) == _lib.SF_EINVAL
    assert L.sf_ignite_device(h, C.c_void_p(dev.data_ptr() + 4), 1) == _lib.SF_EINVAL      # not 16-byte aligned
    assert L.sf_ignite(h, None, 0) == _lib.SF_OK and L.sf_ignite_device(h, None, 0) == _lib.SF_OK
    with pytest.raises(IndexError):
        eng.ignite([(E, 1, 1)])
    with pytest.raises(ValueError):
        eng.ignite([(0, W, 1)])
    with pytest.raises(ValueError):
        eng.ignite_torch(dev.to(torch.int64))
    with pytest.raises(ValueError, match="contiguous"):
        eng.ignite_torch(torch.zeros((2, 8), dtype=torch.int32, device="cuda")[:, ::2])      # a copy would run where the caller cannot order it
    assert _bytes(eng) == before


# ------------------------------------------------------------------------------------------------ 7. arrival and values
@pytest.mark.parametrize("mode", ["fused0", "run_win"])
def test_arrival_and_damage(mode):
    H, W, E = 72, 80, 3
    p = Pair(H, W, [(30, 30), (50, 40), (12, 60)], mode, seed=61)
    vals = np.random.default_rng(5).integers(1, 100, size=(H, W)).astype(np.int32)
    p.eng.enable_arrival(True)
    p.eng.values_set(vals)
    want = lambda: [int(vals[w.arrival >= 0].sum()) for w in p.w]
    p.ignite(p.rows([(70, 5), (71, 5)], [0, 2]), "host")    # before the first update: arrival 0, like the reset's own cell
    for e in (0, 2):
        assert p.eng.arrival(e)[5, 70] == 0 and p.eng.arrival(e)[5, 71] == 0
    assert p.eng.damage().tolist() == want()
    p.step(5)
    d0 = p.eng.damage()
    assert d0.tolist() == want()
    cells = [(3, 66), (4, 66), (3, 66)]
    p.ignite(p.rows(cells, [1, 2]), "device")
    a = [p.eng.arrival(e) for e in range(E)]                # no update in between
    for e in range(E):
        assert (a[e] == p.w[e].arrival).all(), e
    assert a[1][66, 3] == 5 and a[2][66, 4] == 5 and a[0][66, 3] == -1
    d1 = p.eng.damage()
    assert d1.tolist() == want() and (d1 - d0).tolist() == [0, int(vals[66, 3] + vals[66, 4]), int(vals[66, 3] + vals[66, 4])]
    p.ignite(p.rows(cells, [1, 2]), "host")                 # BURNING now: nothing is counted again
    assert p.eng.damage().tolist() == d1.tolist()
    p.step(6)
    for e in range(E):
        assert (p.eng.arrival(e) == p.w[e].arrival).all(), e
    assert p.eng.damage().tolist() == want()
    p.check("end", burn=True)


def test_ensemble_of_forks_that_differ_by_an_ignition():
    """Environments 1..3 are forks of 0; 2 and 3 also start at a far cell: the group {2, 3} reaches it, the group {0, 1} does not."""
    H, W = 72, 80
    p = Pair(H, W, [(30, 30)] * 4, "run_win", seed=71, protos=None)
    p.eng.enable_arrival(True)
    p.step(3)
    p.eng.copy_envs([0, 0, 0], [1, 2, 3])
    p.ignite(p.rows([(70, 60)], [2, 3]), "device")
    p.step(6)
    p.check("forks")
    r = p.eng.ensemble_stats([[0, 1], [2, 3]], horizons=(4, -1), count=True, prob=True)
    p.eng.sync()
    count = r["count"].cpu().numpy()
    exp = np.stack([np.stack([sum(((p.w[e].arrival >= 0) & (p.w[e].arrival <= h)).astype(np.int32) for e in g) for h in (4, 10 ** 6)]) for g in ([0, 1], [2, 3])])
    assert (count == exp).all()
    diff = count[1, 1] - count[0, 1]
    assert diff[60, 70] == 2 and diff.min() >= 0 and (diff > 0).sum() > 1 and not diff[:40, :50].any()
    assert count[1, 0, 60, 70] == 2                          # lit behind update 3: reached by horizon 4
    assert (r["prob"].cpu().numpy() == exp / 2.0).all()


# ------------------------------------------------------------------------------------------------ 8. state
@pytest.mark.parametrize("mode", ["fused0", "run_win"])
def test_fork_snapshot_and_reset_behind_an_ignition(mode):
    H, W, E = 72, 80, 4
    p = Pair(H, W, [(30, 30), (50, 40), (12, 60), (40, 20)], mode, seed=81)
    p.step(3)
    p.ignite([(0, 70, 60, 0), (1, 5, 5, 0)], "device")
    blob = p.eng.save_state([0, 1])                         # an ignited cell that has not been stepped
    then = copy.deepcopy(p.w[:2])
    p.eng.copy_envs([0], [3])
    p.w[3] = copy.deepcopy(p.w[0])
    p.step(4)
    maps = p.eng.fire_maps()
    assert (maps[3] == maps[0]).all() and (p.eng.burn(3) == p.eng.burn(0)).all() and (p.eng.status()[0][3] == p.eng.status()[0][0]).all()
    p.check("fork")
    p.eng.load_state([2, 3], blob)                          # environments 2, 3 become 0, 1 as they were behind the ignition
    p.w[2], p.w[3] = then
    p.check("restored")
    p.step(4)
    p.check("restored and stepped")
    p.ignite([(1, 60, 60, 0), (1, 61, 60, 0)], "host")
    p.eng.reset_envs([1], [(40, 40)])                       # a reset behind an ignition leaves what a reset leaves
    p.inits[1] = (40, 40)
    p.w[1] = p.fresh(1)
    st, el = p.eng.status()
    assert st[1].tolist() == [1, 0, H * W - 1, 1, 0, 0, 0, 0] and el[1] == 0.0
    m = p.eng.fire_map(1)
    assert m[40, 40] == 1 and int((m != 0).sum()) == 1
    p.step(3)
    p.check("reset", burn=True)


# ------------------------------------------------------------------------------------------------ 9. readers
def test_delta_reports_exactly_the_cells_lit():
    H, W = 37, 101
    p = Pair(H, W, [(50, 18), (50, 18)], "fused0", seed=91)
    p.step(3)
    for e in (0, 1):
        if p.eng.fire_map_delta(e) is None:
            pass                                            # (the first query of an environment may ask for the whole map)
    p.step(1)
    for e in (0, 1):
        p.eng.fire_map_delta(e)
    burning = np.argwhere(p.w[0].fire_map == 1)[0]
    cells = [(100, 36), (0, 0), (64, 7), (64, 7), (int(burning[1]), int(burning[0]))]
    p.ignite(p.rows(cells, [1]), "device")
    idx, val = p.eng.fire_map_delta(1)
    assert sorted(idx.tolist()) == sorted([36 * W + 100, 0, 7 * W + 64]) and (val == 1).all()
    idx0, _ = p.eng.fire_map_delta(0)
    assert len(idx0) == 0


def test_spread_graph_roots():
    H, W = 24, 40
    p = Pair(H, W, [(8, 8)], "fused0", seed=93)
    p.eng.enable_spread_graph(True)
    p.eng.reset(p.inits)
    p.step(2, kind=None)
    p.ignite([(0, 30, 15, 0)], "host")
    p.step(3, kind=None)
    par = p.eng.spread_parents(0)
    assert par[15, 30] == 0                                 # a root of the graph
    edges = p.eng.spread_edges(0)
    assert any((sx, sy) == (30, 15) for (sx, sy, x, y) in edges)      # and a parent of what it lights
    assert sorted(edges) == sorted((a[0], a[1], b[0], b[1]) for a, b in p.w[0].fire.edges)
    p.check("graph")


def _config(H, W):
    import yaml
    from simfire_amd.config import Config
    y = yaml.safe_load(open(os.path.join(CFG, "functional_config.yml")))
    y["area"]["screen_size"] = [H, W]
    y["terrain"]["topography"]["functional"]["function"] = "flat"
    y["simulation"]["headless"] = True
    return Config(config_dict=y)


def test_fire_simulation_keeps_the_one_array():
    from simfire_amd.config import Config
    from simfire_amd.enums import BurnStatus
    from simfire_amd.simulation import FireSimulation
    sim = FireSimulation(Config(os.path.join(CFG, "test_config_flat_simple.yml")))
    the_array = sim.fire_map
    sim.run(2)
    H, W = np.asarray(sim.fire_map).shape
    sim.fire_map[H - 1, 0] = int(BurnStatus.FIRELINE)       # a caller's edit in front of the call: synced first
    ys, xs = np.nonzero(np.asarray(sim.fire_map) == int(BurnStatus.BURNING))
    sim.ignite([(W - 1, H - 1), (0, 0), (0, H - 1), (int(xs[0]), int(ys[0]))])
    assert sim.fire_map is the_array
    m = np.asarray(sim.fire_map)
    assert m[H - 1, W - 1] == 1 and m[0, 0] == 1 and m[H - 1, 0] == int(BurnStatus.FIRELINE)      # shown at once; the line cell was skipped
    assert (m == sim._engine.fire_map(0)).all()
    burning = int((m == 1).sum())
    fm, active = sim.run(1)
    assert fm is the_array and (np.asarray(fm) == sim._engine.fire_map(0)).all() and active
    assert int((np.asarray(fm) == 1).sum()) > burning
    sim.ignite([])


def test_a_tensor_still_being_written_on_torchs_stream():
    """The advertised use: the rows are the output of work still queued on torch's current stream.  The tensor holds (0, 0, 0) rows
    until a copy behind a few long matrix products fills it; ``BatchedFireSimulation.ignite`` given its ``[n, 3]`` form must light
    the rows the copy brings, not what the memory held when the call was made."""
    import torch
    from simfire_amd.simulation import BatchedFireSimulation
    sim = BatchedFireSimulation(_config(24, 40), 2, ignitions=np.array([(10, 10), (30, 7)], dtype=np.int32))
    sim.run(2, return_maps=False)
    real = torch.tensor([[0, 39, 23], [1, 0, 23], [1, 39, 0]], dtype=torch.int32, device="cuda")
    buf = torch.zeros((3, 3), dtype=torch.int32, device="cuda")
    a = torch.randn((8192, 8192), dtype=torch.float16, device="cuda")
    torch.cuda.synchronize()
    for _ in range(12):
        a = (a @ a).clamp_(-1.0, 1.0)
    buf.copy_(real, non_blocking=True)
    sim.ignite(buf)
    assert sim.fire_map(0)[23, 39] == 1 and sim.fire_map(1)[23, 0] == 1 and sim.fire_map(1)[0, 39] == 1
    assert sim.fire_map(0)[0, 0] == 0 and sim.fire_map(1)[0, 0] == 0


def test_a_device_tensor_is_ordered_before_the_handle_reads_it(monkeypatch):
    """The frame of ``BatchedFireSimulation.ignite`` for a CUDA tensor, by what it calls in which order (the race of the test above
    needs a stream that is busy at the right moment): whatever it makes of the tensor on torch's current stream - four columns,
    contiguous - is made first, then that stream is waited for, and only then the engine is handed the tensor."""
    import torch
    from simfire_amd.simulation import BatchedFireSimulation
    sim = BatchedFireSimulation(_config(24, 40), 2, ignitions=np.array([(10, 10), (30, 7)], dtype=np.int32))
    events = []
    real_stream = torch.cuda.current_stream

    class Stream:
        def __init__(self, s):
            self.s = s

        def synchronize(self):
            events.append("wait")
            self.s.synchronize()

    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: Stream(real_stream(device)))
    real_ignite = sim._engine.ignite_torch
    monkeypatch.setattr(sim._engine, "ignite_torch", lambda p: (events.append(("engine", tuple(p.shape), p.is_contiguous())), real_ignite(p)))
    for rows in (torch.tensor([[0, 39, 23], [1, 0, 23]], dtype=torch.int32, device="cuda"),
                 torch.tensor([[0, 38, 23, 0], [1, 1, 23, 0]], dtype=torch.int32, device="cuda"),
                 torch.zeros((2, 8), dtype=torch.int32, device="cuda")[:, ::2]):
        events.clear()
        sim.ignite(rows)
        assert events == ["wait", ("engine", (2, 4), True)], events
    assert sim.fire_map(0)[23, 39] == 1 and sim.fire_map(1)[23, 1] == 1 and sim.fire_map(0)[0, 0] == 1      # (the last tensor: zeros, row (0, 0, 0))


def test_batched_simulation_and_env_forward():
    import torch
    import simfire_amd
    from simfire_amd.simulation import BatchedFireSimulation
    cfg = _config(24, 40)
    E, K = 3, 2
    ign = np.array([(10, 10), (30, 7), (3, 20)], dtype=np.int32)
    sim = BatchedFireSimulation(cfg, E, ignitions=ign)
    sim.run(2, return_maps=False)
    sim.ignite([(0, 39, 23), (2, 39, 0)])
    sim.ignite(torch.tensor([[1, 0, 23], [1, 40, 3]], dtype=torch.int32, device="cuda"))      # [n, 3] on the device; a column off the grid is dropped
    assert sim.fire_map(0)[23, 39] == 1 and sim.fire_map(2)[0, 39] == 1 and sim.fire_map(1)[23, 0] == 1 and sim.fire_map(1)[23, 39] == 0
    with pytest.raises(IndexError):
        sim.ignite([(E, 1, 1)])
    src, m0 = sim.get_state([0]), sim.fire_map(0)
    sim.clone_envs([0], [1])
    sim.run(3, return_maps=False)
    m3 = sim.fire_map(0)
    assert (m3 == sim.fire_map(1)).all() and m3[23, 39] in (1, 2) and int((m3 != 0).sum()) > int((m0 != 0).sum())
    sim.set_state(src, [2])
    assert (sim.fire_map(2) == m0).all()
    sim.run(3, return_maps=False)
    assert (sim.fire_map(2) == m3).all()
    starts = np.array([(1, 1), (2, 2)], dtype=np.int32)
    env = simfire_amd.BatchedFireEnv(BatchedFireSimulation(cfg, E, ignitions=ign), K, starts, n_updates=1)
    twin = simfire_amd.BatchedFireEnv(BatchedFireSimulation(cfg, E, ignitions=ign), K, starts, n_updates=1)
    env.reset()
    twin.reset()
    actions = torch.zeros((E, K), dtype=torch.int32, device="cuda")
    o1, o2 = env.step(actions)[0], twin.step(actions)[0]
    assert torch.equal(o1, o2)
    env.ignite([(1, 38, 22)])
    o1, o2 = env.step(actions)[0], twin.step(actions)[0]
    assert not torch.equal(o1[1], o2[1]) and torch.equal(o1[0], o2[0]) and torch.equal(o1[2], o2[2])
    assert env.sim.fire_map(1)[22, 38] == 1 and twin.sim.fire_map(1)[22, 38] == 0
