"""Per-environment terrain (``FireEngine(per_env_terrain=True)``: one R table per environment, and one cell-major copy of it for the
window phase) in every launch structure.

A kernel that read environment 0's table - or a cell-major copy that went stale - for environment e would pass every test on a
shared table.  Here every environment has a random table of its own (exact ties, barren cells of its own, a scale of its own), so
that a read of any other environment's table changes burn_amounts at the first cell it visits.  Each case is compared bit for bit
with ``oracle/fire_dense.c`` run once per environment (tests/_per_env_oracle.py) - fire maps, result rows, elapsed_time,
burn_amounts - and asserts that the launch structure it is about really ran.  Run with ``pytest -m gpu``."""
import numpy as np
import pytest

from _per_env_oracle import PerEnvOracle
from oracle import fire_dense

pytestmark = pytest.mark.gpu

VALUES = (0.0, 3.0, 7.5, 12.0, 30.0, 400.0, 1200.0)


def _scale(e):
    return 1.0 + 0.37 * (e % 7) + 0.0013 * e


def _table(rng, H, W, e):
    """Exact ties, barren cells of this environment's own, a scale of its own."""
    R8 = rng.choice(VALUES, size=(8, H, W)) * _scale(e)
    R8[:, rng.random((H, W)) < 0.1] = 0.0
    return R8


def _world(rng, H, W, E, att=None, md=None):
    md = int(rng.integers(1, 6)) if md is None else md
    att = bool(rng.integers(2)) if att is None else att
    kw = dict(shape=(H, W), n_envs=E, max_fire_duration=md, pixel_scale=float(rng.choice([5.0, 20.0, 50.0])),
              update_rate=float(rng.choice([1.0, 0.5, 1.5])),
              max_time=(None if rng.random() < 0.7 else float(rng.integers(15, 60))),
              attenuate_line_ros=att, diagonal_spread=True)
    return kw, [_table(rng, H, W, e) for e in range(E)]


def _inits(rng, H, W, E):
    """Ignitions anywhere, also at the grid's edges and in its corners."""
    out = []
    for _ in range(E):
        q = rng.random()
        if q < 0.25:
            out.append((int(rng.choice([0, 1, W - 2, W - 1])), int(rng.choice([0, 1, H - 2, H - 1]))))
        elif q < 0.4:
            out.append((int(rng.choice([0, W - 1])), int(rng.integers(H))))
        else:
            out.append((int(rng.integers(W)), int(rng.integers(H))))
    return out


def _pair(kw, tabs, inits):
    from simfire_amd.engine import FireEngine
    eng = FireEngine(per_env_terrain=True, **kw)
    o = PerEnvOracle(**kw)
    for e, t in enumerate(tabs):
        eng.set_rtable(t, env=e)
        o.set_rtable(t, env=e)
    eng.reset(inits)
    o.reset(inits)
    return eng, o


def _same(eng, o, burn=True, envs=None, tag=None):
    st, el = eng.status()
    so, eo = o.status()
    assert (st == so).all() and (el == eo).all(), tag
    envs = range(o.n_envs) if envs is None else envs
    maps = eng.fire_maps()
    for e in envs:
        assert (maps[e] == o.fire_map(e)).all(), (tag, e)
    if burn:
        for e in envs:
            assert (eng.burn(e) == o.burn(e)).all(), (tag, e, "burn")


def _lines(rng, o, E, H, W, n=20):
    """Control lines anywhere, and on two burning cells of one environment."""
    pts = [(int(rng.integers(E)), int(rng.integers(W)), int(rng.integers(H)), int(rng.integers(3, 6))) for _ in range(n)]
    e0 = int(rng.integers(E))
    burning = np.argwhere(o.fire_map(e0) == 1)
    if len(burning):
        y, x = burning[rng.integers(len(burning))]
        pts += [(e0, int(x), int(y), int(rng.integers(3, 6))), (e0, min(int(x) + 1, W - 1), int(y), int(rng.integers(3, 6)))]
    return pts


def _drive(rng, eng, o, total, n_range, after, burn_every=3, resets=True, lines=True):
    """Calls of random length with control lines and resets between them; equal to the oracle after every call (burn_amounts
    every `burn_every` calls and at the end: reading them moves the handle to its row-major planes)."""
    E, H, W = o.n_envs, o.H, o.W
    done, call = 0, 0
    while done < total:
        n = int(rng.integers(*n_range))
        if lines and rng.random() < 0.4:
            pts = _lines(rng, o, E, H, W)
            eng.apply_mitigation(pts)
            o.apply_mitigation(pts)
        if resets and rng.random() < 0.12 and done > 6:
            e0, x, y = int(rng.integers(E)), int(rng.integers(W)), int(rng.integers(H))
            eng.reset_env(e0, x, y)
            o.reset_env(e0, x, y)
        eng.step(n)
        o.step(n)
        done += n
        call += 1
        after(n)
        _same(eng, o, burn=(call % burn_every == 0), tag=(done, n))
    _same(eng, o, tag=("end", done))


# ------------------------------------------------------------------ the launch-structure matrix
@pytest.mark.parametrize("mode", ["fused0", "fused1", "generic6", "generic14", "generic28"])
def test_per_step_kernels(mode):
    """k_select + k_step, the fused per-step kernel, and k_step_cells (the per-cell kernel) on 1-, 2- and 4-byte sprite planes."""
    rng = np.random.default_rng(61000 + ["fused0", "fused1", "generic6", "generic14", "generic28"].index(mode))
    H, W, E = int(rng.integers(64, 140)), int(rng.integers(64, 160)), 4
    md = int(mode[7:]) if mode.startswith("generic") else None
    kw, tabs = _world(rng, H, W, E, md=md)
    eng, o = _pair(kw, tabs, _inits(rng, H, W, E))
    want = 3
    if mode.startswith("generic"):
        eng.set_generic(True)
    else:
        want = int(mode[-1])
        eng.set_fused(want)

    def after(n):
        assert eng.last_launch_kind() == want
    _drive(rng, eng, o, 40, (1, 8), after)


@pytest.mark.parametrize("win", [0, 1, 2, 3, 7])
def test_resident_window_phase_and_general_loop(win):
    """k_run: the general loop alone (run_window = 0), the window phase, and the hand-over inside one launch after `win` updates."""
    rng = np.random.default_rng(62000 + win)
    H, W, E = int(rng.integers(64, 300)), int(rng.integers(64, 300)), 5
    kw, tabs = _world(rng, H, W, E)
    eng, o = _pair(kw, tabs, _inits(rng, H, W, E))
    eng.set_fused(2)
    eng.set_tuning(run_window=win)
    eng.enable_counters(True)

    def after(n):
        assert eng.last_launch_kind() == 2
    _drive(rng, eng, o, 80, (2, 25), after)
    cnt = eng.counters()["window_updates"]
    assert (cnt == 0) if win == 0 else (cnt > 0), cnt


@pytest.mark.parametrize("win", [1, 3])
def test_window_kernel_in_front_of_the_resident_launch(win):
    """k_win in front of k_run (run_compact = 2): calls it makes alone (win = 1, short calls of young fires) and calls that leave work
    behind for k_run (win = 3: the window is left after three updates)."""
    rng = np.random.default_rng(63000 + win)
    H, W, E = int(rng.integers(64, 300)), int(rng.integers(64, 300)), 6
    kw, tabs = _world(rng, H, W, E)
    eng, o = _pair(kw, tabs, _inits(rng, H, W, E))
    eng.set_tuning(run_compact=2, run_window=win)
    eng.enable_counters(True)
    seen = []

    def after(n):
        seen.append((n, eng.last_launch_kind(), eng.last_launches()))
    eng.step(2)
    o.step(2)
    after(2)
    _same(eng, o, tag="first")
    _drive(rng, eng, o, 60, (2, 12), after)
    kinds = [k for _, k, _ in seen]
    assert kinds[0] == 4 and set(kinds) <= {2, 4}, seen
    assert eng.counters()["window_updates"] > 0
    if win == 1:
        assert any(k == 4 and l == 1 for _, k, l in seen), seen          # k_win alone
    else:
        assert any(k == 4 and l == 2 for _, k, l in seen), seen          # k_win + k_run behind it


@pytest.mark.parametrize("T,place,seg,recut", [(2, 0, 2, 1), (3, 1, 5, 0), (4, 2, 3, 1), (2, 1, 1, 0)])
def test_fixed_teams(T, place, seg, recut):
    """k_run<TEAM>: every environment's rows cut into T bands, one workgroup each, the bands cut anew inside the launch (or one launch
    per segment)."""
    rng = np.random.default_rng(64000 + 10 * T + place)
    H, W, E = int(rng.integers(130, 300)), int(rng.integers(64, 260)), 3
    kw, tabs = _world(rng, H, W, E)
    eng, o = _pair(kw, tabs, _inits(rng, H, W, E))
    eng.set_fused(2)
    eng.set_tuning(run_team=T, team_placement=place, run_segment=seg, team_recut=recut)
    teams = []

    def after(n):
        assert eng.last_launch_kind() == 2
        teams.append(bool((eng.team_sizes() == T).all()))
    _drive(rng, eng, o, 110, (4, 40), after)
    assert any(teams)


@pytest.mark.parametrize("seg", [1, 4, 12])
def test_teams_that_grow(seg):
    """k_run<TEAM = 2> with joins (run_join = -2): a workgroup done with its environment joins another environment's team and must
    switch to that environment's table."""
    rng = np.random.default_rng(65000 + seg)
    H, W, E = int(rng.integers(100, 300)), int(rng.integers(64, 300)), 5
    kw, tabs = _world(rng, H, W, E)
    eng, o = _pair(kw, tabs, _inits(rng, H, W, E))
    eng.set_fused(2)
    eng.set_tuning(run_join=-2, run_segment=seg, team_placement=seg % 3)
    grown, joins = [0], [0]

    def after(n):
        assert eng.last_launch_kind() == 2 and eng.last_launches() == 1
        sizes = eng.team_sizes()
        assert sizes.min() >= 1 and sizes.max() <= 4, sizes
        grown[0] += int((sizes > 1).sum())
        log = eng.join_log()
        joins[0] += int((log[:, 2] != 255).sum()) if len(log) else 0
    _drive(rng, eng, o, 120, (4, 50), after)
    assert grown[0] > 0 and joins[0] > 0


@pytest.mark.parametrize("shape", [(91, 1102), (150, 1100)])
def test_two_word_rows_plain_and_team_launches_take_turns(shape):
    """Rows of two bitmap words (W > 1024): step() runs as teams, step_mitigated() as the plain kernel."""
    rng = np.random.default_rng(66000 + shape[0])
    H, W = shape
    E = 3
    kw, tabs = _world(rng, H, W, E)
    eng, o = _pair(kw, tabs, [(900, 20), (400, H - 2), (1030, 60)])
    eng.set_fused(2)
    kinds = set()
    for t in range(18):
        if t % 3 == 1:
            n = int(rng.integers(1, 5))
            blk = np.zeros((n, E, 2, 3), dtype=np.int32)
            blk[..., 0] = rng.integers(0, W, (n, E, 2))
            blk[..., 1] = rng.integers(0, H, (n, E, 2))
            blk[..., 2] = rng.integers(3, 6, (n, E, 2))
            eng.step_mitigated(blk)
            for s in range(n):
                o.apply_mitigation([(e, int(blk[s, e, i, 0]), int(blk[s, e, i, 1]), int(blk[s, e, i, 2])) for e in range(E) for i in range(2)])
                o.step(1)
        else:
            n = int(rng.integers(1, 6))
            eng.step(n)
            o.step(n)
        assert eng.last_launch_kind() == 2
        kinds.add(int(eng.team_sizes().max()) > 0)
        _same(eng, o, burn=(t % 4 == 3), tag=t)
    _same(eng, o, tag="end")
    assert kinds == {False, True}


@pytest.mark.parametrize("K", [12, 64, 80])
def test_step_mitigated(K):
    """sf_step_mitigated inside k_run: lines inside the window phase (K <= 64: one wave takes the points), more points per step through
    the whole workgroup (K = 80: without the window phase)."""
    rng = np.random.default_rng(67000 + K)
    H, W, E = 90, 210, 4
    kw, tabs = _world(rng, H, W, E, att=bool(K % 2 == 0))
    eng, o = _pair(kw, tabs, _inits(rng, H, W, E))
    eng.set_fused(2)
    eng.enable_counters(True)
    for i, chunk in enumerate((1, 7, 15, 22)):
        blk = np.zeros((chunk, E, K, 3), dtype=np.int32)
        blk[..., 0] = rng.integers(0, W, (chunk, E, K))
        blk[..., 1] = rng.integers(0, H, (chunk, E, K))
        blk[..., 2] = rng.integers(2, 7, (chunk, E, K))                  # 2 and 6: padding
        for s in range(chunk):
            burning = np.argwhere(o.fire_map(1) == 1)
            if len(burning):                                              # a line on a burning cell of environment 1
                y, x = burning[rng.integers(len(burning))]
                blk[s, 1, 3] = (x, y, int(rng.integers(3, 6)))
            rows = [(e, int(blk[s, e, k, 0]), int(blk[s, e, k, 1]), int(blk[s, e, k, 2])) for e in range(E) for k in range(K)
                    if 3 <= blk[s, e, k, 2] <= 5]
            o.apply_mitigation(rows)
            o.step(1)
        eng.step_mitigated(blk)
        assert eng.last_launch_kind() == 2
        _same(eng, o, burn=(i % 2 == 1), tag=(K, chunk))
    if K <= 64:
        assert eng.counters()["window_updates"] > 0


@pytest.mark.parametrize("K", [0, 9])
def test_closed_loop(K):
    """sf_loop_start / sf_loop_step: the resident launch driven one update at a time, with K points per environment and step."""
    rng = np.random.default_rng(68000 + K)
    H, W, E = 100, 150, 4
    kw, tabs = _world(rng, H, W, E)
    eng, o = _pair(kw, tabs, _inits(rng, H, W, E))
    eng.step(3)
    o.step(3)
    eng.loop_start(K)
    assert eng.last_launch_kind() == 2
    for s in range(30):
        pts = None
        if K:
            pts = np.zeros((E, K, 3), dtype=np.int32)
            pts[..., 0] = rng.integers(0, W, (E, K))
            pts[..., 1] = rng.integers(0, H, (E, K))
            pts[..., 2] = rng.integers(2, 7, (E, K))
            burning = np.argwhere(o.fire_map(2) == 1)
            if len(burning):
                y, x = burning[rng.integers(len(burning))]
                pts[2, 0] = (int(x), int(y), 3 + s % 3)
            o.apply_mitigation([(e, int(p[0]), int(p[1]), int(p[2])) for e in range(E) for p in pts[e] if 3 <= p[2] <= 5])
        o.step(1)
        status, elapsed = eng.loop_step(pts)
        so, eo = o.status()
        assert (status == so).all() and (elapsed == eo).all(), s
        if s == 15:
            _same(eng, o, burn=False, tag="mid")        # (any other call ends the loop)
            eng.loop_start(K)
    eng.loop_stop()
    _same(eng, o, tag="end")


def test_run_delta_with_a_host_mirror():
    """sf_run_delta: the updates, one environment's row and the cells of its map that changed; a host mirror kept from the deltas."""
    rng = np.random.default_rng(69000)
    H, W, E = 96, 140, 4
    kw, tabs = _world(rng, H, W, E)
    eng, o = _pair(kw, tabs, _inits(rng, H, W, E))
    eng.set_fused(2)
    mirror = [None] * E
    kinds = set()
    for t in range(16):
        e = int(rng.integers(E))
        n = int(rng.integers(1, 12))
        row, el, d = eng.run_delta(n, env=e, cap=int(rng.choice([4096, 64])))
        kinds.add(eng.last_launch_kind())
        o.step(n)
        so, eo = o.status()
        assert (row == so[e]).all() and el == eo[e], (t, e)
        if d is None or mirror[e] is None:
            mirror[e] = eng.fire_map(e).astype(np.int64)
        else:
            mirror[e].reshape(-1)[d[0]] = d[1]
        assert (mirror[e] == o.fire_map(e)).all(), (t, e)
    _same(eng, o, tag="end")
    assert 2 in kinds


# ------------------------------------------------------------------ tables that change between resident calls
def _layers(rng, H, W):
    return (rng.uniform(0.01, 0.3, (H, W)), rng.uniform(0.5, 6.0, (H, W)), rng.uniform(0.12, 0.4, (H, W)),
            rng.uniform(1000, 3500, (H, W)), rng.uniform(0, 400, (H, W)), rng.uniform(0, 900, (H, W)), rng.uniform(0, 360, (H, W)))


def _fbfm(rng, H, W):
    codes = rng.choice([1, 2, 3, 4, 5, 8, 9, 10, 13, 91, 98], size=(H, W)).astype(np.int32)
    return codes, rng.uniform(0, 400, (H, W)), rng.uniform(0, 900, (H, W)), rng.uniform(0, 360, (H, W))


def _structure(eng, kind):
    if kind == "window":
        eng.set_fused(2)
        eng.set_tuning(run_window=1)
    else:
        eng.set_tuning(run_compact=2, run_window=1)
    eng.enable_counters(True)


@pytest.mark.parametrize("kind", ["window", "kwin"])
@pytest.mark.parametrize("path", ["rtable", "layers", "fbfm", "layers_all"])
def test_table_changed_between_resident_calls(path, kind):
    """The cell-major copy exists and is current (window-phase calls ran); then one environment's table (or all of them) is replaced.
    Environment k follows its new table from the next call on, the others keep theirs."""
    rng = np.random.default_rng(70000 + 10 * ["rtable", "layers", "fbfm", "layers_all"].index(path) + (kind == "kwin"))
    H, W, E, k = int(rng.integers(64, 200)), int(rng.integers(64, 200)), 4, 2
    kw, tabs = _world(rng, H, W, E)
    inits = [(int(rng.integers(8, W - 8)), int(rng.integers(8, H - 8))) for _ in range(E)]
    eng, o = _pair(kw, tabs, inits)
    _structure(eng, kind)
    want = 2 if kind == "window" else 4
    for n in (3, 4):
        eng.step(n)
        o.step(n)
        _same(eng, o, burn=False, tag=("before", n))
    before = eng.counters(reset=True)["window_updates"]
    assert before > 0 and eng.last_launch_kind() == want
    if path == "rtable":
        new = _table(rng, H, W, E + 3)
        eng.set_rtable(new, env=k)
        o.set_rtable(new, env=k)
    elif path == "layers":
        eng.set_layers(*_layers(rng, H, W), env=k)
        o.set_rtable(eng.get_rtable(k), env=k)
    elif path == "fbfm":
        eng.set_layers_fbfm(*_fbfm(rng, H, W), env=k)
        o.set_rtable(eng.get_rtable(k), env=k)
    else:
        eng.set_layers(*_layers(rng, H, W))
        o.set_rtable(eng.get_rtable(0))
    for e in range(E):
        if path == "layers_all":
            assert (eng.get_rtable(e) == eng.get_rtable(0)).all(), e
        elif e == k:
            assert not (eng.get_rtable(e) == tabs[e]).all()
        else:
            assert (eng.get_rtable(e) == tabs[e]).all(), e
    # environment k also burns anew from a young fire, so that its next updates surely run in the window
    eng.reset_env(k, *inits[k])
    o.reset_env(k, *inits[k])
    for n in (2, 3, 5, 4, 8):
        eng.step(n)
        o.step(n)
        assert eng.last_launch_kind() == want
        _same(eng, o, burn=False, tag=(path, kind, n))
    _same(eng, o, tag=(path, kind, "end"))
    assert eng.counters()["window_updates"] > 0


# ------------------------------------------------------------------ fork and restore
@pytest.mark.parametrize("kind", ["window", "kwin"])
@pytest.mark.parametrize("terrain", [True, False])
def test_fork_after_the_cell_major_copy_was_built(terrain, kind):
    """copy_envs(src, dst, terrain) after window-phase calls built the cell-major copies: with terrain dst goes on over src's table
    (and has src's layers), without over its own."""
    rng = np.random.default_rng(71000 + 2 * terrain + (kind == "kwin"))
    H, W, E = int(rng.integers(64, 200)), int(rng.integers(64, 200)), 4
    kw, tabs = _world(rng, H, W, E)
    inits = [(int(rng.integers(8, W - 8)), int(rng.integers(8, H - 8))) for _ in range(E)]
    eng, o = _pair(kw, tabs, inits)
    for e in range(E):
        eng.set_layers(*_layers(rng, H, W), env=e)       # (layers for attribute_data; the tables are set again below)
        eng.set_rtable(tabs[e], env=e)
    _structure(eng, kind)
    want = 2 if kind == "window" else 4
    eng.step(2)
    o.step(2)
    assert eng.counters(reset=True)["window_updates"] > 0
    _same(eng, o, burn=False, tag="before")
    src, dst = 1, 3
    eng.copy_envs([src], [dst], terrain=terrain)
    o.copy_env(src, dst, terrain=terrain)
    a_src, a_dst = eng.attribute_data(src), eng.attribute_data(dst)
    if terrain:
        assert all((a_src[name] == a_dst[name]).all() for name in a_src)
        assert (eng.get_rtable(dst) == tabs[src]).all()
    else:
        assert not (a_src["w_0"] == a_dst["w_0"]).all()
        assert (eng.get_rtable(dst) == tabs[dst]).all()
    # (short calls: the window holds a fire for its first updates only; a call of one update is no resident launch unless forced)
    for n in ((1 if kind == "window" else 2), 2, 2, 5, 4):
        eng.step(n)
        o.step(n)
        assert eng.last_launch_kind() == want
        _same(eng, o, burn=False, tag=(terrain, kind, n))
    _same(eng, o, tag="end")
    assert eng.counters()["window_updates"] > 0


@pytest.mark.parametrize("kind", ["window", "kwin"])
def test_state_loaded_into_a_handle_with_other_tables(kind):
    """load_state into an environment of another per-environment handle whose table differs: a blob holds no terrain, so the fire
    goes on over the receiver's table."""
    rng = np.random.default_rng(72000 + (kind == "kwin"))
    H, W, E = 120, 150, 3
    kw, tabs_a = _world(rng, H, W, E, att=True)
    tabs_b = [_table(rng, H, W, E + e) for e in range(E)]
    inits = [(int(rng.integers(8, W - 8)), int(rng.integers(8, H - 8))) for _ in range(E)]
    a, oa = _pair(kw, tabs_a, inits)
    b, ob = _pair(kw, tabs_b, inits[::-1])
    for x in (a, b):
        _structure(x, kind)
    for x in (a, b, oa, ob):
        x.step(2)
    assert b.counters(reset=True)["window_updates"] > 0
    blob = a.save_state([1])
    b.load_state([2], blob)
    ob.copy_env(1, 2, source=oa)
    assert (b.get_rtable(2) == tabs_b[2]).all()
    for n in ((1 if kind == "window" else 2), 2, 3, 6):
        b.step(n)
        ob.step(n)
        assert b.last_launch_kind() == (2 if kind == "window" else 4)
        _same(b, ob, burn=False, tag=(kind, n))
    _same(b, ob, tag="end")
    assert b.counters()["window_updates"] > 0


# ------------------------------------------------------------------ more environments than CUs, by the automatic plan
def test_more_environments_than_cus_each_with_its_own_table():
    """300 environments of 96 x 128, default tuning: k_win in front of k_run while the fires are young, plain k_run later."""
    rng = np.random.default_rng(73000)
    H, W, E = 96, 128, 300
    kw, tabs = _world(rng, H, W, E, att=False, md=3)
    kw.update(max_time=None, pixel_scale=20.0, update_rate=1.0)
    eng, o = _pair(kw, tabs, [(int(rng.integers(W)), int(rng.integers(H))) for _ in range(E)])
    kinds = []
    sample = (0, 1, 128, 255, 256, 257, 299)
    for i, n in enumerate((5, 12, 20, 40)):
        if i == 2:
            pts = [(int(rng.integers(E)), int(rng.integers(W)), int(rng.integers(H)), int(rng.integers(3, 6))) for _ in range(200)]
            eng.apply_mitigation(pts)
            o.apply_mitigation(pts)
        eng.step(n)
        o.step(n, threads=16)
        kinds.append(eng.last_launch_kind())
        _same(eng, o, envs=sample, tag=(i, n))
    assert kinds[0] == 4 and kinds[-1] == 2, kinds


def test_c3_grid_teams_sized_by_the_cost_model():
    """1024 x 1024 x 6 environments, each with its own layers (wind turned per environment), 200 updates in one call: teams sized by
    the cost model."""
    from simfire_amd import workloads
    from simfire_amd.engine import FireEngine
    w = workloads.c3(1024, 6)
    kw = w.engine_kwargs()
    eng = FireEngine(M_f=w.M_f, per_env_terrain=True, **kw)
    o = PerEnvOracle(**kw)
    w0, de, mx, sg, el, U, Ud = w.layers()
    for e in range(6):
        eng.set_layers(w0, de, mx, sg, el + 25.0 * e, U * (0.6 + 0.15 * e), (Ud + 61.0 * e) % 360.0, env=e)
        o.set_rtable(eng.get_rtable(e), env=e)
    eng.reset(w.init_xy)
    o.reset(w.init_xy)
    eng.step(200)
    o.step(200, threads=6)
    assert eng.last_launch_kind() == 2
    assert (eng.team_sizes() > 1).any(), eng.team_sizes()
    _same(eng, o, tag="c3")


# ------------------------------------------------------------------ the per-environment R table against the f64 oracle
@pytest.mark.parametrize("W", [77, 1000, 1030])
def test_per_env_rtable_against_the_f64_oracle(W):
    """k_rtable through set_layers(env=e) and set_layers_fbfm(env=e) against DenseOracle.build_rtable (libm, f64): within 1e-5 of the
    per-direction scale, more than half of the entries bit-equal.  Edge inputs: w_0 = 0 (R = 0), M_x <= M_f, zero wind, wind from
    0 / 90 / 180 / 270 / 359.9 degrees, steep elevation steps (one-sided slopes at the borders)."""
    from simfire_amd.engine import FireEngine
    from simfire_amd.parameters import fuel_planes
    rng = np.random.default_rng(74000 + W)
    H, E, M_f = 40, 4, 0.03
    kw = dict(shape=(H, W), n_envs=E, max_fire_duration=4, pixel_scale=30.0, update_rate=1.0)
    y, x = np.mgrid[0:H, 0:W]
    steps = 600.0 * ((x // 5 + y // 3) % 2) + 40.0 * (x % 7 == 0)      # steep steps everywhere, the borders included

    def check(T, To, tag):
        scale = np.maximum(To.max(axis=0, keepdims=True), 1e-30)
        assert (np.abs(T - To) <= 1e-5 * scale).all(), tag
        assert (T == To).mean() > 0.5, tag

    eng = FireEngine(M_f=M_f, per_env_terrain=True, **kw)
    layers = []
    for e in range(E):
        w0, de, mx, sg = (rng.uniform(0.01, 0.3, (H, W)), rng.uniform(0.5, 6.0, (H, W)), rng.uniform(0.05, 0.4, (H, W)),
                          rng.uniform(1000, 3500, (H, W)))
        U, Ud = rng.uniform(0, 900, (H, W)), rng.uniform(0, 360, (H, W))
        if e == 0:
            w0[:, ::3] = 0.0                                            # no fuel
        if e == 1:
            mx[::2] = rng.choice([0.01, 0.02, M_f, np.float32(M_f)], size=mx[::2].shape)     # M_x <= M_f
        if e == 2:
            U[:] = 0.0
        if e == 3:
            Ud = rng.choice([0.0, 90.0, 180.0, 270.0, 359.9], size=(H, W))
        layers.append((w0, de, mx, sg, steps + 37.0 * e, U, Ud))
        eng.set_layers(*layers[-1], env=e)
    for e in range(E):
        o = fire_dense.DenseOracle(**dict(kw, n_envs=1))
        o.build_rtable(*layers[e], M_f)
        T = eng.get_rtable(e)
        check(T, o.get_rtable(), ("layers", W, e))
        if e == 0:
            assert (T[:, :, ::3] == 0.0).all()
    # from fuel-code rasters (non-burnable codes: w_0 = 0 -> R = 0)
    for e in range(E):
        codes = rng.choice([1, 2, 4, 5, 8, 9, 10, 13, 91, 98], size=(H, W)).astype(np.int32)
        U = np.zeros((H, W)) if e == 2 else rng.uniform(0, 900, (H, W))
        Ud = rng.choice([0.0, 90.0, 180.0, 270.0, 359.9], size=(H, W))
        eng.set_layers_fbfm(codes, steps * (1 + e), U, Ud, env=e)
        o = fire_dense.DenseOracle(**dict(kw, n_envs=1))
        o.build_rtable(*fuel_planes(codes), steps * (1 + e), U, Ud, M_f)
        T = eng.get_rtable(e)
        check(T, o.get_rtable(), ("fbfm", W, e))
        assert (T[:, np.isin(codes, [91, 98])] == 0.0).all()


# ------------------------------------------------------------------ end to end through the Python surface
def test_batched_simulation_of_six_configs_equals_solo_runs():
    """BatchedFireSimulation(configs, 6) on 96 x 130 configs with their own fuel, elevation and wind; run(n), run(1) loops long
    enough to move to the resident launch, update_mitigation + run pairs: every environment equals FireSimulation(config)."""
    import os
    import yaml
    from simfire_amd.config import Config
    from simfire_amd.simulation import BatchedFireSimulation, FireSimulation
    cfg_dir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "configs")
    y = yaml.safe_load(open(os.path.join(cfg_dir, "test_config_flat_simple.yml")))
    H, W, E = 96, 130, 6
    rng = np.random.default_rng(75000)
    cfgs = []
    for e in range(E):
        codes = rng.choice([1, 2, 3, 4, 5, 8, 10, 91], size=(H, W))
        elev = rng.uniform(0, 40.0 * (e + 1), (H, W))
        speed = np.full((H, W), 200.0 * (e + 1))
        direction = np.full((H, W), 55.0 * e)
        yy = yaml.safe_load(yaml.safe_dump(y))
        yy["fire"]["fire_initial_position"] = {"type": "static", "static": {"position": f"({20 + 15 * e}, {30 + 7 * e})"}}
        cfgs.append(Config.from_arrays(yy, codes, elev, speed, direction))
    ign = [c.fire.fire_initial_position for c in cfgs]
    batch = BatchedFireSimulation(cfgs, E, ignitions=ign)
    solos = [FireSimulation(c) for c in cfgs]
    # run(1) without maps: step(1) + a look at the result rows, which moves to the resident launch after two such pairs (a loop that
    # fetches the maps after every update stays on the per-step kernels)
    plan = [("run", 4), ("run", 9)] + [("poll", 1)] * 8 + [("mit", 3), ("run", 5), ("mit", 4), ("poll", 1), ("poll", 1), ("poll", 1),
                                                          ("run", 12)]
    kinds = []
    for i, (op, v) in enumerate(plan):
        if op == "mit":
            rows = [(e, int(rng.integers(W)), int(rng.integers(H)), v) for e in range(E) for _ in range(15)]
            batch.update_mitigation(rows)
            for e, s in enumerate(solos):
                s.update_mitigation([(x, yy_, t) for (ee, x, yy_, t) in rows if ee == e])
            continue
        maps, active = batch.run(v, return_maps=(op == "run"))
        kinds.append(batch._engine.last_launch_kind())
        st, el = batch._engine.status()
        for e, s in enumerate(solos):
            fm, _ = s.run(v)
            so, eo = s._engine.status()
            assert (st[e] == so[0]).all() and el[e] == eo[0], (i, e)
            if maps is not None:
                assert (maps[e] == fm).all(), (i, e)
    assert kinds[2 + 7] == 2 and kinds[-2] == 2, kinds                # (the run(1) loops moved to the resident launch)
    st, el = batch._engine.status()
    for e, s in enumerate(solos):
        so, eo = s._engine.status()
        assert (st[e] == so[0]).all() and el[e] == eo[0], e
        assert (batch._engine.burn(e) == s._engine.burn(0)).all(), e
    assert not (maps[0] == maps[1]).all()
