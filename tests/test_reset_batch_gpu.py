"""Batched resets on the GPU (``sf_reset_envs`` / ``sf_reset_where``).  The yardsticks are the existing path
- a twin handle reset with the ``sf_reset_env`` loop - and ``oracle/fire_dense.c`` replaying every environment's log from its
last reset; never the new code against itself.  Run with ``pytest -m gpu``."""
import numpy as np
import pytest

from oracle import fire_dense
from test_env_state_gpu import MODES, RESIDENT, _Replay, _check, _world

pytestmark = pytest.mark.gpu


def _make(kw, E, mode, R8, inits, prune=False, graph=False, per_env=False):
    from simfire_amd.engine import FireEngine
    eng = FireEngine(n_envs=E, per_env_terrain=per_env, **kw)
    m = MODES[mode]
    eng.set_fused(m["fused"])
    if m.get("tuning"):
        eng.set_tuning(**m["tuning"])
    if prune:
        eng.set_prune_after_quit(True)
    if graph:
        eng.enable_spread_graph(True)
    if per_env:
        for e in range(E):
            eng.set_rtable(R8[e], env=e)
    else:
        eng.set_rtable(R8)
    eng.reset(inits)
    return eng


def _blobs(eng):
    return eng.save_state(list(range(eng.n_envs)))


def _same(a, b, tag):
    ba, bb = _blobs(a), _blobs(b)
    for e in range(a.n_envs):
        assert ba[e].tobytes() == bb[e].tobytes(), (tag, "state blob of environment", e)
    sa, ea = a.status()
    sb, eb = b.status()
    assert (sa == sb).all() and ea.tobytes() == eb.tobytes(), (tag, sa, sb)
    return bb


def _points(rng, E, H, W, p=0.35):
    pts = []
    for e in range(E):
        if rng.random() < p:
            pts += [(e, int(rng.integers(W)), int(rng.integers(H)), int(rng.integers(3, 6))) for _ in range(int(rng.integers(1, 5)))]
    return pts


# ------------------------------------------------------------------ 1. equal to the sf_reset_env loop
def _twin_world(seed, mode, H, W, md, att, prune=False, graph=False, E=None, before=(4, 14), after=(10, 31)):
    """Handles A and B built alike and driven through the same random log; at a random update a random subset is reset - A with the
    ``sf_reset_env`` loop, B with one ``sf_reset_envs``.  All state blobs and the result block equal then and after 10 - 30 further
    updates; on B the blobs of the environments that were not reset are what they were before the call."""
    rng = np.random.default_rng(seed)
    E = int(rng.integers(4, 9)) if E is None else E
    kw, R8 = _world(rng, H, W, md, att, diag=True)
    inits = [(int(rng.integers(W)), int(rng.integers(H))) for _ in range(E)]
    a, b = (_make(kw, E, mode, R8, inits, prune, graph) for _ in range(2))
    resident = mode in RESIDENT and md <= 5 and not graph
    chunk = 1 if mode in ("fused0", "fused1") else int(rng.integers(2, 4))

    def drive(n_updates):
        t = 0
        while t < n_updates:
            pts = _points(rng, E, H, W)
            n = min(chunk, n_updates - t)
            for x in (a, b):
                if pts:
                    x.apply_mitigation(pts)
                x.step(n)
            t += n

    drive(int(rng.integers(*before)))
    _same(a, b, (seed, mode, "before the reset"))            # (save_state / status read the plane that is current: no conversion)
    layout = b.cell_layout()
    assert a.cell_layout() == layout
    if mode != "run_kwin":                                   # (the automatic choice may step a small grid with the per-step kernels)
        assert layout == (1 if resident else 0), (mode, layout)
    was = _blobs(b)
    envs = rng.choice(E, size=int(rng.integers(1, E)), replace=False).astype(np.int32)
    xy = np.stack([rng.integers(0, W, len(envs)), rng.integers(0, H, len(envs))], axis=1).astype(np.int32)
    for e, (x, y) in zip(envs, xy):
        a.reset_env(int(e), int(x), int(y))
    b.reset_envs(envs, xy)
    assert b.cell_layout() == layout and a.cell_layout() == layout
    now = _same(a, b, (seed, mode, "after the reset", envs.tolist()))
    for e in range(E):
        if e not in envs:
            assert now[e].tobytes() == was[e].tobytes(), (seed, mode, "environment not reset changed", e)
    drive(int(rng.integers(*after)))
    _same(a, b, (seed, mode, "at the end"))
    assert a.fire_maps().tobytes() == b.fire_maps().tobytes()
    for e in range(E):
        assert a.burn(e).tobytes() == b.burn(e).tobytes(), (seed, mode, e)
        if graph:
            assert (a.spread_parents(e) == b.spread_parents(e)).all()
    assert b.status()[0][:, 1].max() > 0


CASES = {
    "37x101_md4_att": dict(H=37, W=101, md=4, att=True),
    "64x64_md7": dict(H=64, W=64, md=7, att=False),
    "225x225_md4_prune": dict(H=225, W=225, md=4, att=False, prune=True),
    "225x225_md4_att_graph": dict(H=225, W=225, md=4, att=True, graph=True),
    "225x225_md4_att": dict(H=225, W=225, md=4, att=True),
}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", list(CASES))
def test_equal_to_the_reset_env_loop(case, mode):
    _twin_world(81000 + 17 * list(CASES).index(case) + list(MODES).index(mode), mode, **CASES[case])


@pytest.mark.parametrize("mode", ["run", "fused1"])
def test_equal_to_the_reset_env_loop_1024(mode):
    _twin_world(82000 + len(mode), mode, H=1024, W=1024, md=4, att=True, E=4, before=(20, 30), after=(10, 20))


# ------------------------------------------------------------------ 2. equal to the oracle
@pytest.mark.parametrize("mode", list(MODES))
def test_equal_to_the_oracle(mode):
    """Every environment's log restarts at its reset; after every update fire_map, burn, result row and elapsed_time equal the
    oracle replaying the log.  Resets follow the launch the mode names directly (its plane is the current one)."""
    rng = np.random.default_rng(83000 + list(MODES).index(mode))
    H, W = (150, 165) if mode in ("run_team", "run_win", "run_kwin") else (61, 83)
    E, md = 6, 4
    kw, R8 = _world(rng, H, W, md, True, diag=True)
    kw.update(max_time=5.0, update_rate=1.0, pixel_scale=20.0)      # every episode QUITs on the runtime check at its 7th update
    R8[:] = np.maximum(R8, 30.0)                                    # (a burning cell passes its fire on in one update: no fire dies before)
    inits = [(int(rng.integers(W)), int(rng.integers(H))) for _ in range(E)]
    eng = _make(kw, E, mode, R8, inits)
    rep = _Replay(kw, False, False)
    logs = [[("table", 0), ("reset", inits[e])] for e in range(E)]
    refs = {e: rep.run(logs[e], [R8]) for e in range(E)}
    resident = mode in RESIDENT
    chunk = 1 if not resident else 2
    x0, x15 = 16 * int(rng.integers(1, W // 16)), 16 * int(rng.integers(1, W // 16)) + 15
    # update -> list of reset_envs calls (environments, ignitions)
    events = {
        4: [([0, 1, 0], [(5, 5), (W - 1, H - 1), (x0, int(rng.integers(H)))])],                 # still burning; 0 is named twice: its last ignition wins
        12: [([2, 3], [(0, 0), (x15, int(rng.integers(H)))]),                                  # after QUIT; a grid corner
             ([3], [(int(rng.integers(W)), int(rng.integers(H)))])],                           # twice in a row
        16: [([4, 5, 1], [(0, H - 1), (W - 1, 0), (x0 + 15, 0)])],
    }
    running_at = {4: [0, 1], 12: [], 16: []}
    quit_at = {4: [], 12: [2, 3], 16: [4, 5]}
    t, steps = 0, 26
    while t < steps:
        pts = _points(rng, E, H, W)
        for (e, x, y, ty) in pts:
            logs[e].append(("mit", [(x, y, ty)]))
            rep.apply(refs[e], ("mit", [(x, y, ty)]), [R8])
        if pts:
            eng.apply_mitigation(pts)
        n = min(chunk, steps - t)
        eng.step(n)
        t += n
        for e in range(E):
            logs[e] += [("step",)] * n
            for _ in range(n):
                rep.apply(refs[e], ("step",), [R8])
        if t in events:
            if mode != "run_kwin":
                assert eng.cell_layout() == (1 if resident else 0), (mode, t)      # straight after the launch: its plane is current
            for e in running_at[t]:
                assert refs[e].status()[0][0, 0] == 1, (t, e)
            for e in quit_at[t]:
                assert refs[e].status()[0][0, 0] == 0, (t, e)
            for envs, xy in events[t]:
                eng.reset_envs(envs, xy)
                for e, p in zip(envs, xy):                 # (in order: a later entry of the same environment replaces the earlier one)
                    logs[e] = [("table", 0), ("reset", p)]
                    refs[e] = rep.run(logs[e], [R8])
        for e in range(E):
            _check(eng, e, refs[e], (mode, t, e))


# ------------------------------------------------------------------ 3. the mask form
def _mask_world(mode):
    """64 x 64, six environments with tables of their own: 0, 2 and 5 cannot spread (their fires are out after max_fire_duration
    updates), the others spread for ever.  Two handles alike, and the split checked with the oracle."""
    H = W = 64
    E, out = 6, [0, 2, 5]
    kw = dict(shape=(H, W), max_fire_duration=4, pixel_scale=50.0, update_rate=1.0, max_time=None, attenuate_line_ros=True,
              diagonal_spread=True)
    tabs = [np.full((8, H, W), 0.0 if e in out else 30.0) for e in range(E)]
    inits = [(20, 30)] * E
    for e in (0, 1):
        o = fire_dense.DenseOracle(**kw)
        o.set_rtable(tabs[e])
        o.reset([(20, 30)])
        o.step(6)
        assert o.status()[0][0, 0] == (0 if e == 0 else 1)
    a, b = (_make(kw, E, mode, tabs, inits, per_env=True) for _ in range(2))
    for x in (a, b):
        x.step(6)
    st = b.status()[0]
    assert sorted(np.flatnonzero(st[:, 0] == 0).tolist()) == out and (st[[1, 3, 4], 0] == 1).all()      # both kinds exist
    return a, b, kw, tabs, out


@pytest.mark.parametrize("mode", ["fused0", "run"])
def test_mask_form(mode):
    import torch
    a, b, kw, tabs, out = _mask_world(mode)
    E, W, H = 6, 64, 64
    rng = np.random.default_rng(84000)
    xy = np.stack([rng.integers(0, W, E), rng.integers(0, H, E)], axis=1).astype(np.int32)
    # not running, decided on the device
    done = np.flatnonzero(a.status()[0][:, 0] == 0)
    a.reset_envs(done, xy[done])
    b.reset_where(None, xy)
    _same(a, b, "reset_where(None)")
    assert (b.status()[0][:, 0] == 1).all()
    for x in (a, b):
        x.step(3)
    _same(a, b, "3 updates later")
    # an explicit mask that also selects running environments; bool and uint8; ignitions as a device tensor
    for dtype, sel in ((torch.uint8, [1, 2, 4]), (torch.bool, [0, 3])):
        mask = torch.zeros(E, dtype=dtype, device="cuda")
        mask[sel] = 1
        xy = np.stack([rng.integers(0, W, E), rng.integers(0, H, E)], axis=1).astype(np.int32)
        a.reset_envs(sel, xy[sel])
        b.reset_where(mask, torch.from_numpy(xy).cuda() if dtype is torch.bool else xy)
        _same(a, b, ("explicit mask", sel))
        for x in (a, b):
            x.step(2)
    # nothing selected: nothing changes
    was = _blobs(b)
    b.reset_where(torch.zeros(E, dtype=torch.uint8, device="cuda"), xy)
    now = _blobs(b)
    assert now.tobytes() == was.tobytes()
    # a device ignition off the grid: that environment is left as it is - not running -, the others are reset
    for x in (a, b):
        x.step(6)                                        # the fires of 0, 2, 5 are out again
    done = np.flatnonzero(a.status()[0][:, 0] == 0)
    assert len(done) >= 2
    bad = int(done[1])
    was = _blobs(b)
    dxy = torch.from_numpy(xy).cuda()
    dxy[bad, 0] = W
    others = [int(e) for e in done if e != bad]
    a.reset_envs(others, xy[others])
    b.reset_where(None, dxy)
    now = _same(a, b, "ignition off the grid")
    assert now[bad].tobytes() == was[bad].tobytes()
    st = b.status()[0]
    assert st[bad, 0] == 0 and (st[others, 0] == 1).all() and (st[others, 1] == 0).all()
    # ... and the episodes that follow are the oracle's
    for x in (a, b):
        x.step(4)
    for e in others:
        o = fire_dense.DenseOracle(**kw)
        o.set_rtable(tabs[e])
        o.reset([tuple(int(v) for v in xy[e])])
        o.step(4)
        _check(b, e, o, ("oracle", e))


def test_mask_form_takes_environments_that_quit_and_still_prune():
    """``prune_after_quit``: an environment that QUIT on the runtime check keeps pruning (its state word is 2) and its result row says
    not running - the maskless form takes it like the list built from the result block."""
    rng = np.random.default_rng(84500)
    H, W, E = 60, 70, 5
    kw, R8 = _world(rng, H, W, 4, True)
    kw.update(max_time=4.0, update_rate=1.0, pixel_scale=20.0)
    R8[:] = np.maximum(R8, 30.0)
    inits = [(int(rng.integers(W)), int(rng.integers(H))) for _ in range(E)]
    a, b = (_make(kw, E, "fused0", R8, inits, prune=True) for _ in range(2))
    for x in (a, b):
        x.step(4)
        x.reset_env(1, 9, 9)                                # (one environment younger than the others: still running below)
        x.step(3)
    st = a.status()[0]
    assert st[1, 0] == 1 and (st[[0, 2, 3, 4], 0] == 0).all() and (st[:, 3] > 0).all()      # QUIT with cells still burning: pruning goes on
    xy = np.stack([rng.integers(0, W, E), rng.integers(0, H, E)], axis=1).astype(np.int32)
    done = np.flatnonzero(st[:, 0] == 0)
    a.reset_envs(done, xy[done])
    b.reset_where(None, xy)
    _same(a, b, "prune_after_quit")
    for x in (a, b):
        x.step(5)
    _same(a, b, "prune_after_quit, 5 updates later")


# ------------------------------------------------------------------ 4. neighbours keep working
def test_fire_map_delta_after_a_batched_reset():
    rng = np.random.default_rng(85000)
    H, W, E = 70, 90, 4
    kw, R8 = _world(rng, H, W, 4, True)
    R8[:] = np.maximum(R8, 7.5)
    eng = _make(kw, E, "fused0", R8, [(10, 10), (20, 20), (30, 30), (40, 40)])
    for e in range(E):
        eng.fire_map_delta(e)                               # (the first query sets the reference point up)
    eng.step(5)
    for e in range(E):
        assert eng.fire_map_delta(e) is not None
    eng.step(2)
    eng.reset_envs([1, 3], [(17, 3), (0, 69)])
    for e, (x, y) in ((1, (17, 3)), (3, (0, 69))):
        idx, val = eng.fire_map_delta(e)
        assert idx.tolist() == [y * W + x] and val.tolist() == [1], (e, idx, val)      # exactly the ignition cell, BURNING
    assert eng.fire_map_delta(0) is not None                # an environment that was not reset keeps its reference point
    eng.step(3)
    eng.reset_where(None, np.array([(1, 1)] * E, dtype=np.int32))      # (whoever is selected, here nobody: the host cannot know)
    for e in range(E):
        assert eng.fire_map_delta(e) is None                # -1 once: fetch the whole map
    maps = eng.fire_maps().copy()
    eng.step(2)
    for e in range(E):
        idx, val = eng.fire_map_delta(e)                    # ... then deltas again
        m = maps[e].reshape(-1).copy()
        m[idx] = val
        assert (m.reshape(H, W) == eng.fire_map(e)).all(), e


@pytest.mark.parametrize("fused", [0, 2])
def test_observe_and_render_of_a_reset_environment(fused):
    import torch
    import test_observe_gpu as TO
    import test_render_gpu as TR
    eng, rng = TO._engine(90, 140, 4, 86000 + fused)
    eng.set_fused(fused)
    eng.step(7)
    assert eng.cell_layout() == (1 if fused == 2 else 0)
    eng.reset_envs([0, 2], [(139, 0), (64, 45)])
    TO._check(eng, agents=TO._agents(rng, 4, 90, 140))      # (observe first: it reads the plane the reset wrote)
    assert eng.fire_map(0)[0, 139] == 1 and (eng.fire_map(0) != 0).sum() == 1
    w = TR._World(90, 140, 4, 86100 + fused)
    w.eng.set_fused(fused)
    w.eng.step(7)
    mask = torch.tensor([0, 1, 0, 1], dtype=torch.uint8, device="cuda")
    w.eng.reset_where(mask, np.array([(0, 0), (3, 89), (5, 5), (128, 40)], dtype=np.int32))
    TR._check(w, agents=TR._agents(w.rng, 4, 90, 140))
    assert (w.eng.fire_map(3) != 0).sum() == 1 and w.eng.fire_map(3)[40, 128] == 1


@pytest.mark.parametrize("mode", ["fused1", "run"])
def test_clone_from_a_freshly_reset_environment(mode):
    rng = np.random.default_rng(87000)
    H, W, E = 80, 100, 4
    kw, R8 = _world(rng, H, W, 4, True)
    inits = [(int(rng.integers(W)), int(rng.integers(H))) for _ in range(E)]
    eng = _make(kw, E, mode, R8, inits)
    eng.step(6)
    eng.reset_envs([2], [(33, 44)])
    eng.copy_envs([2, 2], [0, 3])
    log = [("table", 0), ("reset", (33, 44))]
    rep = _Replay(kw, False, False)
    for t in range(8):
        eng.step(2)
        log += [("step",)] * 2
        ref = rep.run(log, [R8])
        for e in (0, 2, 3):
            _check(eng, e, ref, (mode, t, e))
    ref1 = rep.run([("table", 0), ("reset", inits[1])] + [("step",)] * 22, [R8])
    _check(eng, 1, ref1, "not reset")


def test_closed_loop_after_reset_done():
    """``reset_done`` with a mask, then a closed-loop episode against the oracle; ``reset_done`` while the loop runs ends it and
    still resets correctly."""
    import torch
    from test_env_state_gpu import _batched
    sim = _batched(4)
    eng = sim._engine
    H = W = 96
    kw = dict(shape=(H, W), max_fire_duration=int(eng.params.max_fire_duration), pixel_scale=float(eng.params.pixel_scale),
              update_rate=float(eng.params.update_rate), max_time=(float(eng.params.max_time) if eng.params.has_max_time else None),
              attenuate_line_ros=bool(eng.params.attenuate_line_ros), diagonal_spread=bool(eng.params.diagonal_spread))
    R8 = eng.get_rtable(0)
    orcs = []
    for e in range(4):
        o = fire_dense.DenseOracle(**kw)
        o.set_rtable(R8)
        o.reset([tuple(int(v) for v in sim.ignitions[e])])
        orcs.append(o)
    sim.run(9, return_maps=False)
    for o in orcs:
        o.step(9)
    sim.ignitions[1] = (80, 15)
    sim.ignitions[3] = (0, 95)
    sim.reset_done(torch.tensor([0, 1, 0, 1], dtype=torch.bool, device="cuda"))
    for e in (1, 3):
        orcs[e].reset([tuple(int(v) for v in sim.ignitions[e])])
    rng = np.random.default_rng(88000)

    def episode(n):
        for _ in range(n):
            pts = np.stack([rng.integers(0, W, (4, 2)), rng.integers(0, H, (4, 2)), rng.integers(3, 6, (4, 2))], axis=2).astype(np.int32)
            rows, el = sim.loop_step(pts)
            for e in range(4):
                orcs[e].apply_mitigation([(0, int(x), int(y), int(ty)) for (x, y, ty) in pts[e]])
                orcs[e].step(1)
                so, eo = orcs[e].status()
                assert (rows[e] == so[0]).all() and el[e] == eo[0], (e, rows[e], so[0])

    sim.loop_start(2)
    episode(7)
    sim.ignitions[0] = (50, 50)
    sim.reset_done(torch.tensor([1, 0, 0, 0], dtype=torch.uint8, device="cuda"))      # the loop is running: it is ended first
    orcs[0].reset([(50, 50)])
    with pytest.raises(Exception, match="loop_start"):
        eng.loop_step(None)
    for e in range(4):
        _check(eng, e, orcs[e], ("after reset_done in the loop", e))
    sim.loop_start(2)
    episode(5)
    sim.loop_stop()
    for e in range(4):
        _check(eng, e, orcs[e], ("at the end", e))


# ------------------------------------------------------------------ 5. seeds through the one batched call
@pytest.mark.parametrize("kind", [0, 2])
def test_layer_seeds_and_reset_of_a_list(kind):
    import test_layer_gen_gpu as TL
    from simfire_amd.config import Config
    from simfire_amd.simulation import BatchedFireSimulation
    H, W, E = 128, 144, 6
    listed = [1, 3, 4]
    default = (827, 1113, 2345, 650)
    seeds = [((11 * e - 20, 1113 + e, 300 + 7 * e, 650 - 3 * e) if e in listed else default) for e in range(E)]
    sim = BatchedFireSimulation(Config(config_dict=TL._dict(H, W), simplex_topography=True), E, per_env_terrain=True)
    sim._engine.set_fused(kind)
    sim.run(10, return_maps=False)
    assert sim.set_seeds({"elevation": [seeds[e][0] for e in listed], "fuel": [seeds[e][1] for e in listed],
                          "wind_speed": [seeds[e][2] for e in listed], "wind_direction": [seeds[e][3] for e in listed]}, envs=listed) is True
    calls = {"reset_envs": 0, "reset_env": 0}
    for name in calls:
        def counted(*a, _f=getattr(sim._engine, name), _n=name, **k):
            calls[_n] += 1
            return _f(*a, **k)
        setattr(sim._engine, name, counted)
    sim.reset(listed)
    assert calls == {"reset_envs": 1, "reset_env": 0}
    host = TL._host_batch(H, W, seeds, None, ignitions=sim.ignitions.copy())
    host._engine.set_fused(kind)
    for e in listed:
        assert sim._engine.get_rtable(e).tobytes() == host._engine.get_rtable(e).tobytes()
    for it in range(3):
        sim.run(12, return_maps=False)
        host.run(12, return_maps=False)
        sa, ea = sim.results()
        sb, eb = host.results()
        np.testing.assert_array_equal(sa[listed], sb[listed])
        assert ea[listed].tobytes() == eb[listed].tobytes()
        for e in listed:
            assert sim._engine.fire_map(e).tobytes() == host._engine.fire_map(e).tobytes(), (it, e)
            assert sim._engine.burn(e).tobytes() == host._engine.burn(e).tobytes(), (it, e)
    assert sim.results()[0][listed, 1].min() > 0


# ------------------------------------------------------------------ 6. async mode
@pytest.mark.parametrize("mode", ["fused0", "run"])
def test_async_mode(mode):
    rng = np.random.default_rng(89000)
    H, W, E = 120, 130, 5
    kw, R8 = _world(rng, H, W, 4, True)
    inits = [(int(rng.integers(W)), int(rng.integers(H))) for _ in range(E)]
    a, b = (_make(kw, E, mode, R8, inits) for _ in range(2))
    b.set_async(True)
    for x in (a, b):
        x.step(8)
        x.reset_envs([4, 0], [(129, 119), (16, 7)])
        x.step(5)
        x.reset_envs([1], [(3, 3)])
        x.reset_envs([2, 1], [(64, 64), (15, 100)])      # back to back: the second call's list follows the first through the pinned buffer
        x.step(3)
    b.sync()
    _same(a, b, "async")
