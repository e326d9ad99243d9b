"""Fire influence on the GPU (``sf_influence``).  The yardstick is ``tests/_influence_oracle.py`` - the definition,
and its leaf-peeling restatement where a grid is large - fed with what is fetched AFTER the call (parent masks, arrivals, the forecast's
``pred``).  Every comparison is equality: all results are integers and integer addition commutes, so no bit may depend on how the
walkers are scheduled.  Run with ``pytest -m gpu``."""
import ctypes as C
import os

import numpy as np
import pytest

import _influence_oracle as io
import _influence_worlds as iw
import _travel_worlds as tw

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tests", "golden", "configs")
PLANES = ("cells", "value", "pred")
COUNTS = ("forest", "roots", "cyclic")
_cache = {}


def _want(pred, include=None, weights=None, inclusive=False):
    """The oracle's answer, computed once per request and left unchanged."""
    key = (pred.shape, pred.tobytes(), None if include is None else include.tobytes(), None if weights is None else weights.tobytes(), inclusive)
    if key not in _cache:
        _cache[key] = io.answer_peel(pred, include, weights, inclusive)
    return _cache[key]


def _engine(H, W, E, per_env=False, reset=True):
    from simfire_amd.engine import FireEngine
    eng = FireEngine(n_envs=E, per_env_terrain=per_env, **iw.engine_kwargs(H, W))
    if not per_env:
        eng.set_rtable(np.full((8, H, W), 1e-3))
    if reset:
        eng.reset(np.zeros((E, 2), dtype=np.int32))
    return eng


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(r, eng):
    eng.sync()                                               # (a handle in async mode has only enqueued)
    assert all(v.is_cuda for v in r.values())
    return {k: v.cpu().numpy() for k, v in r.items()}


def _same(r, i, want, tag, pts=None, R=0):
    """Row ``i`` of every output ``r`` holds equals the oracle's answer."""
    for name in PLANES:
        if name in r:
            bad = np.argwhere(r[name][i] != want[name])
            assert r[name].dtype == want[name].dtype and not len(bad), (tag, i, name, len(bad), bad[:5].tolist())
    for name in COUNTS:
        if name in r:
            assert r[name].dtype == np.int32 and int(r[name][i]) == want[name], (tag, i, name, int(r[name][i]), want[name])
    if pts is not None:
        wp = io.points(want, pts, R)
        for name, w in wp.items():
            assert r[name].dtype == w.dtype and np.array_equal(r[name][i], w), (tag, i, name, r[name][i].tolist()[:8], w.tolist()[:8])


# ---------------------------------------------------------------------------------------------- 1. the scenes
@pytest.mark.parametrize("shape", iw.SCENE_SHAPES, ids=["%dx%d" % s for s in iw.SCENE_SHAPES])
def test_scenes(shape):
    """Every scene in a row of its own of ONE call (a plane per listed environment; the list repeats the three environments), with
    weights per environment number, a shared include plane, points and routes, all outputs together; then ``inclusive``, each output
    alone - the accumulators then live in scratch - and the plain request.  Then every scene as ONE plane shared by a list of two."""
    H, W = shape
    sc = iw.scenes(H, W)
    n, E, R = len(sc), 3, 16
    eng = _engine(H, W, E)
    envs = [i % E for i in range(n)]
    pred = np.stack([s["pred"] for s in sc])
    w3 = np.stack([iw.weights(H, W, e) for e in range(E)])
    inc = iw.include(H, W)
    pts = np.stack([iw.default_points(H, W, i) for i in range(n)])
    d_pred, d_w, d_inc, d_pts = _dev(pred), _dev(w3), _dev(inc), _dev(pts)
    kw = dict(pred=d_pred, envs=envs, weights=d_w, include=d_inc)
    both = _np(eng.influence(points=d_pts, max_route=R, value=True, pred_out=True, counts=True, **kw), eng)
    assert set(both) == set(PLANES) | set(COUNTS) | {"point_cells", "point_value", "point_route", "point_hops"}
    incl = _np(eng.influence(inclusive=True, value=True, **kw), eng)
    alone = dict(cells=_np(eng.influence(**kw), eng), value=_np(eng.influence(cells=False, value=True, **kw), eng),
                 pred=_np(eng.influence(cells=False, pred_out=True, pred=d_pred, envs=envs), eng),
                 counts=_np(eng.influence(cells=False, counts=True, pred=d_pred, envs=envs), eng),
                 points=_np(eng.influence(cells=False, points=d_pts, max_route=R, **kw), eng))
    plain = _np(eng.influence(pred=d_pred, envs=envs, counts=True), eng)
    for i, s in enumerate(sc):
        tag = (shape, s["name"])
        _same(both, i, _want(s["pred"], inc, w3[envs[i]]), tag, pts[i], R)
        _same(incl, i, _want(s["pred"], inc, w3[envs[i]], True), tag + ("inclusive",))
        _same(plain, i, _want(s["pred"]), tag + ("plain",))
    assert list(alone["cells"]) == ["cells"] and list(alone["value"]) == ["value"] and list(alone["pred"]) == ["pred"] and set(alone["counts"]) == set(COUNTS)
    assert set(alone["points"]) == {"point_cells", "point_value", "point_route", "point_hops"}
    for part in alone.values():
        for name, v in part.items():
            assert np.array_equal(v, both[name]), (shape, "alone", name)
    for s in sc:
        r = _np(eng.influence(pred=_dev(s["pred"]), envs=[2, 0], counts=True), eng)
        for i in range(2):
            _same(r, i, _want(s["pred"]), (shape, s["name"], "shared"))


def test_routes_below_at_and_above_their_length():
    """The serpentine's leaf is 80 hops from its root on 9 x 9: ``max_route`` 80 cuts the route short, 81 holds it exactly, 82 leaves
    one entry unwritten; on the cycle scenes a route never ends."""
    H = W = 9
    eng = _engine(H, W, 2)
    s = iw.serpentine(H, W)
    pts = np.array([[(W - 1, H - 1, 1), (0, 0, 1), (4, 4, 0)]] * 2, dtype=np.int32)
    for R, hops in ((80, -2), (81, 80), (82, 80)):
        r = _np(eng.influence(pred=_dev(s), envs=[0, 1], points=_dev(pts), max_route=R, cells=False), eng)
        assert r["point_hops"].tolist() == [[hops, 0, -1]] * 2 and r["point_route"].shape == (2, 3, R)
        _same(r, 1, _want(s), ("route", R), pts[1], R)
        assert r["point_route"][0, 0, -1] == (1 if R == 80 else 0 if R == 81 else -1)
    for make, at in ((iw.two_cycle, (1, 1)), (iw.fed_cycle, (2, H - 1))):
        p = make(H, W)
        q = np.array([[at + (1,)]], dtype=np.int32)
        r = _np(eng.influence(pred=_dev(p), envs=[1], points=_dev(q), max_route=40), eng)
        _same(r, 0, _want(p), ("cycle", at), q[0], 40)
        assert r["point_hops"].tolist() == [[-2]] and (r["point_route"] >= 0).all()


# ---------------------------------------------------------------------------------------------- 2. the history source
@pytest.mark.parametrize("shape,lines", [((33, 17), False), ((64, 64), False), ((33, 17), True)], ids=["33x17", "64x64", "33x17_lines_on_burning"])
def test_history(shape, lines):
    """Real rollouts of 41 updates, a terrain per environment, graph and arrival on from the reset; with ``lines`` control lines are
    drawn on burning cells between the step calls (a later ignition then ORs later parents into a mask).  The parent masks and the
    arrivals are fetched afterwards and fed to the oracle; ``value`` is weighted by the handle's value plane."""
    H, W = shape
    E = 4
    rng = np.random.default_rng(2810 + H + int(lines))
    eng = _engine(H, W, E, per_env=True, reset=False)
    for e in range(E):
        eng.set_rtable(tw.random_rates(rng, H, W, dead=0.05), env=e)
    eng.enable_spread_graph(True)
    eng.enable_arrival(True)
    eng.reset(np.stack([rng.integers(W // 4, W - W // 4, size=E), rng.integers(H // 4, H - H // 4, size=E)], axis=1).astype(np.int32))
    vals = rng.integers(-1000, 1000, size=(E, H, W)).astype(np.int32)
    eng.values_set(vals)
    for n_up in (7, 11, 23):
        if lines:
            rows = []
            for e in range(E):
                ys, xs = np.nonzero(eng.fire_map(e) == 1)
                rows += [(e, int(xs[j]), int(ys[j]), 3 + j % 3) for j in range(0, len(ys), 3)]
            assert rows
            eng.apply_mitigation(rows)
        eng.step(n_up)
    envs = [3, 0, 1, 2, 0]
    pts = np.stack([iw.default_points(H, W, 50 + i) for i in range(len(envs))])
    r = _np(eng.influence(history=True, envs=envs, weights="values", value=True, pred_out=True, counts=True, points=_dev(pts), max_route=24), eng)
    only = _np(eng.influence(history=True, envs=envs, cells=False, pred_out=True), eng)
    assert np.array_equal(only["pred"], r["pred"])
    trees = []
    for i, e in enumerate(envs):
        codes = io.history_codes(eng.spread_parents(e), eng.arrival(e))
        want = _want(codes, None, vals[e])
        assert want["cyclic"] == 0 and want["forest"] > 20, (shape, e, want["forest"])
        _same(r, i, want, (shape, lines, e), pts[i], 24)
        trees.append(want["forest"])
        arr = eng.arrival(e)
        assert want["roots"] >= 1 and (r["pred"][i][arr < 0] == -1).all()
    assert len(set(trees)) > 1                                # the environments' fires differ


# ---------------------------------------------------------------------------------------------- 3. the forecast source
@pytest.mark.parametrize("max_minutes", [None, 1.0])
def test_forecast(max_minutes):
    """``travel(pred=True, reached=True)`` fed into ``influence`` without a host copy: every reached cell hangs below a root, so the
    roots' ``cells`` add up to ``reached``; the oracle runs on the fetched ``pred``."""
    H, W, E = 40, 130, 3
    rng = np.random.default_rng(2820)
    eng = _engine(H, W, E, per_env=True, reset=False)
    for e in range(E):
        eng.set_rtable(tw.random_rates(rng, H, W), env=e)
    eng.reset(np.zeros((E, 2), dtype=np.int32))
    for e in range(E):
        eng.load_fire_map(e, tw.random_map(rng, H, W))
    t = eng.travel(plane=False, pred=True, reached=True, max_minutes=max_minutes)
    r = _np(eng.influence(pred=t["pred"], counts=True, pred_out=True), eng)
    pred, reached = t["pred"].cpu().numpy(), t["reached"].cpu().numpy()
    for e in range(E):
        _same(r, e, _want(pred[e]), ("forecast", max_minutes, e))
        roots = (r["pred"][e] < 0) & (r["cells"][e] > 0)
        assert int(r["cells"][e][roots].sum()) == int(reached[e]) == int(r["forest"][e]) > 0 and int(roots.sum()) == int(r["roots"][e])
        assert int(r["cyclic"][e]) == 0
    if max_minutes is not None:
        full = _np(eng.travel(plane=False, reached=True), eng)["reached"]
        assert (reached < full).any()


def _config_24x40():
    import yaml
    from simfire_amd.config import Config
    y = yaml.safe_load(open(os.path.join(CFG, "functional_config.yml")))
    y["area"]["screen_size"] = [24, 40]
    y["terrain"]["topography"]["functional"]["function"] = "flat"
    y["simulation"]["headless"] = True
    return Config(config_dict=y)


def test_batched_simulation_forecast_with_a_horizon():
    from simfire_amd.simulation import BatchedFireSimulation
    bat = BatchedFireSimulation(_config_24x40(), 3)
    bat.run(3, return_maps=False)
    eng = bat._engine
    t = _np(eng.travel(plane=True, pred=True), eng)           # (the simulation classes run their handle in async mode: wait before reading)
    horizon = float(np.median(t["minutes"][np.isfinite(t["minutes"]) & (t["minutes"] > 0)]))
    r = bat.fire_influence("forecast", envs=[2, 0], horizon=horizon, counts=True, pred_out=True, device=False)
    whole = bat.fire_influence("forecast", envs=[2, 0], device=False)
    for i, e in enumerate((2, 0)):
        inc = ((t["minutes"][e] >= 0) & (t["minutes"][e] <= horizon)).astype(np.uint8)
        assert 0 < inc.sum() < inc.size
        _same(r, i, _want(t["pred"][e], inc), ("horizon", e))
        _same(whole, i, _want(t["pred"][e]), ("forecast", e))
    assert (r["cells"] <= whole["cells"]).all() and (r["cells"] < whole["cells"]).any()
    with pytest.raises(ValueError, match="fire_influence"):
        bat.fire_influence("history", horizon=3.0)


# ---------------------------------------------------------------------------------------------- 4. lists, chunks, many environments
def test_lists_with_repeats_and_chunks():
    """A list with repeats, worked through in chunks of two and of one under a small ``scratch_bytes``: the same bits as the default;
    the scratch is counted by ``memory_bytes``."""
    H, W, E = 40, 130, 3
    eng = _engine(H, W, E)
    sc = iw.scenes(H, W)
    envs = [2, 0, 2, 1, 1, 0, 2]
    pred = np.stack([sc[(3 * i) % len(sc)]["pred"] for i in range(len(envs))])
    w = iw.weights(H, W, 3)
    pts = np.stack([iw.default_points(H, W, 20 + i) for i in range(len(envs))])
    kw = dict(pred=_dev(pred), envs=envs, weights=_dev(w), points=_dev(pts), max_route=9, value=True, pred_out=True, counts=True)
    before = eng.memory_bytes()
    need = eng.influence_scratch_bytes(weighted=True, value=True)
    two = _np(eng.influence(scratch_bytes=2 * need + 17, **kw), eng)
    assert eng.memory_bytes() == before + 2 * need
    one = _np(eng.influence(scratch_bytes=need, **kw), eng)
    assert eng.memory_bytes() == before + 2 * need            # never shrunk
    deflt = _np(eng.influence(**kw), eng)
    assert eng.memory_bytes() == before + len(envs) * need
    for name in deflt:
        assert np.array_equal(two[name], deflt[name]) and np.array_equal(one[name], deflt[name]), name
    for i in range(len(envs)):
        _same(deflt, i, _want(pred[i], None, w), ("chunks", i), pts[i], 9)
    # without the cells output its accumulator is scratch too: a larger need, the same bits
    need2 = eng.influence_scratch_bytes(cells=False, weighted=True, value=True)
    assert need2 > need
    r = _np(eng.influence(cells=False, scratch_bytes=need2, **kw), eng)
    for name in r:
        assert np.array_equal(r[name], deflt[name]), name
    with pytest.raises(ValueError, match="scratch_bytes"):
        eng.influence(cells=False, scratch_bytes=need2 - 1, **kw)
    assert all(len(v) == 0 for v in eng.influence(pred=_dev(pred[0]), envs=[], counts=True).values())


def test_more_environments_than_cus():
    import torch
    n = torch.cuda.get_device_properties(0).multi_processor_count + 8
    H = W = 9
    eng = _engine(H, W, n)
    pred = np.stack([iw.random_forest(H, W, 300 + i % 40) if i % 5 else np.random.default_rng(i).integers(-2, 9, size=(H, W)).astype(np.int8) for i in range(n)])
    r = _np(eng.influence(pred=_dev(pred), inclusive=True, counts=True), eng)
    for i in range(n):
        _same(r, i, _want(pred[i], None, None, True), ("many", i))
    assert len({int(v) for v in r["forest"]}) > 4 and (r["cyclic"] > 0).any()


# ---------------------------------------------------------------------------------------------- 5. reads only, async
def test_reads_only_and_async_mode():
    """Influence calls of both sources between the step calls of a rollout change neither the state blobs nor the maps; in async mode
    the calls only enqueue, and what they deliver after one wait is what the same calls deliver one by one."""
    H, W, E = 33, 17, 3
    rng = np.random.default_rng(2830)
    R8 = tw.random_rates(rng, H, W, dead=0.05)
    inits = np.array([[8, 16], [4, 5], [12, 28]], dtype=np.int32)
    vals = rng.integers(-50, 50, size=(H, W)).astype(np.int32)
    pred = _dev(iw.random_forest(H, W, 9))
    got = []
    for is_async in (False, True):
        eng = _engine(H, W, E, reset=False)
        eng.set_rtable(R8)
        eng.enable_spread_graph(True)
        eng.enable_arrival(True)
        eng.reset(inits)
        eng.values_set(vals)
        eng.set_async(is_async)
        out = []
        for n_up in (5, 9):
            eng.step(n_up)
            if not is_async:
                blob, maps = eng.save_state(list(range(E))), eng.fire_maps()
            out.append(eng.influence(history=True, weights="values", value=True, pred_out=True, counts=True))
            out.append(eng.influence(pred=pred, envs=[1, 1, 0], cells=False, counts=True))
            if not is_async:
                assert np.array_equal(eng.save_state(list(range(E))), blob) and np.array_equal(eng.fire_maps(), maps)
        eng.sync()
        got.append([{k: v.cpu().numpy() for k, v in r.items()} for r in out])
        if is_async:
            for e in range(E):
                _same(got[1][2], e, _want(io.history_codes(eng.spread_parents(e), eng.arrival(e)), None, vals), ("async", e))
    for x, y in zip(*got):
        assert set(x) == set(y)
        for name in x:
            assert np.array_equal(x[name], y[name]), name
    assert got[0][2]["forest"].min() > 10


# ---------------------------------------------------------------------------------------------- 6. refusals
def test_errors_through_the_raw_call():
    import torch
    from simfire_amd import _lib
    H, W, E = 24, 40, 3
    b = _engine(H, W, E, reset=False)
    L, h = b._L, b._h
    need = b.influence_scratch_bytes()
    cells = torch.full((E, H, W), -7, dtype=torch.int32, device="cuda")
    value = torch.full((E, H, W), -7, dtype=torch.int64, device="cuda")
    cnt = torch.full((E,), -7, dtype=torch.int32, device="cuda")
    pc = torch.full((E, 3), -7, dtype=torch.int32, device="cuda")
    pv = torch.full((E, 3), -7, dtype=torch.int64, device="cuda")
    route = torch.full((E, 3, 4), -7, dtype=torch.int32, device="cuda")
    pred = torch.full((H, W), -1, dtype=torch.int8, device="cuda")
    wts = torch.ones((H, W), dtype=torch.int32, device="cuda")
    pts = torch.zeros((E, 3, 3), dtype=torch.int32, device="cuda")
    all_envs = np.arange(E, dtype=np.int32)

    def rc(n=E, envs=all_envs, reserved=(0, 0), outs=None, **fields):
        p = _lib.SfInfluenceParams(**dict(dict(pred=pred.data_ptr()), **fields))
        p.reserved[0], p.reserved[1] = reserved
        o = _lib.SfInfluenceOut(**(dict(cells=cells.data_ptr()) if outs is None else outs))
        e = None if envs is None else np.ascontiguousarray(envs, dtype=np.int32)
        return L.sf_influence(h, C.byref(p), n, None if e is None else e.ctypes.data_as(C.c_void_p), C.byref(o))

    hist = dict(pred_source=1, pred=None)
    assert rc() == _lib.SF_ESTATE and b"sf_reset" in L.sf_last_error()        # before reset
    b.reset(np.zeros((E, 2), dtype=np.int32))
    assert rc(**hist) == _lib.SF_ESTATE and b"sf_enable_spread_graph" in L.sf_last_error()
    b.enable_spread_graph(True)
    assert rc(**hist) == _lib.SF_ESTATE and b"sf_enable_arrival" in L.sf_last_error()
    assert rc(weight_mode=1, outs=dict(value=value.data_ptr())) == _lib.SF_ESTATE and b"sf_values_set" in L.sf_last_error()
    b.enable_arrival(True)
    withpts = dict(k=3, points=pts.data_ptr())
    routes = dict(point_route=route.data_ptr(), point_hops=pc.data_ptr())
    bad = [dict(pred_source=2), dict(pred_source=-1), dict(weight_mode=3), dict(weight_mode=-1), dict(pred=None), dict(pred_source=1),
           dict(weight_mode=2), dict(weights=wts.data_ptr()), dict(weight_mode=1, weights=wts.data_ptr()),
           dict(outs=dict(value=value.data_ptr())), dict(outs=dict(point_value=pv.data_ptr()), **withpts),
           dict(k=-1), dict(k=257, points=pts.data_ptr(), outs=dict(point_cells=pc.data_ptr())), dict(k=3, outs=dict(point_cells=pc.data_ptr())),
           dict(points=pts.data_ptr()), dict(outs=dict(point_cells=pc.data_ptr())), dict(**withpts),
           dict(max_route=-1, outs=dict(point_cells=pc.data_ptr()), **withpts), dict(max_route=(1 << 20) + 1, outs=routes, **withpts),
           dict(max_route=4, outs=dict(point_route=route.data_ptr()), **withpts), dict(max_route=4, outs=dict(point_hops=pc.data_ptr()), **withpts),
           dict(max_route=4, outs=dict(point_cells=pc.data_ptr()), **withpts), dict(max_route=0, outs=routes, **withpts), dict(max_route=4),
           dict(outs=dict(cells=cells.data_ptr() + 2)), dict(outs=dict(forest=cnt.data_ptr() + 1)), dict(outs=dict(roots=cnt.data_ptr() + 2)),
           dict(outs=dict(cyclic=cnt.data_ptr() + 3)), dict(weight_mode=2, weights=wts.data_ptr(), outs=dict(value=value.data_ptr() + 4)),
           dict(weight_mode=2, weights=wts.data_ptr() + 2), dict(outs=dict(point_cells=pc.data_ptr() + 2), **withpts),
           dict(k=3, points=pts.data_ptr() + 2, outs=dict(point_cells=pc.data_ptr())),
           dict(weight_mode=2, weights=wts.data_ptr(), outs=dict(point_value=pv.data_ptr() + 4), **withpts),
           dict(scratch_bytes=need - 1), dict(scratch_bytes=1), dict(scratch_bytes=-1),
           dict(scratch_bytes=need, outs=dict(forest=cnt.data_ptr())),                    # (without cells the need is larger)
           dict(reserved=(1, 0)), dict(reserved=(0, 1)), dict(outs=dict()),
           dict(envs=[0, E]), dict(envs=[-1, 0], n=2), dict(n=-1), dict(envs=None)]
    for kwargs in bad:
        kwargs = dict(kwargs)
        if "envs" in kwargs and kwargs["envs"] is not None and "n" not in kwargs:
            kwargs["n"] = len(kwargs["envs"])
        assert rc(**kwargs) == _lib.SF_EINVAL, kwargs
        assert b"sf_influence" in L.sf_last_error(), kwargs
    b.sync()
    for t in (cells, value, cnt, pc, pv, route):
        assert (t == -7).all()                                # nothing was enqueued
    assert rc(n=0) == _lib.SF_OK
    assert rc(max_route=4, outs=dict(point_cells=pc.data_ptr(), **routes), **withpts) == _lib.SF_OK      # the call after an error works
    assert rc(**hist) == _lib.SF_OK and rc(scratch_bytes=need) == _lib.SF_OK
    b.sync()
    assert (pc.cpu().numpy() == -1).all() and (route.cpu().numpy() == -1).all()           # (id 0: padding; hops share pc's memory: -1 too)
    assert (cells.cpu().numpy() == 0).all()
    # a graph switched off in the middle of an episode keeps its masks, but they miss what ignites from then on: no tree from those
    b.enable_spread_graph(False)
    assert rc(**hist) == _lib.SF_ESTATE and b"sf_enable_spread_graph" in L.sf_last_error()
    with pytest.raises(ValueError, match="spread graph"):
        b.influence(history=True)
    b.enable_spread_graph(True)
    assert rc(**hist) == _lib.SF_OK
    wide = _engine(5, 8200, 1)
    wcells = torch.zeros((1, 5, 8200), dtype=torch.int32, device="cuda")
    wpred = torch.full((5, 8200), -1, dtype=torch.int8, device="cuda")
    p, o, e = _lib.SfInfluenceParams(pred=wpred.data_ptr()), _lib.SfInfluenceOut(cells=wcells.data_ptr()), np.zeros(1, dtype=np.int32)
    assert wide._L.sf_influence(wide._h, C.byref(p), 1, e.ctypes.data_as(C.c_void_p), C.byref(o)) == _lib.SF_ENOTSUP
    for kwargs in (dict(pred=pred.float()), dict(pred=pred[:, :-1]), dict(pred=pred.cpu()), dict(pred=pred, points=pts[:, :, :2]),
                   dict(pred=pred, weights=wts.long()), dict(pred=pred, include=wts), dict(pred=pred, envs=[0], points=pts)):
        with pytest.raises(ValueError, match="influence"):
            b.influence(**kwargs)


# ---------------------------------------------------------------------------------------------- 7. the simulation classes
def test_fire_simulation_fire_influence_after_a_host_edit():
    from simfire_amd.config import Config
    from simfire_amd.enums import BurnStatus
    from simfire_amd.simulation import FireSimulation
    sim = FireSimulation(Config(os.path.join(CFG, "test_config_flat_simple.yml")))
    sim.enable_spread_graph(True)
    sim.record_arrival = True
    for _ in range(8):                                        # until the fire has spread a little: a few cells beside the ignition
        sim.run(1)
        if (np.asarray(sim.fire_map) != 0).sum() > 3:
            break
    eng = sim._engine
    got = sim.fire_influence()
    want = _want(io.history_codes(eng.spread_parents(0), eng.arrival(0)))
    assert got.dtype == np.int32 and got.shape == want["cells"].shape and np.array_equal(got, want["cells"]) and got.max() > 0
    m = np.asarray(sim.fire_map)
    H, W = m.shape
    ys, xs = np.nonzero(m == 1)
    free = [y for y in range(H) if (m[y] == 0).all()]
    assert len(ys) and free, m.tolist()
    y0 = min(free, key=lambda y: abs(y - int(ys.mean())))     # the untouched row nearest to the fire
    before = sim.fire_influence("forecast")
    sim.fire_map[y0, :] = int(BurnStatus.FIRELINE)            # a host edit: a line across the whole map beside the fire
    after = sim.fire_influence("forecast", inclusive=True)
    pred = _np(eng.travel(plane=False, pred=True, envs=[0]), eng)["pred"][0]
    assert (np.asarray(sim.fire_map)[y0] == 3).all() and (pred[y0] == -1).all()
    assert np.array_equal(after, _want(pred, None, None, True)["cells"]) and before.sum() > (after - 1).sum() >= 0
    both = sim.fire_influence("forecast", weights=_dev(np.full((H, W), 3, dtype=np.int32)), value=True)
    assert set(both) == {"cells", "value"} and np.array_equal(both["value"], 3 * both["cells"].astype(np.int64))
