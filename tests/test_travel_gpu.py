"""Fire travel time on the GPU (``sf_travel``).  The yardstick is ``tests/_travel_oracle.py`` - a float32 heap
Dijkstra - fed with the maps, the planes and the R tables (``sf_get_rtable_env``) fetched AFTER the call (a getter may convert the
current plane).  Every comparison is equality: ``minutes``, ``pred``, ``point_minutes``, ``reached``, ``last`` - the solution is
unique, so no bit may depend on how the kernel schedules its relaxations.  Run with ``pytest -m gpu``."""
import ctypes as C
import os

import numpy as np
import pytest

import _arrival_worlds as aw
import _reach_oracle as ro
import _reach_worlds as rw
import _travel_oracle as to
import _travel_worlds as tw

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tests", "golden", "configs")
BURNING, UNBURNED = ("BURNING",), ("UNBURNED",)
# the scenes of the widest shape the tests keep (the oracle takes half a second a scene there)
WIDE = ("random_1", "serpentine_h", "serpentine_v", "spiral", "fast_strip", "corner_gap_8", "border_gap_4", "source_on_a_tile_border", "both_per_env",
        "points_capped")


def _engine(kw, E, mode, R8=None, per_env=False):
    from simfire_amd.engine import FireEngine
    eng = FireEngine(n_envs=E, per_env_terrain=per_env, **kw)
    m = aw.mode_settings(mode)
    eng.set_fused(m["fused"])
    if m.get("tuning"):
        eng.set_tuning(**m["tuning"])
    if R8 is not None:
        eng.set_rtable(R8)
    return eng


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ask(eng, src, thr, conn, envs=None, passable=None, sources=None, points=None, **more):
    """(every output of ``travel`` as NumPy arrays, the maps fetched AFTER the call, the layout the call read).  ``passable``,
    ``sources``, ``points``: host arrays."""
    lay, kind = eng.cell_layout(), eng.last_launch_kind()
    r = eng.travel(src, thr, envs=envs, connectivity=conn or None, passable=_dev(passable), sources=_dev(sources), points=_dev(points),
                   plane=True, pred=True, reached=True, last=True, activations=True, **more)
    eng.sync()                                               # (a handle in async mode has only enqueued)
    assert (eng.cell_layout(), eng.last_launch_kind()) == (lay, kind)
    assert all(v.is_cuda for v in r.values())
    r = {k: v.cpu().numpy() for k, v in r.items()}
    return r, eng.fire_maps(), lay


def _same(eng, r, maps, envs, src, thr, conn, tag, passable=None, sources=None, points=None, max_minutes=0.0, tables=None):
    """Every output of every listed environment equals the oracle on its map and its table.  Returns the oracle's answers."""
    H, W = maps.shape[1:]
    n = len(envs)
    assert r["minutes"].shape == (n, H, W) and r["minutes"].dtype == np.float32 and r["pred"].dtype == np.int8 and r["pred"].shape == (n, H, W)
    assert r["reached"].dtype == np.int32 and r["last"].dtype == np.float32 and r["last"].shape == (n,)
    ps = float(eng.params.pixel_scale)
    conn = conn or (8 if eng.params.diagonal_spread else 4)
    wants, cache = [], {}
    for i, e in enumerate(envs):
        p = None if passable is None else (passable if passable.ndim == 2 else passable[e])
        s = None if sources is None else (sources if sources.ndim == 2 else sources[e])
        if tables is None and e not in cache:
            cache[e] = eng.get_rtable(e)
        R8 = tables[e] if tables is not None else cache[e]
        want = to.answer(maps[e], R8, ps, ro.mask_of(src) if src else 0, ro.mask_of(thr), conn, p, s, None if points is None else points[i], max_minutes)
        bad = np.argwhere(r["minutes"][i] != want["minutes"])
        assert not len(bad), (tag, i, e, len(bad), bad[:5].tolist(), [(float(r["minutes"][i][tuple(b)]), float(want["minutes"][tuple(b)])) for b in bad[:5]])
        bad = np.argwhere(r["pred"][i] != want["pred"])
        assert not len(bad), (tag, i, e, len(bad), bad[:5].tolist(), [(int(r["pred"][i][tuple(b)]), int(want["pred"][tuple(b)])) for b in bad[:5]])
        assert int(r["reached"][i]) == want["reached"], (tag, i, e, int(r["reached"][i]), want["reached"])
        assert r["last"][i] == want["last"], (tag, i, e, float(r["last"][i]), float(want["last"]))
        if points is not None:
            assert r["point_minutes"][i].tolist() == want["point_minutes"].tolist(), (tag, i, e, r["point_minutes"][i].tolist(), want["point_minutes"].tolist())
        wants.append(want)
    return wants


# ---------------------------------------------------------------------------------------------- 1. the hand-made scenes
@pytest.mark.parametrize("shape", tw.SCENE_SHAPES, ids=["%dx%d" % s for s in tw.SCENE_SHAPES])
@pytest.mark.parametrize("mode", ["fused0", "run"])
def test_scenes(shape, mode):
    """Every scene of ``_travel_worlds.scenes`` in an environment of its own, each with its own R table (a terrain table per
    environment), through ``load_fire_map``.  ``fused0``: read in the row-major layout as loaded - equality with the oracle and what
    the scene claims.  ``run``: one update first, so that the cells lie in the blocked plane - equality with the oracle on the maps
    as they are then."""
    H, W = shape
    sc = tw.scenes(H, W)
    if W > 1000:
        sc = [s for s in sc if s["name"] in WIDE]
    E = len(sc)
    b = _engine(tw.engine_kwargs(H, W), E, mode, per_env=True)
    for e, s in enumerate(sc):
        b.set_rtable(s["R8"], env=e)
    b.reset(np.full((E, 2), 0, dtype=np.int32))
    for e, s in enumerate(sc):
        b.load_fire_map(e, s["map"])
    if mode == "run":
        b.step(1)
    per_pas, per_src = rw.per_env_passable(E, H, W), tw.per_env_sources(E, H, W)
    tables = [b.get_rtable(e) for e in range(E)]
    lays, acts = [], []
    for e, s in enumerate(sc):
        assert (tables[e] == s["R8"]).all()
        pas = per_pas if isinstance(s["passable"], str) else s["passable"]
        src = per_src if isinstance(s["sources"], str) else s["sources"]
        pts = s["points"][None]
        r, maps, lay = _ask(b, s["source"], s["through"], s["conn"], envs=[e], passable=pas, sources=src, points=pts, max_minutes=s["max_minutes"] or None)
        _same(b, r, maps, [e], s["source"], s["through"], s["conn"], (shape, mode, s["name"]), passable=pas, sources=src, points=pts,
              max_minutes=s["max_minutes"], tables=tables)
        if mode == "fused0":
            assert (maps[e] == s["map"]).all()
            if s["claim"] is not None:
                s["claim"](dict(minutes=r["minutes"][0], pred=r["pred"][0], point_minutes=r["point_minutes"][0], reached=int(r["reached"][0]),
                                last=r["last"][0]))
        lays.append(lay)
        acts.append((s["name"], int(r["activations"][0])))
    print("tile activations:", shape, mode, acts)
    if mode == "run" and H * W > 81:
        assert set(lays) == {1}, lays
    if mode == "fused0":
        assert set(lays) == {0}, lays
    if mode == "fused0" and shape == (40, 130):
        tiles = 2 * 5
        assert dict(acts)["serpentine_h"] > 3 * tiles and dict(acts)["no_source"] == 0      # tiles are activated again and again


@pytest.mark.parametrize("mode", ["fused0", "run"])
def test_max_minutes(mode):
    """A straight corridor of 30 cells under a uniform table: capped just below, inside and exactly at its travel time."""
    H, W = 9, 40
    R8 = np.full((8, H, W), 7.0)
    b = _engine(tw.engine_kwargs(H, W), 2, mode, R8)
    b.reset(np.zeros((2, 2), dtype=np.int32))
    b.load_fire_map(1, tw.corridor(H, W, 30))
    if mode == "run":
        b.step(1)
    w = np.float32(30.0 / 7.0)
    end = float(tw.fold(w, 30))
    for M, n in ((float(np.nextafter(np.float32(end), np.float32(0))), 29), (end, 30), (float(tw.fold(w, 17)) + 0.5, 17), (0.0, 30), (1e30, 30)):
        pts = np.array([[[31, 2, 1], [1 + n, 2, 1], [2 + n, 1, 1]]], dtype=np.int32)
        r, maps, _ = _ask(b, BURNING, UNBURNED, 4, envs=[1], points=pts, max_minutes=M or None)
        _same(b, r, maps, [1], BURNING, UNBURNED, 4, (mode, M), points=pts, max_minutes=M)
        if mode == "run":
            continue                                          # (the update may have moved the fire: equality with the oracle only)
        assert int(r["reached"][0]) == n and r["last"][0] == tw.fold(w, n)
        if 0 < M < 1e30:
            assert r["minutes"][0].max() == np.float32(M) and r["point_minutes"][0][2] == np.float32(M)
        assert r["point_minutes"][0][1] == tw.fold(w, n) and (r["pred"][0][2, 2:2 + n] == 4).all() and (r["pred"][0][2, 2 + n:] == -1).all()


# ---------------------------------------------------------------------------------------------- 2. lists, chunks, many environments
@pytest.mark.parametrize("mode", ["run", "fused0"])
def test_lists_and_chunks(mode):
    """Lists in any order with repeats; a call without a minutes plane works in the scratch, chunk by chunk when the budget holds one
    environment only - bit for bit what the default call gives; the scratch grows and never shrinks."""
    import torch
    kw, R8, E, inits = aw.make_world("24x40")
    b = _engine(kw, E, mode, R8)
    H, W = kw["shape"]
    need = b.travel_scratch_bytes()
    assert need == (4 * H * W + 255) // 256 * 256
    b.reset(inits)
    b.step(7)
    b.apply_mitigation(rw.line_rows(1, E, H, W, inits))
    b.step(2)
    pts = np.random.default_rng(5303).integers(0, 24, size=(E, 5, 3)).astype(np.int32)
    mem0 = b.memory_bytes()
    full = b.travel(points=_dev(pts), pred=True, reached=True, last=True)            # the working array is the minutes plane: no scratch
    assert b.memory_bytes() == mem0
    one = b.travel(points=_dev(pts), plane=False, pred=True, reached=True, last=True, scratch_bytes=need)      # E chunks of one
    assert b.memory_bytes() - mem0 == need
    every = b.travel(points=_dev(pts), plane=False, pred=True, reached=True, last=True)
    assert b.memory_bytes() - mem0 == E * need
    b.travel(plane=False, reached=True, scratch_bytes=need)
    assert b.memory_bytes() - mem0 == E * need
    for name in ("pred", "point_minutes", "reached", "last"):
        assert torch.equal(one[name], full[name]) and torch.equal(every[name], full[name]), name
    assert "minutes" not in one and int(full["reached"].sum()) > 0
    for envs in ([e for e in reversed(range(E))], [0, E - 1, 0, 0, 2, E - 1, 2], [1, 3], [2]):
        src, thr = tw.MASK_PAIRS[len(envs) % 4]
        p = pts[:len(envs)] if len(envs) <= E else None
        base, maps, _ = _ask(b, src, thr, 0, envs=envs, points=p)
        _same(b, base, maps, envs, src, thr, 0, (mode, envs), points=p)
        got = b.travel(src, thr, envs=envs, points=_dev(p), plane=False, pred=True, reached=True, last=True, scratch_bytes=2 * need + 7)
        for name in got:
            assert (got[name].cpu().numpy() == base[name]).all(), (mode, envs, name)
    with pytest.raises(ValueError, match="scratch_bytes"):
        b.travel(scratch_bytes=need - 1)
    assert b.travel(envs=[])["minutes"].shape == (0, H, W)


def test_more_environments_than_cus():
    import torch
    n = torch.cuda.get_device_properties(0).multi_processor_count + 8
    rng = np.random.default_rng(5305)
    H = W = 9
    b = _engine(tw.engine_kwargs(H, W), n, "fused0", tw.random_rates(rng, H, W))
    b.reset(np.stack([rng.integers(0, W, size=n), rng.integers(0, H, size=n)], axis=1).astype(np.int32))
    b.step(2)
    r, maps, _ = _ask(b, BURNING, UNBURNED, 8)
    wants = _same(b, r, maps, range(n), BURNING, UNBURNED, 8, "many")
    assert len({w["reached"] for w in wants}) > 4


# ---------------------------------------------------------------------------------------------- 3. the table the handle holds now
def _config_24x40():
    import yaml
    from simfire_amd.config import Config
    y = yaml.safe_load(open(os.path.join(CFG, "functional_config.yml")))
    y["area"]["screen_size"] = [24, 40]
    y["terrain"]["topography"]["functional"]["function"] = "flat"
    y["simulation"]["headless"] = True
    return Config(config_dict=y)


def test_set_wind_changes_the_plane():
    from simfire_amd.simulation import BatchedFireSimulation
    bat = BatchedFireSimulation(_config_24x40(), 3)
    bat.run(3, return_maps=False)
    eng = bat._engine
    before, maps, _ = _ask(eng, BURNING, UNBURNED, 0)
    tables = [eng.get_rtable(e) for e in range(3)]
    _same(eng, before, maps, range(3), BURNING, UNBURNED, 0, "before", tables=tables)
    bat.set_wind(25.0, 200.0)
    after, maps, _ = _ask(eng, BURNING, UNBURNED, 0)
    tables2 = [eng.get_rtable(e) for e in range(3)]
    assert not (tables2[0] == tables[0]).all()
    _same(eng, after, maps, range(3), BURNING, UNBURNED, 0, "after", tables=tables2)
    assert not (after["minutes"] == before["minutes"]).all()
    up = bat.time_to_fire(envs=[1], unit="updates", device=False, last=True)
    rate = np.float32(eng.params.update_rate)
    assert (up["minutes"][0] == np.where(after["minutes"][1] < 0, after["minutes"][1], after["minutes"][1] / rate)).all()
    assert up["last"][0] == after["last"][1] / rate


def test_a_handle_fed_by_set_rtable_alone():
    """No layers: the R table is all the call needs.  Before the table, and before the reset, SF_ESTATE."""
    from simfire_amd import _lib
    from simfire_amd.engine import FireEngine
    H, W = 33, 17
    rng = np.random.default_rng(5306)
    b = FireEngine(n_envs=2, **tw.engine_kwargs(H, W, diag=False))
    with pytest.raises(_lib.SimfireHipError, match="sf_travel"):
        b.travel()
    R8 = tw.random_rates(rng, H, W)
    b.set_rtable(R8)
    with pytest.raises(_lib.SimfireHipError, match="sf_reset"):
        b.travel()
    b.reset(np.array([[3, 4], [10, 30]], dtype=np.int32))
    r, maps, _ = _ask(b, BURNING, UNBURNED, 0)                # (0: the handle's diagonal_spread - off)
    _same(b, r, maps, range(2), BURNING, UNBURNED, 4, "rtable only")
    r8, maps, _ = _ask(b, BURNING, UNBURNED, 8)
    _same(b, r8, maps, range(2), BURNING, UNBURNED, 8, "rtable only, 8")
    assert not (r8["minutes"] == r["minutes"]).all()


# ---------------------------------------------------------------------------------------------- 4. reads only, async
@pytest.mark.parametrize("mode", ["run", "fused0"])
def test_reads_only(mode):
    """The same rollout on two handles, arrival recording and a value plane on, one of them with travel calls between its step calls:
    maps, burn amounts, status rows, elapsed times, arrival planes, damage and the ``fire_map_delta`` sequence are the same."""
    import torch
    kw, R8, E, inits = aw.make_world("24x40")
    H, W = kw["shape"]
    a, b = _engine(kw, E, mode, R8), _engine(kw, E, mode, R8)
    rng = np.random.default_rng(5304)
    vals = rng.integers(-1000, 1000, size=(H, W)).astype(np.int32)
    pts = torch.from_numpy(rng.integers(0, 24, size=(E, 7, 3)).astype(np.int32)).cuda()
    pas = torch.from_numpy((rng.random((H, W)) < 0.9).astype(np.uint8)).cuda()
    srcs = torch.from_numpy((rng.random((E, H, W)) < 0.01).astype(np.uint8)).cuda()
    deltas = {id(a): [], id(b): []}
    for h in (a, b):
        h.reset(inits)
        h.enable_arrival(True)
        h.values_set(vals)
        for i, n in enumerate((1, 2, 3, 5)):
            h.step(n)
            if h is b:
                src, thr = tw.MASK_PAIRS[i]
                for call in (lambda: h.travel(src, thr, pred=True, reached=True, last=True),
                             lambda: h.travel(src, thr, connectivity=4, points=pts, plane=False, passable=pas, sources=srcs),
                             lambda: h.travel(None, thr, connectivity=8, envs=[E - 1, 0], sources=srcs, plane=False, pred=True,
                                              scratch_bytes=h.travel_scratch_bytes(), max_minutes=3.0)):
                    lay, kind = h.cell_layout(), h.last_launch_kind()
                    call()
                    assert (h.cell_layout(), h.last_launch_kind()) == (lay, kind), (mode, i)
                assert lay == (1 if mode == "run" else 0)
            d = h.fire_map_delta(0)
            deltas[id(h)].append(None if d is None else sorted(zip(d[0].tolist(), d[1].tolist())))
    assert deltas[id(a)] == deltas[id(b)] and any(deltas[id(a)])
    sa, ea = a.status()
    sb, eb = b.status()
    assert (sa == sb).all() and (ea == eb).all()
    assert (a.damage() == b.damage()).all()
    assert (a.fire_maps() == b.fire_maps()).all()
    for e in range(E):
        assert (a.arrival(e) == b.arrival(e)).all() and (a.burn(e) == b.burn(e)).all(), (mode, e)


def test_async_mode():
    """In async mode the calls only enqueue: steps and travel calls queued behind each other, one wait, the results those of the
    same calls made one by one."""
    kw, R8, E, inits = aw.make_world("24x40")
    a, b = _engine(kw, E, "run", R8), _engine(kw, E, "run", R8)
    b.set_async(True)
    got = {id(a): [], id(b): []}
    for h in (a, b):
        h.reset(inits)
        for n in (3, 4):
            h.step(n)
            got[id(h)].append(h.travel(pred=True, reached=True, last=True))
            got[id(h)].append(h.travel(plane=False, reached=True, max_minutes=5.0))
    b.sync()
    for x, y in zip(got[id(a)], got[id(b)]):
        for name in x:
            assert (x[name].cpu().numpy() == y[name].cpu().numpy()).all(), name
    r = {k: v.cpu().numpy() for k, v in got[id(b)][2].items()}
    _same(b, r, b.fire_maps(), range(E), BURNING, UNBURNED, 0, "async")


# ---------------------------------------------------------------------------------------------- 5. errors
def test_errors_through_the_raw_call():
    import torch
    from simfire_amd import _lib
    kw, R8, E, inits = aw.make_world("24x40")
    b = _engine(kw, E, "run", R8)
    H, W = kw["shape"]
    L, h = b._L, b._h
    need = b.travel_scratch_bytes()
    reached = torch.full((E,), -7, dtype=torch.int32, device="cuda")
    pm = torch.full((E, 3), -7.0, dtype=torch.float32, device="cuda")
    plane = torch.full((E, H, W), -7.0, dtype=torch.float32, device="cuda")
    pts = torch.zeros((E, 3, 3), dtype=torch.int32, device="cuda")
    sg = torch.ones((H, W), dtype=torch.uint8, device="cuda")
    all_envs = np.arange(E, dtype=np.int32)

    def rc(n=E, envs=all_envs, reserved=(0, 0), outs=None, **fields):
        p = _lib.SfTravelParams(**dict(dict(source_mask=2, through_mask=1), **fields))
        p.reserved[0], p.reserved[1] = reserved
        o = _lib.SfTravelOut(**(dict(reached=reached.data_ptr()) if outs is None else outs))
        e = None if envs is None else np.ascontiguousarray(envs, dtype=np.int32)
        return L.sf_travel(h, C.byref(p), n, None if e is None else e.ctypes.data_as(C.c_void_p), C.byref(o))

    assert rc() == _lib.SF_ESTATE                             # before reset
    assert b"sf_reset" in L.sf_last_error()
    b.reset(inits)
    b.step(3)
    withpts = dict(k=3, points=pts.data_ptr())
    bad = [dict(source_mask=0), dict(source_mask=-1), dict(source_mask=64), dict(through_mask=0), dict(through_mask=-1), dict(through_mask=64),
           dict(source_mask=64, sources=sg.data_ptr()), dict(connectivity=6), dict(connectivity=-1), dict(connectivity=1),
           dict(k=-1), dict(k=257, points=pts.data_ptr(), outs=dict(point_minutes=pm.data_ptr())), dict(k=3, outs=dict(point_minutes=pm.data_ptr())),
           dict(points=pts.data_ptr()), dict(outs=dict(reached=reached.data_ptr(), point_minutes=pm.data_ptr())), dict(**withpts),
           dict(max_minutes=-1.0), dict(max_minutes=float("nan")), dict(reserved=(1, 0)), dict(reserved=(0, 1)), dict(outs=dict()),
           dict(outs=dict(reached=reached.data_ptr() + 2)), dict(outs=dict(minutes=plane.data_ptr() + 2)), dict(outs=dict(last=pm.data_ptr() + 1)),
           dict(outs=dict(activations=reached.data_ptr() + 1)), dict(outs=dict(point_minutes=pm.data_ptr() + 2), **withpts),
           dict(k=3, points=pts.data_ptr() + 2, outs=dict(point_minutes=pm.data_ptr())),
           dict(envs=[0, E]), dict(envs=[-1, 0], n=2), dict(scratch_bytes=need - 1), dict(scratch_bytes=1), dict(scratch_bytes=-1),
           dict(n=-1), dict(envs=None)]
    for kwargs in bad:
        kwargs = dict(kwargs)
        if "envs" in kwargs and kwargs["envs"] is not None and "n" not in kwargs:
            kwargs["n"] = len(kwargs["envs"])
        assert rc(**kwargs) == _lib.SF_EINVAL, kwargs
        assert b"sf_travel" in L.sf_last_error(), kwargs
    b.sync()
    assert (reached == -7).all() and (pm == -7).all() and (plane == -7).all()        # nothing was enqueued
    assert rc(outs=dict(point_minutes=pm.data_ptr()), **withpts) == _lib.SF_OK        # the call after an error works
    assert rc(n=0) == _lib.SF_OK
    assert rc(source_mask=0, sources=sg.data_ptr()) == _lib.SF_OK
    b.sync()
    assert (pm.cpu().numpy() == -1).all() and (reached.cpu().numpy() == 0).all()      # (id 0: padding; every cell a source: none reached)
    r, maps, _ = _ask(b, BURNING, UNBURNED, 0)
    _same(b, r, maps, range(E), BURNING, UNBURNED, 0, "after the errors")
    for kwargs in (dict(points=pts[:, :, :2]), dict(points=torch.zeros((E, 257, 3), dtype=torch.int32, device="cuda")), dict(points=pts.cpu()),
                   dict(passable=torch.ones((H, W), dtype=torch.float32, device="cuda")), dict(sources=torch.ones((H, W + 1), dtype=torch.uint8, device="cuda"))):
        with pytest.raises(ValueError, match="travel"):
            b.travel(**kwargs)


# ---------------------------------------------------------------------------------------------- 6. BatchedFireEnv
@pytest.mark.parametrize("max_ticks", [0, 4])
def test_batched_fire_env_time_to_fire(max_ticks):
    """``info["minutes_to_fire"]`` of every tick is what a direct call gives for the device positions behind that tick - through an
    auto-reset tick too; without the option ``info`` has the old keys only."""
    import torch
    import simfire_amd
    from simfire_amd.simulation import BatchedFireSimulation
    cfg = _config_24x40()
    H, W = cfg.area.screen_size
    E, K = 3, 4
    ign = np.array([(10, 10), (W - 5, 7), (3, H - 4)], dtype=np.int32)
    starts = np.array([(W - 1, 16), (W - 2, 11), (20, 12), (5, 5)], dtype=np.int32)
    option = dict(through=("UNBURNED", "FIRELINE"), max_minutes=500.0)
    sim = BatchedFireSimulation(cfg, E, ignitions=ign)
    env = simfire_amd.BatchedFireEnv(sim, K, starts, n_updates=1, max_ticks=max_ticks, time_to_fire=option)
    plain = simfire_amd.BatchedFireEnv(BatchedFireSimulation(cfg, E, ignitions=ign), K, starts, n_updates=1, max_ticks=max_ticks)
    env.reset()
    plain.reset()
    rng = np.random.default_rng(5307)
    restarted, finite = False, 0
    for t in range(7):
        actions = torch.from_numpy(rng.integers(0, 20, size=(E, K)).astype(np.int32)).cuda()
        obs, reward, done, info = env.step(actions)
        obs_p, reward_p, done_p, info_p = plain.step(actions)
        assert set(info) == set(info_p) | {"minutes_to_fire"} and torch.equal(obs, obs_p) and torch.equal(reward, reward_p)
        got = info["minutes_to_fire"]
        assert got.dtype == torch.float32 and got.shape == (E, K) and got.is_cuda
        direct = sim.time_to_fire(plane=False, agents=True, **option)["point_minutes"]
        assert torch.equal(got, direct), (t, got.tolist(), direct.tolist())
        pos = env.positions().cpu().numpy()
        maps = sim._engine.fire_maps()
        for e in range(E):
            want = to.answer(maps[e], sim._engine.get_rtable(e), float(sim._engine.params.pixel_scale), 2, 1 | 8,
                             8 if sim._engine.params.diagonal_spread else 4, pts=pos[e], max_minutes=500.0)
            assert got[e].cpu().numpy().tolist() == want["point_minutes"].tolist(), (t, e)
        finite += int((got > 0).sum())
        if max_ticks and (t + 1) % max_ticks == 0:
            assert bool(done.all().item())
            restarted = True
            assert (pos[:, :, :2] == starts[None]).all()
    assert restarted == bool(max_ticks) and finite > 0
    with pytest.raises(ValueError, match="time_to_fire"):
        simfire_amd.BatchedFireEnv(sim, K, starts, time_to_fire=dict(radius=3))


# ---------------------------------------------------------------------------------------------- 7. the simulation classes
def test_fire_simulation_time_to_fire_after_a_host_edit():
    from simfire_amd.config import Config
    from simfire_amd.enums import BurnStatus
    from simfire_amd.simulation import FireSimulation
    sim = FireSimulation(Config(os.path.join(CFG, "test_config_flat_simple.yml")))
    sim.run(2)
    eng = sim._engine
    ps, conn = float(eng.params.pixel_scale), 8 if eng.params.diagonal_spread else 4
    T = sim.time_to_fire()
    m = np.asarray(sim.fire_map)
    H, W = m.shape
    want = to.answer(m, eng.get_rtable(0), ps, 2, 1, conn)
    assert T.dtype == np.float32 and T.shape == m.shape and (T == want["minutes"]).all() and T.max() > 0
    ys, xs = np.nonzero(m == 1)
    y0 = ys.max() + 2 if ys.max() + 3 < H else ys.min() - 2
    sim.fire_map[y0, :] = int(BurnStatus.FIRELINE)            # a host edit: a line across the whole map beside the fire
    T2 = sim.time_to_fire()
    m2 = np.asarray(sim.fire_map)
    assert (m2[y0] == 3).all() and (T2 == to.answer(m2, eng.get_rtable(0), ps, 2, 1, conn)["minutes"]).all()
    beyond = T2[y0 + 1:] if y0 > ys.max() else T2[:y0]
    assert (T2[y0] == -1).all() and beyond.size and not np.isfinite(beyond[beyond >= 0]).any() and (T2 != T).any()
    through = sim.time_to_fire(through=("UNBURNED", "FIRELINE"), max_minutes=float(T.max()) / 2, unit="updates")
    w2 = to.answer(m2, eng.get_rtable(0), ps, 2, 1 | 8, conn, max_minutes=float(T.max()) / 2)["minutes"]
    assert (through == np.where(w2 < 0, w2, w2 / np.float32(eng.params.update_rate))).all()


@pytest.mark.parametrize("mode", ["run", "fused0"])
def test_uniform_world_against_the_device_arrival(mode):
    """Flat, windless, uniform, q = pixel_scale / (R * update_rate) = 4.29: the device's own arrival plane shows h * (floor(q) + 1)
    updates for a cell h Chebyshev cells from the ignition, the travel plane - asked for right after the reset - the h-fold float32 sum
    of w: the forecast is the automaton without the rounding up to whole updates."""
    H, W, R, md = 17, 19, 7.0, 8
    b = _engine(tw.engine_kwargs(H, W, md=md), 1, mode, np.full((8, H, W), R))
    y0, x0 = 8, 9
    b.reset(np.array([[x0, y0]], dtype=np.int32))
    b.enable_arrival(True)
    r, maps, _ = _ask(b, BURNING, UNBURNED, 8)
    h = np.maximum(np.abs(np.arange(H)[:, None] - y0), np.abs(np.arange(W)[None, :] - x0))
    w = np.float32(tw.PIXEL_SCALE / R)
    folds = np.array([tw.fold(w, n) for n in range(max(H, W))], dtype=np.float32)
    assert (r["minutes"][0] == folds[h]).all() and int(r["reached"][0]) == H * W - 1 and r["last"][0] == folds[h.max()]
    b.step(5 * 9 + 2)
    assert (b.arrival(0) == h * 5).all()
