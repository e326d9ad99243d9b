"""Reach of the fire on the GPU (``sf_reach``).  The yardstick is ``tests/_reach_oracle.py`` - plain repeated
dilation - fed with the maps the older getters return.  ``reach`` is always called FIRST and the maps are fetched afterwards (a getter
may convert the current plane); every comparison is equality.  Run with ``pytest -m gpu``."""
import ctypes as C
import os

import numpy as np
import pytest

import _arrival_worlds as aw
import _reach_oracle as ro
import _reach_worlds as rw

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tests", "golden", "configs")
BURNING, UNBURNED = ("BURNING",), ("UNBURNED",)


def _engine(kw, E, R8, mode):
    from simfire_amd.engine import FireEngine
    eng = FireEngine(n_envs=E, **kw)
    m = aw.mode_settings(mode)
    eng.set_fused(m["fused"])
    if m.get("tuning"):
        eng.set_tuning(**m["tuning"])
    eng.set_rtable(R8)
    return eng


def _world(case, mode, n_envs=None):
    kw, R8, E, inits = aw.make_world(case, n_envs)
    return _engine(kw, E, R8, mode), E, inits, kw


def _conn(kw, conn):
    return conn if conn else (8 if kw["diagonal_spread"] else 4)


def _ask(eng, src, thr, conn, envs=None, passable=None, points=None, value=False, **more):
    """(the outputs of ``reach`` as NumPy arrays, the maps fetched AFTER the call, the layout the call read)."""
    lay, kind = eng.cell_layout(), eng.last_launch_kind()
    r = eng.reach(src, thr, envs=envs, connectivity=conn or None, passable=passable, points=points, count=True, value=value, mask=True,
                  seeds=True, rounds=True, **more)
    assert (eng.cell_layout(), eng.last_launch_kind()) == (lay, kind)
    r = {k: v.cpu().numpy() for k, v in r.items()}
    return r, eng.fire_maps(), lay


def _same(r, maps, envs, src, thr, conn, tag, passable=None, points=None, values=None):
    """Every output of every listed environment equals the oracle on its map.  Returns the oracle's masks."""
    H, W = maps.shape[1:]
    n = len(envs)
    assert r["mask"].shape == (n, H, W) and r["mask"].dtype == np.uint8 and r["count"].shape == (n,) and r["count"].dtype == np.int32
    wants = []
    for i, e in enumerate(envs):
        p = None if passable is None else (passable if passable.ndim == 2 else passable[e])
        want = ro.reach(maps[e], ro.mask_of(src), ro.mask_of(thr), conn, p)
        bad = np.argwhere(r["mask"][i] != want.astype(np.uint8))
        assert not len(bad), (tag, i, e, len(bad), bad[:5].tolist(), int(r["count"][i]), ro.count(want))
        assert int(r["count"][i]) == ro.count(want), (tag, i, e)
        assert int(r["seeds"][i]) == ro.seeds(maps[e], ro.mask_of(src)), (tag, i, e)
        assert int(r["rounds"][i]) > 0, (tag, i, e, int(r["rounds"][i]))
        if values is not None:
            assert r["value"].dtype == np.int64 and int(r["value"][i]) == ro.value(want, values if values.ndim == 2 else values[e]), (tag, i, e)
        if points is not None:
            assert r["point_in"].dtype == np.int32 and r["point_in"][i].tolist() == ro.point_in(want, points[i]).tolist(), (tag, i, e)
        wants.append(want)
    return wants


# ---------------------------------------------------------------------------------------------- 1. through an episode
@pytest.mark.parametrize("case,mode", rw.PAIRS, ids=["%s-%s" % p for p in rw.PAIRS])
def test_reach_through_an_episode(case, mode):
    """Behind calls of 1, 2, 3, 5, 7 and 11 updates, the mask pairs and connectivities of ``_reach_worlds.queries`` in turn, control
    lines drawn between the calls of every second mode: every output of every environment equals the oracle on the maps; the ``run*``
    modes were read in the blocked layout, ``fused0`` in the row-major one."""
    b, E, inits, kw = _world(case, mode)
    H, W = kw["shape"]
    lays, sizes = [], []

    def on_query(i, n, src, thr, conn):
        r, maps, lay = _ask(b, src, thr, conn)
        wants = _same(r, maps, range(E), src, thr, _conn(kw, conn), (case, mode, i, n, src, thr, conn))
        lays.append(lay)
        sizes.append(sum(int(w.sum()) for w in wants))
    rw.run_episode(case, mode, b, inits, on_query, H, W)
    print("layouts behind the calls:", case, mode, lays, "cells reached:", sizes)
    assert max(sizes) > 0
    if mode.startswith("run"):
        assert lays == [1] * len(rw.CALLS), lays
    if mode == "fused0":
        assert lays == [0] * len(rw.CALLS), lays


# ---------------------------------------------------------------------------------------------- 2. the hand-made scenes
@pytest.mark.parametrize("shape", rw.SCENE_SHAPES, ids=["%dx%d" % s for s in rw.SCENE_SHAPES])
@pytest.mark.parametrize("mode", ["fused0", "run"])
def test_scenes(shape, mode):
    """Every scene of ``_reach_worlds.scenes`` in an environment of its own through ``load_fire_map``: equality with the oracle and
    the count the scene claims, read in the row-major layout; then one update (a ``run`` handle keeps the cells in its blocked plane
    behind it) and every scene again against the oracle on the maps as they are then."""
    import torch
    H, W = shape
    sc = rw.scenes(H, W)
    E = len(sc)
    kw, R8 = rw.make_scene_world(H, W, True)
    b = _engine(kw, E, R8, mode)
    b.reset(np.full((E, 2), 0, dtype=np.int32))
    for e, s in enumerate(sc):
        b.load_fire_map(e, s["map"])
    per_env = rw.per_env_passable(E, H, W)
    per_env_dev = torch.from_numpy(per_env).cuda()
    for turn in range(2):
        lays = []
        for e, s in enumerate(sc):
            pas = per_env if isinstance(s["passable"], str) else s["passable"]
            pas_dev = None if pas is None else (per_env_dev if pas.ndim == 3 else torch.from_numpy(pas).cuda())
            pts = None if s["points"] is None else s["points"][None]
            r, maps, lay = _ask(b, s["source"], s["through"], s["conn"], envs=[e], passable=pas_dev,
                                points=None if pts is None else torch.from_numpy(pts).cuda())
            _same(r, maps, [e], s["source"], s["through"], s["conn"], (shape, mode, turn, s["name"]), passable=pas, points=pts)
            if turn == 0:
                assert (maps[e] == s["map"]).all()
                if s["expect"] is not None:
                    assert int(r["count"][0]) == s["expect"], (shape, mode, s["name"])
            lays.append(lay)
        if turn == 0:
            b.step(1)
        elif mode == "run" and H * W > 81:
            assert set(lays) == {1}, lays
        elif mode == "fused0":
            assert set(lays) == {0}, lays


@pytest.mark.parametrize("mode", ["fused0", "run"])
def test_max_rounds_on_the_long_serpentine(mode):
    """``max_rounds = 1`` on a corridor of thousands of cells: either the fill was done (rounds > 0, equality), or rounds < 0, the mask
    is a subset of the oracle's that holds every open neighbour of a seed, count is its size, and the same call without the bound is
    then equal with rounds > 0."""
    H, W = 40, 130
    s = next(s for s in rw.scenes(H, W) if s["name"] == "serpentine_h_4")
    kw, R8 = rw.make_scene_world(H, W, True)
    b = _engine(kw, 3, R8, mode)
    b.reset(np.zeros((3, 2), dtype=np.int32))
    b.load_fire_map(1, s["map"])
    if mode == "run":
        b.step(1)
    r, maps, _ = _ask(b, BURNING, UNBURNED, 4, envs=[1], max_rounds=1)
    want = ro.reach(maps[1], 2, 1, 4)
    rounds = int(r["rounds"][0])
    assert rounds in (1, -1) and want.sum() > 2000
    if rounds > 0:
        assert (r["mask"][0] == want).all() and int(r["count"][0]) == want.sum()
    else:
        got = r["mask"][0].astype(bool)
        assert (got <= want).all() and (ro.first_round(maps[1], 2, 1, 4) <= got).all() and int(r["count"][0]) == got.sum() < want.sum()
        assert int(r["seeds"][0]) == ro.seeds(maps[1], 2)
    r, maps, _ = _ask(b, BURNING, UNBURNED, 4, envs=[1])
    _same(r, maps, [1], BURNING, UNBURNED, 4, (mode, "to the fixed point"))
    print("rounds with max_rounds = 1:", rounds, "to the fixed point:", int(r["rounds"][0]))
    r5, _, _ = _ask(b, BURNING, UNBURNED, 4, envs=[1], max_rounds=int(r["rounds"][0]))
    assert int(r5["rounds"][0]) == int(r["rounds"][0]) and (r5["mask"] == r["mask"]).all()      # the bound met exactly: the fixed point, said so


@pytest.mark.parametrize("mode", ["fused0", "run"])
def test_more_bands_than_threads(mode):
    """977 x 1030: 62 band rows (the last with one row) x 17 words (the last with 6 cells) = 1054 bands - the kernel that walks the
    bands in passes over the scratch planes, its second pass partly empty.  Random maps with an empty strip (rounds) and a wall."""
    import torch
    H, W = 977, 1030
    kw, R8 = rw.make_scene_world(H, W, True)
    b = _engine(kw, 2, R8, mode)
    assert b.reach_scratch_bytes() == (1054 * (16 * 16 + 20) + 255) // 256 * 256
    b.reset(np.zeros((2, 2), dtype=np.int32))
    rng = np.random.default_rng(5106)
    vals = rng.integers(-1000, 1000, size=(H, W)).astype(np.int32)
    b.enable_arrival(True)
    b.values_set(vals)
    for e in range(2):
        u = rng.random((H, W))
        m = np.where(u < 0.2, 3, np.where(u < 0.22, 1, np.where(u < 0.26, 2, 0))).astype(np.uint8)
        m[:, 40:100] = 0                                      # a strip the fill has to cross (the oracle: a cell per dilation)
        m[:, 700] = 3 + e                                     # a wall: what lies beyond is reached from its own seeds only
        b.load_fire_map(e, m)
    if mode == "run":
        b.step(1)
    pts = np.stack([rng.integers(-2, W + 2, size=(2, 40)), rng.integers(-2, H + 2, size=(2, 40)), rng.integers(0, 3, size=(2, 40))], axis=-1).astype(np.int32)
    for src, thr, conn in ((BURNING, UNBURNED, 4), (BURNING, UNBURNED, 8)):
        r, maps, lay = _ask(b, src, thr, conn, points=torch.from_numpy(pts).cuda(), value=True)
        _same(r, maps, range(2), src, thr, conn, (mode, conn), points=pts, values=vals)
        assert lay == (1 if mode == "run" else 0) and r["rounds"].min() > 1 and 0 < r["count"].min() and (r["count"] < (maps == 0).sum(axis=(1, 2))).all()
    one = b.reach(count=True, mask=True, rounds=True, scratch_bytes=b.reach_scratch_bytes())
    assert (one["mask"].cpu().numpy() == r["mask"]).all() and (one["rounds"].cpu().numpy() == r["rounds"]).all()


# ---------------------------------------------------------------------------------------------- 3. values and points
@pytest.mark.parametrize("mode,per_env", [("run", False), ("fused0", True), ("run", True)])
def test_value_and_points(mode, per_env):
    import torch
    b, E, inits, kw = _world("24x40", mode)
    H, W = kw["shape"]
    rng = np.random.default_rng(5101)
    vals = rng.integers(-(1 << 24), (1 << 24) + 1, size=(E, H, W) if per_env else (H, W)).astype(np.int32)
    vals.flat[0], vals.flat[-1] = -(1 << 24), 1 << 24
    b.reset(inits)
    b.enable_arrival(True)
    b.values_set(vals)
    k = 9
    for i, n in enumerate((2, 3, 5)):
        b.step(n)
        pts = np.stack([rng.integers(-2, W + 2, size=(E, k)), rng.integers(-2, H + 2, size=(E, k)), rng.integers(-1, 3, size=(E, k))],
                       axis=-1).astype(np.int32)
        pts[:, 0] = (W - 1, H - 1, 1)
        pts[:, 1] = pts[:, 2]
        src, thr = rw.MASK_PAIRS[i]
        r, maps, _ = _ask(b, src, thr, (8, 4, 0)[i], points=torch.from_numpy(pts).cuda(), value=True)
        _same(r, maps, range(E), src, thr, _conn(kw, (8, 4, 0)[i]), (mode, per_env, i), points=pts, values=vals)
        assert (r["value"] != 0).any() and (r["point_in"] == -1).any() and (r["point_in"] == 1).any()
    envs = [E - 1, 0, 0, 2]                                   # any order, repeats: points[i] and row i belong to envs[i]
    pts = pts[:4]
    r, maps, _ = _ask(b, BURNING, UNBURNED, 8, envs=envs, points=torch.from_numpy(pts).cuda(), value=True)
    _same(r, maps, envs, BURNING, UNBURNED, 8, (mode, per_env, "list"), points=pts, values=vals)
    only = b.reach(envs=[1], count=False, value=True)
    assert set(only) == {"value"} and int(only["value"][0]) == ro.value(ro.reach(b.fire_maps()[1], 2, 1, _conn(kw, 0)), vals if vals.ndim == 2 else vals[1])


@pytest.mark.parametrize("mode", ["run", "fused0"])
def test_points_are_the_agents_of_the_handle(mode):
    import torch
    import _agents_worlds as agw
    from simfire_amd.engine import FireEngine
    case = "24x40_k5_u1_att"
    c = agw.CASES[case]
    kw, R8, E, inits, starts = agw.make_world(case)
    b = FireEngine(n_envs=E, **kw)
    b.set_fused(aw.mode_settings(mode)["fused"])
    b.set_rtable(R8)
    b.reset(inits)
    b.agents_create(c["K"], inits, n_updates=1)
    b.agents_place(list(range(E)), starts)
    rng = np.random.default_rng(5102)
    seen = set()
    for t in range(6):
        b.agents_step(torch.from_numpy(rng.integers(0, 20, size=(E, c["K"])).astype(np.int32)).cuda())
        r = b.reach(BURNING, UNBURNED + ro.LINES, points=b.agents_device(), mask=True)
        got, mask = r["point_in"].cpu().numpy(), r["mask"].cpu().numpy()
        pos = b.agents_device().cpu().numpy()
        maps = b.fire_maps()
        for e in range(E):
            want = ro.reach(maps[e], 2, 1 | 56, _conn(kw, 0))
            assert (mask[e] == want).all() and got[e].tolist() == ro.point_in(want, pos[e]).tolist(), (mode, t, e)
            seen.update(got[e].tolist())
    assert {0, 1} <= seen


# ---------------------------------------------------------------------------------------------- 4. lists, chunks, many environments
@pytest.mark.parametrize("mode", ["run", "fused0"])
def test_lists_and_chunks(mode):
    import torch
    b, E, inits, kw = _world("24x40", mode)
    H, W = kw["shape"]
    need = b.reach_scratch_bytes()
    assert need == (2 * 1 * (16 * 16 + 20) + 255) // 256 * 256
    b.reset(inits)
    b.step(7)
    b.apply_mitigation(rw.line_rows(1, E, H, W, inits))
    b.step(2)
    mem0 = b.memory_bytes()                                  # (no getter between the measurements: they may allocate staging of their own)
    kwargs = dict(count=True, mask=True, seeds=True, rounds=True)
    one = b.reach(scratch_bytes=need, **kwargs)              # one environment per chunk: E chunks
    assert b.memory_bytes() - mem0 == need
    full = b.reach(**kwargs)
    assert b.memory_bytes() - mem0 == E * need               # grown to what the call needs ...
    b.reach(scratch_bytes=need, **kwargs)
    assert b.memory_bytes() - mem0 == E * need               # ... and never shrunk
    for name in kwargs:
        assert torch.equal(one[name], full[name]), name      # chunking changes no bit
    pts = np.random.default_rng(5103).integers(0, 24, size=(7, 5, 3)).astype(np.int32)
    dev = torch.from_numpy(pts).cuda()
    for envs in ([e for e in reversed(range(E))], [0, E - 1, 0, 0, 2, E - 1, 2], [1, 3], [2]):
        src, thr = rw.MASK_PAIRS[len(envs) % 4]
        p = dev[:len(envs)] if len(envs) <= 7 else None
        base, maps, _ = _ask(b, src, thr, 4, envs=envs, points=p)
        _same(base, maps, envs, src, thr, 4, (mode, envs), points=None if p is None else pts[:len(envs)])
        for scratch in (need, 2 * need + 7, 3 * need):
            got, _, _ = _ask(b, src, thr, 4, envs=envs, points=p, scratch_bytes=scratch)
            for name in base:
                assert (got[name] == base[name]).all(), (mode, envs, scratch, name)
    with pytest.raises(ValueError, match="scratch_bytes"):
        b.reach(scratch_bytes=need - 1)
    assert b.reach(envs=[], mask=True)["mask"].shape == (0, H, W)


def test_more_environments_than_cus():
    import torch
    n = torch.cuda.get_device_properties(0).multi_processor_count + 8
    b, E, inits, kw = _world("64x64_many", "auto_many", n)
    assert E == n
    b.reset(inits)
    b.step(7)
    b.apply_mitigation(rw.line_rows(2, E, 64, 64, inits))
    b.step(3)
    for src, thr, conn in ((BURNING, UNBURNED, 0), (BURNING, UNBURNED + ro.LINES, 4)):
        r, maps, _ = _ask(b, src, thr, conn)
        wants = _same(r, maps, range(E), src, thr, _conn(kw, conn), ("many", src, thr, conn))
    assert len({int(w.sum()) for w in wants}) > 8


# ---------------------------------------------------------------------------------------------- 5. reads only
@pytest.mark.parametrize("mode", ["run", "fused0"])
def test_reads_only(mode):
    """The same rollout on two handles, arrival recording and a value plane on, one of them with reach calls between its step calls:
    maps, burn amounts, status rows, elapsed times, arrival planes, damage and the ``fire_map_delta`` sequence are the same."""
    import torch
    kw, R8, E, inits = aw.make_world("24x40")
    H, W = kw["shape"]
    a, b = _engine(kw, E, R8, mode), _engine(kw, E, R8, mode)
    rng = np.random.default_rng(5104)
    vals = rng.integers(-1000, 1000, size=(H, W)).astype(np.int32)
    pts = torch.from_numpy(rng.integers(0, 24, size=(E, 7, 3)).astype(np.int32)).cuda()
    pas = torch.from_numpy((rng.random((H, W)) < 0.9).astype(np.uint8)).cuda()
    deltas = {id(a): [], id(b): []}
    for h in (a, b):
        h.reset(inits)
        h.enable_arrival(True)
        h.values_set(vals)
        for i, n in enumerate((1, 2, 3, 5)):
            h.step(n)
            if h is b:
                src, thr = rw.MASK_PAIRS[i]
                for call in (lambda: h.reach(src, thr, mask=True, value=True, seeds=True, rounds=True),
                             lambda: h.reach(src, thr, connectivity=4, points=pts, passable=pas),
                             lambda: h.reach(src, thr, envs=[E - 1, 0], scratch_bytes=h.reach_scratch_bytes(), max_rounds=1)):
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


# ---------------------------------------------------------------------------------------------- 6. errors
def test_errors_through_the_raw_call():
    import torch
    from simfire_amd import _lib
    b, E, inits, kw = _world("24x40", "run")
    H, W = kw["shape"]
    L, h = b._L, b._h
    need = b.reach_scratch_bytes()
    count = torch.full((E,), -7, dtype=torch.int32, device="cuda")
    value = torch.full((E,), -7, dtype=torch.int64, device="cuda")
    pin = torch.full((E, 3), -7, dtype=torch.int32, device="cuda")
    pts = torch.zeros((E, 3, 3), dtype=torch.int32, device="cuda")
    all_envs = np.arange(E, dtype=np.int32)

    def rc(n=E, envs=all_envs, reserved=(0, 0), outs=None, **fields):
        p = _lib.SfReachParams(**dict(dict(source_mask=2, through_mask=1), **fields))
        p.reserved[0], p.reserved[1] = reserved
        o = _lib.SfReachOut(**(dict(count=count.data_ptr()) if outs is None else outs))
        e = None if envs is None else np.ascontiguousarray(envs, dtype=np.int32)
        return L.sf_reach(h, C.byref(p), n, None if e is None else e.ctypes.data_as(C.c_void_p), C.byref(o))

    assert rc() == _lib.SF_ESTATE                             # before reset
    assert b"sf_reset" in L.sf_last_error()
    b.reset(inits)
    b.step(3)
    assert rc(outs=dict(value=value.data_ptr())) == _lib.SF_ESTATE and b"sf_values_set" in L.sf_last_error()      # no value plane
    bad = [dict(source_mask=0), dict(source_mask=64), dict(through_mask=0), dict(through_mask=-1), dict(through_mask=64),
           dict(source_mask=3, through_mask=1), dict(source_mask=2, through_mask=2 | 8), dict(connectivity=6), dict(connectivity=-1),
           dict(k=-1), dict(k=257), dict(k=3), dict(outs=dict(count=count.data_ptr(), point_in=pin.data_ptr())), dict(max_rounds=-1),
           dict(reserved=(1, 0)), dict(reserved=(0, 1)), dict(outs=dict()), dict(outs=dict(count=count.data_ptr() + 2)),
           dict(outs=dict(value=value.data_ptr() + 4)), dict(outs=dict(seeds=count.data_ptr() + 1)), dict(outs=dict(rounds=count.data_ptr() + 2)),
           dict(envs=[0, E]), dict(envs=[-1, 0], n=2), dict(scratch_bytes=need - 1), dict(scratch_bytes=1), dict(scratch_bytes=-1),
           dict(n=-1), dict(envs=None)]
    for kwargs in bad:
        kwargs = dict(kwargs)
        if "envs" in kwargs and kwargs["envs"] is not None and "n" not in kwargs:
            kwargs["n"] = len(kwargs["envs"])
        assert rc(**kwargs) == _lib.SF_EINVAL, kwargs
        assert b"sf_reach" in L.sf_last_error(), kwargs
    assert (count == -7).all() and (value == -7).all() and (pin == -7).all()          # nothing was enqueued
    assert rc(k=3, points=pts.data_ptr(), outs=dict(point_in=pin.data_ptr())) == _lib.SF_OK      # the call after an error works
    assert rc(n=0) == _lib.SF_OK
    assert (pin.cpu().numpy() == -1).all() and (count == -7).all()                    # (id 0: padding)
    r, maps, _ = _ask(b, BURNING, UNBURNED, 0)
    _same(r, maps, range(E), BURNING, UNBURNED, _conn(kw, 0), "after the errors")
    for kwargs in (dict(points=pts[:, :, :2]), dict(points=torch.zeros((E, 257, 3), dtype=torch.int32, device="cuda")), dict(points=pts.cpu()),
                   dict(passable=torch.ones((H, W), dtype=torch.float32, device="cuda")), dict(passable=torch.ones((H, W + 1), dtype=torch.uint8, device="cuda")),
                   dict(value=True)):
        with pytest.raises(ValueError, match="reach"):
            b.reach(**kwargs)


# ---------------------------------------------------------------------------------------------- 7. BatchedFireEnv
def _config_24x40():
    import yaml
    from simfire_amd.config import Config
    y = yaml.safe_load(open(os.path.join(CFG, "functional_config.yml")))
    y["area"]["screen_size"] = [24, 40]
    y["terrain"]["topography"]["functional"]["function"] = "flat"
    y["simulation"]["headless"] = True
    return Config(config_dict=y)


@pytest.mark.parametrize("option", [dict(), dict(source=("BURNING",), through=UNBURNED + ro.LINES, connectivity=4, value=True),
                                    dict(source=("BURNING", "BURNED"), connectivity=8)])
def test_batched_fire_env_reach(option):
    """``info["reach_cells"]``, ``info["agent_exposed"]`` and ``info["reach_value"]`` equal the oracle on the maps and ``positions()``
    the same ``step`` leaves, also on the tick in which every environment starts anew (max_ticks = 3); without the option ``info``
    has the old keys only."""
    import torch
    import simfire_amd
    from simfire_amd.simulation import BatchedFireSimulation
    cfg = _config_24x40()
    H, W = cfg.area.screen_size
    E, K = 3, 4
    ign = np.array([(10, 10), (W - 5, 7), (3, H - 4)], dtype=np.int32)
    starts = np.array([(0, 0), (W - 1, H - 1), (12, 10), (W // 2, 2)], dtype=np.int32)
    vals = np.random.default_rng(5105).integers(-50, 1000, size=(H, W)).astype(np.int32)
    want_value = option.get("value", False)
    sim = BatchedFireSimulation(cfg, E, ignitions=ign)
    env = simfire_amd.BatchedFireEnv(sim, K, starts, n_updates=1, max_ticks=3, reach=option, values=vals if want_value else None)
    plain = simfire_amd.BatchedFireEnv(BatchedFireSimulation(cfg, E, ignitions=ign), K, starts, n_updates=1, max_ticks=3,
                                       values=vals if want_value else None)
    src, thr = option.get("source", BURNING), option.get("through", UNBURNED)
    conn = option.get("connectivity") or (8 if sim._engine.params.diagonal_spread else 4)
    rng = np.random.default_rng(8809)
    env.reset()
    plain.reset()
    restarted = False
    new = {"reach_cells", "agent_exposed"} | ({"reach_value"} if want_value else set())
    for t in range(5):
        actions = torch.from_numpy(rng.integers(0, 20, size=(E, K)).astype(np.int32)).cuda()
        obs, reward, done, info = env.step(actions)
        obs_p, reward_p, done_p, info_p = plain.step(actions)
        assert not new & set(info_p) and set(info) == set(info_p) | new
        assert torch.equal(obs, obs_p) and torch.equal(done, done_p) and torch.equal(reward, reward_p)
        cells, exposed = info["reach_cells"], info["agent_exposed"]
        assert cells.shape == (E,) and cells.dtype == torch.int32 and cells.is_cuda and exposed.shape == (E, K) and exposed.dtype == torch.int32
        pos = env.positions().cpu().numpy()
        maps = sim._engine.fire_maps()
        for e in range(E):
            want = ro.reach(maps[e], ro.mask_of(src), ro.mask_of(thr), conn)
            assert int(cells[e]) == ro.count(want) and exposed[e].cpu().numpy().tolist() == ro.point_in(want, pos[e]).tolist(), (t, e, option)
            if want_value:
                assert info["reach_value"].dtype == torch.int64 and int(info["reach_value"][e]) == ro.value(want, vals)
        if bool(done.all().item()):
            restarted = True
            assert t == 2 and (maps == 1).sum() == E and (pos[:, :, :2] == starts[None]).all()      # the new episode's state
    assert restarted
    with pytest.raises(ValueError, match="reach"):
        simfire_amd.BatchedFireEnv(sim, K, starts, reach=dict(radius=3))
    with pytest.raises(ValueError, match="reach"):
        simfire_amd.BatchedFireEnv(sim, K, starts, reach=dict(source=("EMBERS",)))


# ---------------------------------------------------------------------------------------------- 8. the simulation classes
def test_simulation_classes_reach():
    import torch
    from simfire_amd.config import Config
    from simfire_amd.enums import BurnStatus
    from simfire_amd.simulation import BatchedFireSimulation, FireSimulation
    sim = FireSimulation(Config(os.path.join(CFG, "test_config_flat_simple.yml")))
    sim.run(2)
    m = np.asarray(sim.fire_map)
    H, W = m.shape
    conn = 8 if sim._engine.params.diagonal_spread else 4
    mask, count, value = sim.reach()
    want = ro.reach(m, 2, 1, conn)
    assert mask.dtype == bool and mask.shape == m.shape and (mask == want).all() and count == want.sum() > 0 and value is None
    ys, xs = np.nonzero(m == 1)
    y0, y1, x0, x1 = max(ys.min() - 2, 0), min(ys.max() + 2, H - 1), max(xs.min() - 2, 0), min(xs.max() + 2, W - 1)
    open_before = count
    # a host edit closes a ring round the fire (where the fire stands at a border of the grid, the border is that side of the ring)
    if y0 < ys.min():
        sim.fire_map[y0, x0:x1 + 1] = int(BurnStatus.FIRELINE)
    if y1 > ys.max():
        sim.fire_map[y1, x0:x1 + 1] = int(BurnStatus.FIRELINE)
    if x0 < xs.min():
        sim.fire_map[y0:y1 + 1, x0] = int(BurnStatus.FIRELINE)
    if x1 > xs.max():
        sim.fire_map[y0:y1 + 1, x1] = int(BurnStatus.FIRELINE)
    mask, count, _ = sim.reach(connectivity=8)
    m = np.asarray(sim.fire_map)
    want = ro.reach(m, 2, 1, 8)
    assert (m == 3).sum() > 0 and (mask == want).all() and count == want.sum()
    assert not mask[:y0].any() and not mask[y1 + 1:].any() and not mask[:, :x0].any() and not mask[:, x1 + 1:].any() and count < open_before
    assert count == ((m[y0:y1 + 1, x0:x1 + 1]) == 0).sum()
    everything, n_all, _ = sim.reach(through=("UNBURNED", "FIRELINE"), connectivity=4)
    assert n_all == (m == 0).sum() + (m == 3).sum() and everything[0, 0]
    bat = BatchedFireSimulation(_config_24x40(), 3)
    bat.run(4, return_maps=False)
    dev = bat.reach(envs=[2, 0], mask=True)
    host = bat.reach(envs=[2, 0], mask=True, device=False)
    assert dev["mask"].is_cuda and set(dev) == {"count", "seeds", "mask"} and all((dev[k].cpu().numpy() == host[k]).all() for k in dev)
    for i, e in enumerate((2, 0)):
        want = ro.reach(bat.fire_map(e), 2, 1, 8 if bat._engine.params.diagonal_spread else 4)
        assert (host["mask"][i] == want).all() and host["count"][i] == want.sum() and host["seeds"][i] == (bat.fire_map(e) == 1).sum()
    pts = torch.tensor([[[0, 0, 1], [50, 0, 1]], [[1, 1, 0], [2, 2, 3]]], dtype=torch.int32, device="cuda")
    assert bat.reach(envs=[2, 0], agents=pts, device=False)["point_in"].tolist() == [[int(host["mask"][0][0, 0]), -1], [-1, int(host["mask"][1][2, 2])]]
