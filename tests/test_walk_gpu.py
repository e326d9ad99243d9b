"""Walking distance on the GPU (``sf_walk``).  The yardstick is ``tests/_walk_oracle.py`` - level-by-level
dilation - fed with the maps the older getters return.  ``walk`` is always called FIRST and the maps are fetched afterwards (a getter
may convert the current plane); every comparison is equality.  Run with ``pytest -m gpu``."""
import ctypes as C
import os

import numpy as np
import pytest

import _arrival_worlds as aw
import _reach_oracle as ro
import _reach_worlds as rw
import _walk_oracle as wo
import _walk_worlds as ww

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


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ask(eng, tgt, thr, conn, envs=None, passable=None, targets=None, points=None, **more):
    """(every output of ``walk`` as NumPy arrays, the maps fetched AFTER the call, the layout the call read).  ``passable``,
    ``targets``, ``points``: host arrays."""
    lay, kind = eng.cell_layout(), eng.last_launch_kind()
    r = eng.walk(tgt, thr, envs=envs, connectivity=conn, passable=_dev(passable), targets=_dev(targets), points=_dev(points), plane=True,
                 step=points is not None and conn != 8, reached=True, levels=True, **more)
    assert (eng.cell_layout(), eng.last_launch_kind()) == (lay, kind)
    assert all(v.dtype.is_floating_point is False and v.is_cuda for v in r.values())
    r = {k: v.cpu().numpy() for k, v in r.items()}
    return r, eng.fire_maps(), lay


def _same(r, maps, envs, tgt, thr, conn, tag, passable=None, targets=None, points=None, max_moves=0):
    """Every output of every listed environment equals the oracle on its map.  Returns the oracle's answers."""
    H, W = maps.shape[1:]
    n = len(envs)
    assert r["moves"].shape == (n, H, W) and r["moves"].dtype == np.int32 and r["reached"].shape == (n,) and r["levels"].dtype == np.int32
    wants = []
    for i, e in enumerate(envs):
        p = None if passable is None else (passable if passable.ndim == 2 else passable[e])
        t = None if targets is None else (targets if targets.ndim == 2 else targets[e])
        want = wo.answer(maps[e], ro.mask_of(tgt) if tgt else 0, ro.mask_of(thr), conn, p, t, None if points is None else points[i], max_moves)
        bad = np.argwhere(r["moves"][i] != want["moves"])
        assert not len(bad), (tag, i, e, len(bad), bad[:5].tolist(), [(int(r["moves"][i][tuple(b)]), int(want["moves"][tuple(b)])) for b in bad[:5]])
        assert int(r["reached"][i]) == want["reached"], (tag, i, e, int(r["reached"][i]), want["reached"])
        assert int(r["levels"][i]) == want["levels"], (tag, i, e, int(r["levels"][i]), want["levels"])
        if points is not None:
            assert r["point_moves"][i].tolist() == want["point_moves"].tolist(), (tag, i, e, r["point_moves"][i].tolist(), want["point_moves"].tolist())
            if conn != 8:
                assert r["point_step"][i].tolist() == want["point_step"].tolist(), (tag, i, e, r["point_step"][i].tolist(), want["point_step"].tolist())
        wants.append(want)
    return wants


# ---------------------------------------------------------------------------------------------- 1. through an episode
@pytest.mark.parametrize("case,mode", rw.PAIRS, ids=["%s-%s" % p for p in rw.PAIRS])
def test_walk_through_an_episode(case, mode):
    """Behind calls of 1, 2, 3, 5, 7 and 11 updates, the mask pairs and connectivities of ``_walk_worlds.queries`` in turn, control
    lines drawn between the calls of every second mode: the plane form, ``reached`` and ``levels`` of every environment and the point
    form for a set of points equal the oracle on the maps; the ``run*`` modes were read in the blocked layout, ``fused0`` in the
    row-major one."""
    kw, R8, E, inits = aw.make_world(case)
    b = _engine(kw, E, R8, mode)
    H, W = kw["shape"]
    lays, sizes = [], []
    pts = np.stack([ww.default_points(H, W, e) for e in range(E)])

    def on_query(i, n, tgt, thr, conn):
        r, maps, lay = _ask(b, tgt, thr, conn, points=pts)
        wants = _same(r, maps, range(E), tgt, thr, conn, (case, mode, i, n, tgt, thr, conn), points=pts)
        lays.append(lay)
        sizes.append(sum(w["reached"] for w in wants))
    ww.run_episode(case, mode, b, inits, on_query, H, W)
    print("layouts behind the calls:", case, mode, lays, "cells reached:", sizes)
    assert max(sizes) > 0
    if mode.startswith("run"):
        assert lays == [1] * len(rw.CALLS), lays
    if mode == "fused0":
        assert lays == [0] * len(rw.CALLS), lays


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
    rng = np.random.default_rng(5202)
    seen = set()
    for t in range(6):
        b.agents_step(torch.from_numpy(rng.integers(0, 20, size=(E, c["K"])).astype(np.int32)).cuda())
        tgt, thr = ww.MASK_PAIRS[t % 2]
        r = b.walk(tgt, thr, points=b.agents_device(), step=True, plane=True)
        pos = b.agents_device().cpu().numpy()
        maps = b.fire_maps()
        for e in range(E):
            want = wo.answer(maps[e], ro.mask_of(tgt), ro.mask_of(thr), 4, pts=pos[e])
            assert (r["moves"][e].cpu().numpy() == want["moves"]).all(), (mode, t, e)
            assert r["point_moves"][e].tolist() == want["point_moves"].tolist() and r["point_step"][e].tolist() == want["point_step"].tolist(), (mode, t, e)
            seen.update(want["point_step"].tolist())
    assert len(seen - {0, -1}) >= 2


# ---------------------------------------------------------------------------------------------- 2. the hand-made scenes
@pytest.mark.parametrize("shape", ww.SCENE_SHAPES, ids=["%dx%d" % s for s in ww.SCENE_SHAPES])
@pytest.mark.parametrize("mode", ["fused0", "run"])
def test_scenes(shape, mode):
    """Every scene of ``_walk_worlds.scenes`` in an environment of its own through ``load_fire_map``.  ``fused0``: read in the
    row-major layout as loaded - equality with the oracle and what the scene claims.  ``run``: one update first, so that the cells lie
    in the blocked plane - equality with the oracle on the maps as they are then."""
    H, W = shape
    sc = ww.scenes(H, W)
    E = len(sc)
    kw, R8 = rw.make_scene_world(H, W, True)
    b = _engine(kw, E, R8, mode)
    b.reset(np.full((E, 2), 0, dtype=np.int32))
    for e, s in enumerate(sc):
        b.load_fire_map(e, s["map"])
    if mode == "run":
        b.step(1)
    per_pas, per_tgt = rw.per_env_passable(E, H, W), ww.per_env_targets(E, H, W)
    lays = []
    for e, s in enumerate(sc):
        pas = per_pas if isinstance(s["passable"], str) else s["passable"]
        tgt = per_tgt if isinstance(s["targets"], str) else s["targets"]
        pts = s["points"][None]
        r, maps, lay = _ask(b, s["target"], s["through"], s["conn"], envs=[e], passable=pas, targets=tgt, points=pts)
        _same(r, maps, [e], s["target"], s["through"], s["conn"], (shape, mode, s["name"]), passable=pas, targets=tgt, points=pts)
        if mode == "fused0":
            assert (maps[e] == s["map"]).all()
            if s["claim"] is not None:
                steps = r["point_step"][0] if s["conn"] != 8 else np.where(r["point_moves"][0] < 0, -1, 0)
                s["claim"](r["moves"][0], r["point_moves"][0], steps, int(r["reached"][0]), int(r["levels"][0]))
        lays.append(lay)
    if mode == "run" and H * W > 81:
        assert set(lays) == {1}, lays
    if mode == "fused0":
        assert set(lays) == {0}, lays


@pytest.mark.parametrize("mode", ["fused0", "run"])
def test_max_moves(mode):
    """A straight corridor of 30 cells: capped at 1, inside it, and at exactly its length, the point whose value equals the cap still
    gets its step; one cell further along the value is the cap and the step 0; plane, ``reached`` and ``levels`` follow the cap."""
    H, W = 9, 40
    kw, R8 = rw.make_scene_world(H, W, True)
    b = _engine(kw, 2, R8, mode)
    b.reset(np.zeros((2, 2), dtype=np.int32))
    b.load_fire_map(1, ww.corridor(H, W, 30))
    if mode == "run":
        b.step(1)
    for M in (1, 17, 30, 31, 0):
        c = min(M, 30) if M else 30
        pts = np.array([[[1 + c, 2, 1], [2 + c, 2, 1], [c, 1, 1], [1 + c, 1, 1]]], dtype=np.int32)      # at the cap; one cell on; beside the route, twice
        r, maps, _ = _ask(b, BURNING, UNBURNED, 4, envs=[1], points=pts, max_moves=M or None)
        _same(r, maps, [1], BURNING, UNBURNED, 4, (mode, M), points=pts, max_moves=M)
        if mode == "run":
            continue                                          # (the update may have moved the fire: equality with the oracle only)
        assert (maps[1] >= 3).sum() == H * W - 31
        if 0 < M <= 30:
            assert r["point_moves"][0].tolist() == [M] * 4 and r["point_step"][0].tolist() == [3, 0, 2, 0] and int(r["levels"][0]) == M == int(r["reached"][0])
            assert r["moves"][0].max() == M
        else:
            assert int(r["levels"][0]) == 30 and r["point_moves"][0].tolist() == [30, 31, 30, 31] and r["point_step"][0].tolist() == [3, 3, 2, 2]


@pytest.mark.parametrize("mode", ["fused0", "run"])
def test_more_bands_than_threads(mode):
    """977 x 1030: 62 band rows (the last with one row) x 17 words (the last with 6 cells) = 1054 bands - the kernel that walks the
    bands in passes over the scratch planes, its second pass partly empty.  Random maps with many targets (few levels for the
    oracle), a strip the search has to cross under a cap, and a wall."""
    H, W = 977, 1030
    kw, R8 = rw.make_scene_world(H, W, True)
    b = _engine(kw, 2, R8, mode)
    assert b.walk_scratch_bytes() == (1054 * (16 * 24 + 40) + 255) // 256 * 256
    b.reset(np.zeros((2, 2), dtype=np.int32))
    rng = np.random.default_rng(5206)
    for e in range(2):
        u = rng.random((H, W))
        m = np.where(u < 0.2, 3, np.where(u < 0.22, 1, np.where(u < 0.26, 2, 0))).astype(np.uint8)
        m[:, 40:240] = 0                                      # a strip wider than the cap
        m[:, 700] = 3 + e                                     # a wall: what lies beyond is reached from its own targets only
        m[H - 1, :] = 0                                       # the last band row: a single row of cells
        b.load_fire_map(e, m)
    if mode == "run":
        b.step(1)
    pts = np.stack([rng.integers(-2, W + 2, size=(2, 40)), rng.integers(-2, H + 2, size=(2, 40)), rng.integers(0, 3, size=(2, 40))], axis=-1).astype(np.int32)
    pts[:, 0] = (W - 1, H - 1, 1)
    pts[:, 1] = (140, H // 2, 1)
    for tgt, thr, conn, M in ((BURNING, UNBURNED, 4, 60), (BURNING, UNBURNED + ("BURNED",), 8, 0)):
        r, maps, lay = _ask(b, tgt, thr, conn, points=pts, max_moves=M or None)
        _same(r, maps, range(2), tgt, thr, conn, (mode, conn), points=pts, max_moves=M)
        assert lay == (1 if mode == "run" else 0) and r["levels"].min() > 10 and r["reached"].min() > 0
    assert (r["levels"] <= 150).all()
    one = b.walk(tgt, thr, connectivity=conn, plane=True, levels=True, reached=True, scratch_bytes=b.walk_scratch_bytes())
    assert all((one[k].cpu().numpy() == r[k]).all() for k in ("moves", "levels", "reached"))


# ---------------------------------------------------------------------------------------------- 3. lists, chunks, many environments
@pytest.mark.parametrize("mode", ["run", "fused0"])
def test_lists_and_chunks(mode):
    import torch
    kw, R8, E, inits = aw.make_world("24x40")
    b = _engine(kw, E, R8, mode)
    H, W = kw["shape"]
    need = b.walk_scratch_bytes()
    assert need == (2 * 1 * (16 * 24 + 40) + 255) // 256 * 256
    b.reset(inits)
    b.step(7)
    b.apply_mitigation(rw.line_rows(1, E, H, W, inits))
    b.step(2)
    mem0 = b.memory_bytes()                                  # (no getter between the measurements: they may allocate staging of their own)
    kwargs = dict(plane=True, reached=True, levels=True)
    one = b.walk(scratch_bytes=need, **kwargs)               # one environment per chunk: E chunks
    assert b.memory_bytes() - mem0 == need
    full = b.walk(**kwargs)
    assert b.memory_bytes() - mem0 == E * need               # grown to what the call needs ...
    b.walk(scratch_bytes=need, **kwargs)
    assert b.memory_bytes() - mem0 == E * need               # ... and never shrunk
    for name in ("moves", "reached", "levels"):
        assert torch.equal(one[name], full[name]), name      # chunking changes no bit
    pts = np.random.default_rng(5203).integers(0, 24, size=(7, 5, 3)).astype(np.int32)
    for envs in ([e for e in reversed(range(E))], [0, E - 1, 0, 0, 2, E - 1, 2], [1, 3], [2]):
        tgt, thr = ww.MASK_PAIRS[len(envs) % 4]
        p = pts[:len(envs)] if len(envs) <= 7 else None
        base, maps, _ = _ask(b, tgt, thr, 4, envs=envs, points=p)
        _same(base, maps, envs, tgt, thr, 4, (mode, envs), points=p)
        for scratch in (need, 2 * need + 7, 3 * need):
            got, _, _ = _ask(b, tgt, thr, 4, envs=envs, points=p, scratch_bytes=scratch)
            for name in base:
                assert (got[name] == base[name]).all(), (mode, envs, scratch, name)
    with pytest.raises(ValueError, match="scratch_bytes"):
        b.walk(plane=True, scratch_bytes=need - 1)
    assert b.walk(envs=[], plane=True)["moves"].shape == (0, H, W)


def test_more_environments_than_cus():
    import torch
    n = torch.cuda.get_device_properties(0).multi_processor_count + 8
    kw, R8, E, inits = aw.make_world("64x64_many", n)
    b = _engine(kw, E, R8, "auto_many")
    assert E == n
    b.reset(inits)
    b.step(7)
    b.apply_mitigation(rw.line_rows(2, E, 64, 64, inits))
    b.step(3)
    for tgt, thr, conn in ((BURNING, UNBURNED, 4), (BURNING, UNBURNED + ro.LINES, 8)):
        r, maps, _ = _ask(b, tgt, thr, conn)
        wants = _same(r, maps, range(E), tgt, thr, conn, ("many", tgt, thr, conn))
    assert len({w["reached"] for w in wants}) > 8


# ---------------------------------------------------------------------------------------------- 4. reads only
@pytest.mark.parametrize("mode", ["run", "fused0"])
def test_reads_only(mode):
    """The same rollout on two handles, arrival recording and a value plane on, one of them with walk calls between its step calls:
    maps, burn amounts, status rows, elapsed times, arrival planes, damage and the ``fire_map_delta`` sequence are the same."""
    import torch
    kw, R8, E, inits = aw.make_world("24x40")
    H, W = kw["shape"]
    a, b = _engine(kw, E, R8, mode), _engine(kw, E, R8, mode)
    rng = np.random.default_rng(5204)
    vals = rng.integers(-1000, 1000, size=(H, W)).astype(np.int32)
    pts = torch.from_numpy(rng.integers(0, 24, size=(E, 7, 3)).astype(np.int32)).cuda()
    pas = torch.from_numpy((rng.random((H, W)) < 0.9).astype(np.uint8)).cuda()
    tgs = torch.from_numpy((rng.random((E, H, W)) < 0.01).astype(np.uint8)).cuda()
    deltas = {id(a): [], id(b): []}
    for h in (a, b):
        h.reset(inits)
        h.enable_arrival(True)
        h.values_set(vals)
        for i, n in enumerate((1, 2, 3, 5)):
            h.step(n)
            if h is b:
                tgt, thr = ww.MASK_PAIRS[i]
                for call in (lambda: h.walk(tgt, thr, plane=True, reached=True, levels=True),
                             lambda: h.walk(tgt, thr, connectivity=4, points=pts, step=True, passable=pas, targets=tgs),
                             lambda: h.walk(None, thr, connectivity=8, envs=[E - 1, 0], targets=tgs, plane=True, scratch_bytes=h.walk_scratch_bytes(), max_moves=3)):
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


# ---------------------------------------------------------------------------------------------- 5. errors
def test_errors_through_the_raw_call():
    import torch
    from simfire_amd import _lib
    kw, R8, E, inits = aw.make_world("24x40")
    b = _engine(kw, E, R8, "run")
    H, W = kw["shape"]
    L, h = b._L, b._h
    need = b.walk_scratch_bytes()
    reached = torch.full((E,), -7, dtype=torch.int32, device="cuda")
    pm = torch.full((E, 3), -7, dtype=torch.int32, device="cuda")
    pts = torch.zeros((E, 3, 3), dtype=torch.int32, device="cuda")
    tg = torch.ones((H, W), dtype=torch.uint8, device="cuda")
    all_envs = np.arange(E, dtype=np.int32)

    def rc(n=E, envs=all_envs, reserved=(0, 0), outs=None, **fields):
        p = _lib.SfWalkParams(**dict(dict(target_mask=2, through_mask=1), **fields))
        p.reserved[0], p.reserved[1] = reserved
        o = _lib.SfWalkOut(**(dict(reached=reached.data_ptr()) if outs is None else outs))
        e = None if envs is None else np.ascontiguousarray(envs, dtype=np.int32)
        return L.sf_walk(h, C.byref(p), n, None if e is None else e.ctypes.data_as(C.c_void_p), C.byref(o))

    assert rc() == _lib.SF_ESTATE                             # before reset
    assert b"sf_reset" in L.sf_last_error()
    b.reset(inits)
    b.step(3)
    both = dict(reached=reached.data_ptr(), point_moves=pm.data_ptr())
    bad = [dict(target_mask=0), dict(target_mask=-1), dict(target_mask=64), dict(through_mask=0), dict(through_mask=-1), dict(through_mask=64),
           dict(target_mask=64, targets=tg.data_ptr()), dict(connectivity=6), dict(connectivity=-1), dict(connectivity=1),
           dict(k=-1), dict(k=257, points=pts.data_ptr()), dict(k=3), dict(points=pts.data_ptr()), dict(outs=both),
           dict(outs=dict(point_step=pm.data_ptr())), dict(k=3, points=pts.data_ptr(), connectivity=8, outs=dict(point_step=pm.data_ptr())),
           dict(max_moves=-1), dict(reserved=(1, 0)), dict(reserved=(0, 1)), dict(outs=dict()), dict(outs=dict(reached=reached.data_ptr() + 2)),
           dict(outs=dict(moves=reached.data_ptr() + 1)), dict(outs=dict(levels=reached.data_ptr() + 2)),
           dict(k=3, points=pts.data_ptr(), outs=dict(point_moves=pm.data_ptr() + 1)),
           dict(envs=[0, E]), dict(envs=[-1, 0], n=2), dict(scratch_bytes=need - 1), dict(scratch_bytes=1), dict(scratch_bytes=-1),
           dict(n=-1), dict(envs=None)]
    for kwargs in bad:
        kwargs = dict(kwargs)
        if "envs" in kwargs and kwargs["envs"] is not None and "n" not in kwargs:
            kwargs["n"] = len(kwargs["envs"])
        assert rc(**kwargs) == _lib.SF_EINVAL, kwargs
        assert b"sf_walk" in L.sf_last_error(), kwargs
    assert (reached == -7).all() and (pm == -7).all()         # nothing was enqueued
    assert rc(k=3, points=pts.data_ptr(), outs=dict(point_moves=pm.data_ptr())) == _lib.SF_OK      # the call after an error works
    assert rc(n=0) == _lib.SF_OK
    assert rc(target_mask=0, targets=tg.data_ptr()) == _lib.SF_OK
    b.sync()
    assert (pm.cpu().numpy() == -1).all() and (reached.cpu().numpy() == 0).all()      # (id 0: padding; every cell a target: none reached)
    r, maps, _ = _ask(b, BURNING, UNBURNED, 4)
    _same(r, maps, range(E), BURNING, UNBURNED, 4, "after the errors")
    for kwargs in (dict(points=pts[:, :, :2]), dict(points=torch.zeros((E, 257, 3), dtype=torch.int32, device="cuda")), dict(points=pts.cpu()),
                   dict(passable=torch.ones((H, W), dtype=torch.float32, device="cuda")), dict(targets=torch.ones((H, W + 1), dtype=torch.uint8, device="cuda")),
                   dict(points=pts, step=True, connectivity=8)):
        with pytest.raises(ValueError, match="walk"):
            b.walk(plane=True, **kwargs)


# ---------------------------------------------------------------------------------------------- 6. BatchedFireEnv
def _config_24x40():
    import yaml
    from simfire_amd.config import Config
    y = yaml.safe_load(open(os.path.join(CFG, "functional_config.yml")))
    y["area"]["screen_size"] = [24, 40]
    y["terrain"]["topography"]["functional"]["function"] = "flat"
    y["simulation"]["headless"] = True
    return Config(config_dict=y)


def _maze(H, W):
    """uint8 [H, W]: two closed columns near the right border, each with one gap - the way to the target winds through both."""
    p = np.ones((H, W), dtype=np.uint8)
    p[:, W - 6] = 0
    p[10, W - 6] = 1
    p[:, W - 3] = 0
    p[13, W - 3] = 1
    return p


@pytest.mark.parametrize("max_ticks", [0, 5])
def test_batched_fire_env_moves_to(max_ticks):
    """``through`` is every status, ``passable`` a maze and ``targets`` one cell, so the fire does not matter: agents fed
    ``info["move_toward"]`` as their actions see ``info["moves_to"]`` fall by exactly 1 per tick to 0 and stay there with move 0.
    With ``max_ticks = 5`` the run goes through an auto-reset tick: the agents are back on their start cells and ``info`` describes
    the new episode.  Without the option ``info`` has the old keys only."""
    import torch
    import simfire_amd
    from simfire_amd.simulation import BatchedFireSimulation
    cfg = _config_24x40()
    H, W = cfg.area.screen_size
    E, K = 3, 4
    ign = np.array([(10, 10), (W - 5, 7), (3, H - 4)], dtype=np.int32)
    starts = np.array([(W - 1, 16), (W - 2, 11), (W - 4, 16), (W - 7, 9)], dtype=np.int32)       # (short routes: the fires outlast the run)
    maze = _maze(H, W)
    tg = np.zeros((H, W), dtype=np.uint8)
    tg[15, W - 1] = 1
    option = dict(target=None, through=ww.EVERY, passable=_dev(maze), targets=_dev(tg))
    sim = BatchedFireSimulation(cfg, E, ignitions=ign)
    env = simfire_amd.BatchedFireEnv(sim, K, starts, n_updates=1, max_ticks=max_ticks, moves_to=option)
    plain = simfire_amd.BatchedFireEnv(BatchedFireSimulation(cfg, E, ignitions=ign), K, starts, n_updates=1, max_ticks=max_ticks)
    zero = wo.answer(np.zeros((H, W), dtype=np.uint8), 0, 63, 4, maze, tg, np.concatenate([starts, np.ones((K, 1), dtype=np.int32)], axis=1))
    first = zero["point_moves"]
    assert first.tolist() == [1, 5, 8, 12]                    # the last two wind through one and both gaps
    d0 = wo.true_moves(np.zeros((H, W), dtype=np.uint8), 0, 63, 4, maze, tg)[0]
    env.reset()
    plain.reset()
    actions = torch.zeros((E, K), dtype=torch.int32, device="cuda")
    obs, reward, done, info = env.step(actions)               # a tick without a move: where the agents stand
    obs_p, reward_p, done_p, info_p = plain.step(actions)
    assert set(info) == set(info_p) | {"moves_to", "move_toward"} and torch.equal(obs, obs_p) and torch.equal(reward, reward_p)
    assert info["moves_to"].dtype == torch.int32 and info["moves_to"].shape == (E, K) and info["move_toward"].shape == (E, K) and info["moves_to"].is_cuda
    assert (info["moves_to"].cpu().numpy() == first[None]).all() and (info["move_toward"].cpu().numpy() == zero["point_step"][None]).all()
    last = info["moves_to"].clone()
    ticks = 1
    restarted = False
    for t in range(int(first.max()) + 3 if not max_ticks else 9):
        obs, reward, done, info = env.step(info["move_toward"])
        ticks += 1
        now = info["moves_to"]
        if max_ticks and ticks % max_ticks == 0:              # the auto-reset tick: the new episode's agents
            assert bool(done.all().item())
            restarted = True
            assert (env.positions().cpu().numpy()[:, :, :2] == starts[None]).all() and (now.cpu().numpy() == first[None]).all()
        else:
            assert not bool(done.any().item()), (t, "an episode ended on its own: the agents were moved")
            assert torch.equal(now, torch.clamp(last - 1, min=0)), (t, now.tolist(), last.tolist())
        assert torch.equal(info["move_toward"] == 0, now == 0)
        pos = env.positions().cpu().numpy()
        want = wo.points_of(d0, pos[0], 4)
        assert now[0].cpu().numpy().tolist() == want[0].tolist() and info["move_toward"][0].cpu().numpy().tolist() == want[1].tolist()
        last = now.clone()
    assert restarted == bool(max_ticks)
    if not max_ticks:
        assert (last == 0).all() and (env.positions().cpu().numpy()[:, :, :2] == (W - 1, 15)).all()
    with pytest.raises(ValueError, match="moves_to"):
        simfire_amd.BatchedFireEnv(sim, K, starts, moves_to=dict(radius=3))


# ---------------------------------------------------------------------------------------------- 7. the simulation classes
def test_simulation_classes_moves_to():
    import torch
    from simfire_amd.config import Config
    from simfire_amd.enums import BurnStatus
    from simfire_amd.simulation import BatchedFireSimulation, FireSimulation
    sim = FireSimulation(Config(os.path.join(CFG, "test_config_flat_simple.yml")))
    sim.run(2)
    m = np.asarray(sim.fire_map)
    H, W = m.shape
    mv = sim.moves_to()
    assert mv.dtype == np.int32 and mv.shape == m.shape and (mv == wo.moves(m, 2, 1, 4)).all() and 0 < mv.max() < wo.FAR
    ys, xs = np.nonzero(m == 1)
    y0, y1, x0, x1 = max(ys.min() - 2, 0), min(ys.max() + 2, H - 1), max(xs.min() - 2, 0), min(xs.max() + 2, W - 1)
    # a host edit closes the corridor: a ring of line round the fire (where the fire stands at a border, the border is that side)
    if y0 < ys.min():
        sim.fire_map[y0, x0:x1 + 1] = int(BurnStatus.FIRELINE)
    if y1 > ys.max():
        sim.fire_map[y1, x0:x1 + 1] = int(BurnStatus.FIRELINE)
    if x0 < xs.min():
        sim.fire_map[y0:y1 + 1, x0] = int(BurnStatus.FIRELINE)
    if x1 > xs.max():
        sim.fire_map[y0:y1 + 1, x1] = int(BurnStatus.FIRELINE)
    mv = sim.moves_to(connectivity=8)
    m = np.asarray(sim.fire_map)
    assert (m == 3).sum() > 0 and (mv == wo.moves(m, 2, 1, 8)).all()
    outside = np.ones((H, W), dtype=bool)
    outside[y0:y1 + 1, x0:x1 + 1] = False
    assert (mv[outside & (m == 0)] == wo.FAR).all() and (mv[m == 3] == wo.BLOCKED).all() and (mv == wo.FAR).sum() > 0
    capped = sim.moves_to(through=("UNBURNED", "FIRELINE"), max_moves=5)
    assert (capped == wo.moves(m, 2, 1 | 8, 4, max_moves=5)).all() and capped.max() == 5
    bat = BatchedFireSimulation(_config_24x40(), 3)
    bat.run(4, return_maps=False)
    dev = bat.moves_to(envs=[2, 0], plane=True)
    host = bat.moves_to(envs=[2, 0], plane=True, device=False)
    assert dev["moves"].is_cuda and set(dev) == {"moves", "reached", "levels"} and all((dev[k].cpu().numpy() == host[k]).all() for k in dev)
    for i, e in enumerate((2, 0)):
        want = wo.answer(bat.fire_map(e), 2, 1, 4)
        assert (host["moves"][i] == want["moves"]).all() and host["reached"][i] == want["reached"] and host["levels"][i] == want["levels"]
    pts = torch.tensor([[[0, 0, 1], [50, 0, 1]], [[1, 1, 0], [2, 2, 3]]], dtype=torch.int32, device="cuda")
    got = bat.moves_to(envs=[2, 0], agents=pts, step=True, device=False)
    assert got["point_moves"].tolist() == [[int(host["moves"][0][0, 0]), -1], [-1, int(host["moves"][1][2, 2])]]
    assert got["point_step"][0][1] == -1 and got["point_step"][1][0] == -1 and 1 <= got["point_step"][0][0] <= 4
