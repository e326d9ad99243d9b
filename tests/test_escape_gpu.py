"""Escape routes on the GPU (``sf_escape``).  The yardstick is ``tests/_escape_oracle.py`` - a max-min
Dijkstra - fed with the maps the older getters return and the same ``minutes``.  ``escape`` is always called FIRST and the maps are
fetched afterwards (a getter may convert the current plane); every comparison is equality, over the plane, the points, the steps
and the four summaries.  Run with ``pytest -m gpu``."""
import ctypes as C
import os

import numpy as np
import pytest

import _arrival_worlds as aw
import _escape_oracle as eo
import _escape_worlds as ew
import _reach_oracle as ro
import _reach_worlds as rw

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tests", "golden", "configs")
BURNING, UNBURNED, BURNED = ("BURNING",), ("UNBURNED",), ("BURNED",)
SUMMARY = ("safe", "escapable", "lost", "top")


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
    return None if a is None else (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).cuda())


def _horizon(eng, envs=None, q=50):
    """A horizon in minutes that the fires of the handle reach part of the grid within: a percentile of the finite travel times, so
    that the closing times a test hands over mix deadlines and NEVER whatever the rates of spread are."""
    t = eng.travel(envs=envs, plane=True)["minutes"].cpu().numpy()
    t = t[np.isfinite(t) & (t > 0)]
    return float(np.percentile(t, q)) if t.size else 1.0


def _ask(eng, minutes, tgt, thr, conn=4, envs=None, passable=None, targets=None, points=None, per_move=1.0, margin=0.0, horizon=64.0,
         flag=False, **more):
    """(every output of ``escape`` as NumPy arrays, the maps fetched AFTER the call, the layout the call read)."""
    lay, kind = eng.cell_layout(), eng.last_launch_kind()
    r = eng.escape(_dev(minutes), target=tgt, through=thr, envs=envs, connectivity=conn, passable=_dev(passable), targets=_dev(targets),
                   points=_dev(points), minutes_per_move=per_move, margin_minutes=margin, horizon_minutes=horizon, unreached_safe=flag,
                   plane=True, step=points is not None, summary=True, **more)
    assert (eng.cell_layout(), eng.last_launch_kind()) == (lay, kind)
    assert all(v.dtype.is_floating_point is False and v.is_cuda for v in r.values())
    r = {k: v.cpu().numpy() for k, v in r.items()}
    return r, eng.fire_maps(), lay


def _same(r, maps, minutes, envs, tgt, thr, conn, tag, passable=None, targets=None, points=None, per_move=1.0, margin=0.0, horizon=64.0,
          flag=False):
    """Every output of every listed environment equals the oracle on its map.  Returns the oracle's answers."""
    H, W = maps.shape[1:]
    n = len(envs)
    assert r["slack"].shape == (n, H, W) and r["slack"].dtype == np.int32 and all(r[k].shape == (n,) and r[k].dtype == np.int32 for k in SUMMARY)
    wants = []
    for i, e in enumerate(envs):
        p = None if passable is None else (passable if passable.ndim == 2 else passable[e])
        t = None if targets is None else (targets if targets.ndim == 2 else targets[e])
        want = eo.answer(maps[e], np.asarray(minutes)[i], ro.mask_of(tgt) if tgt else 0, ro.mask_of(thr), conn, p, t,
                         None if points is None else points[i], per_move, margin, horizon, flag)
        bad = np.argwhere(r["slack"][i] != want["slack"])
        assert not len(bad), (tag, i, e, len(bad), bad[:5].tolist(), [(int(r["slack"][i][tuple(b)]), int(want["slack"][tuple(b)])) for b in bad[:5]])
        got = tuple(int(r[k][i]) for k in SUMMARY)
        assert got == tuple(want[k] for k in SUMMARY), (tag, i, e, got, [want[k] for k in SUMMARY])
        if points is not None:
            assert r["point_slack"][i].tolist() == want["point_slack"].tolist(), (tag, i, e, r["point_slack"][i].tolist(), want["point_slack"].tolist())
            assert r["point_step"][i].tolist() == want["point_step"].tolist(), (tag, i, e, r["point_step"][i].tolist(), want["point_step"].tolist())
        wants.append(want)
    return wants


# ---------------------------------------------------------------------------------------------- 1. the hand-made scenes
@pytest.mark.parametrize("shape", ew.SCENE_SHAPES, ids=["%dx%d" % s for s in ew.SCENE_SHAPES])
@pytest.mark.parametrize("mode", ["fused0", "run"])
def test_scenes(shape, mode):
    """Every scene of ``_escape_worlds.scenes`` in an environment of its own through ``load_fire_map``.  ``fused0``: read in the
    row-major layout as loaded - equality with the oracle and what the scene claims.  ``run``: one update first, so that the cells lie
    in the blocked plane - equality with the oracle on the maps as they are then."""
    H, W = shape
    sc = ew.scenes(H, W)
    E = len(sc)
    kw, R8 = rw.make_scene_world(H, W, True)
    b = _engine(kw, E, R8, mode)
    b.reset(np.full((E, 2), 0, dtype=np.int32))
    for e, s in enumerate(sc):
        b.load_fire_map(e, s["map"])
    if mode == "run":
        b.step(1)
    lays = []
    for e, s in enumerate(sc):
        args = dict(passable=s["passable"], targets=s["targets"], points=s["points"][None], per_move=s["per_move"], margin=s["margin"],
                    horizon=s["horizon"], flag=s["flag"])
        r, maps, lay = _ask(b, s["minutes"][None], s["target"], s["through"], s["conn"], envs=[e], **args)
        _same(r, maps, s["minutes"][None], [e], s["target"], s["through"], s["conn"], (shape, mode, s["name"]), **args)
        if mode == "fused0":
            assert (maps[e] == s["map"]).all()
            if s["claim"] is not None:
                s["claim"]({k: v[0] for k, v in r.items()})
        lays.append(lay)
    if mode == "run" and H * W > 81:
        assert set(lays) == {1}, lays
    if mode == "fused0":
        assert set(lays) == {0}, lays


# ---------------------------------------------------------------------------------------------- 2. episodes under the real forecast
@pytest.mark.parametrize("case,mode", [("24x40", "run"), ("24x40", "fused0"), ("72x80_win", "run_win")])
def test_through_an_episode(case, mode):
    """Behind calls of a few updates, with lines drawn in between: ``minutes`` is the real ``travel(max_minutes=horizon)``, the
    targets a plane (shared, then per environment) or a status, ``passable`` shared and per environment, both connectivities."""
    kw, R8, E, inits = aw.make_world(case)
    b = _engine(kw, E, R8, mode)
    H, W = kw["shape"]
    b.reset(inits)
    rng = np.random.default_rng(3201)
    tg_all = np.zeros((H, W), dtype=np.uint8)
    tg_all[0, :] = tg_all[:, 0] = 1
    tg_env, pas_env = ew.per_env_targets(E, H, W), rw.per_env_passable(E, H, W)
    pas_all = (rng.random((H, W)) < 0.9).astype(np.uint8)
    pts = np.stack([ew.default_points(H, W, e) for e in range(E)])
    finite, steps = 0, set()
    for i, n in enumerate((2, 3, 5, 7)):
        b.step(n)
        if i == 1:
            b.apply_mitigation(rw.line_rows(1, E, H, W, inits))
        horizon = _horizon(b)
        mins = b.travel(max_minutes=float(np.float32(horizon)), plane=True)["minutes"]
        tgt, targets = ((), tg_all) if i % 3 == 0 else (((), tg_env) if i % 3 == 1 else (BURNED + ("FIRELINE",), None))
        per_move = horizon / (24, 50, 10, 30)[i]
        args = dict(passable=(None, pas_all, pas_env)[i % 3], targets=targets, points=pts, per_move=per_move,
                    margin=per_move * (0.0, 1.5, 0.5, 3.0)[i], horizon=horizon, flag=i == 3)
        r, maps, lay = _ask(b, mins, tgt, UNBURNED, (4, 8)[i % 2], **args)
        wants = _same(r, maps, mins.cpu().numpy(), range(E), tgt, UNBURNED, (4, 8)[i % 2], (case, mode, i), **args)
        for w in wants:
            finite += w["escapable"]
            steps.update(w["point_step"].tolist())
        assert lay == (0 if mode == "fused0" else 1)
    assert finite > 100 and len(steps & {1, 2, 3, 4}) >= 2, (finite, steps)


def test_points_are_the_agents_of_the_handle():
    import torch
    import _agents_worlds as agw
    from simfire_amd.engine import FireEngine
    case = "24x40_k5_u1_att"
    c = agw.CASES[case]
    kw, R8, E, inits, starts = agw.make_world(case)
    b = FireEngine(n_envs=E, **kw)
    b.set_rtable(R8)
    b.reset(inits)
    b.agents_create(c["K"], inits, n_updates=1)
    b.agents_place(list(range(E)), starts)
    rng = np.random.default_rng(3202)
    H, W = kw["shape"]
    tg = np.zeros((H, W), dtype=np.uint8)
    tg[:, W - 1] = 1
    for t in range(4):
        b.agents_step(torch.from_numpy(rng.integers(0, 20, size=(E, c["K"])).astype(np.int32)).cuda())
        hz = _horizon(b)
        rate = hz / 20
        mins = b.travel(max_minutes=float(np.float32(hz)), plane=True)["minutes"]
        r = b.escape(mins, targets=_dev(tg), points=b.agents_device(), step=True, plane=True, summary=True, horizon_minutes=hz, minutes_per_move=rate)
        pos = b.agents_device().cpu().numpy()
        maps = b.fire_maps()
        for e in range(E):
            want = eo.answer(maps[e], mins[e].cpu().numpy(), 0, 1, 4, None, tg, pos[e], rate, 0.0, hz)
            assert (r["slack"][e].cpu().numpy() == want["slack"]).all(), (t, e)
            assert r["point_slack"][e].tolist() == want["point_slack"].tolist() and r["point_step"][e].tolist() == want["point_step"].tolist(), (t, e)


# ---------------------------------------------------------------------------------------------- 3. the passes form, the move bound
def _rooms(H, W, rng):
    """A sparse map for a large grid: corridors every 24 rows and 40 columns (they cross every band and word boundary) and a few
    targets on them; everything else wall, so that the oracle's heap stays small."""
    m = np.full((H, W), 3, dtype=np.uint8)
    m[8::24, :] = 0
    m[:, 5::40] = 0
    ys, xs = np.nonzero(m == 0)
    pick = rng.choice(len(ys), size=60, replace=False)
    m[ys[pick], xs[pick]] = 2
    return m


@pytest.mark.parametrize("mode", ["fused0", "run"])
def test_more_bands_than_threads(mode):
    """977 x 1030: 62 band rows x 17 words = 1054 bands - the kernel that walks the bands in passes over the scratch planes.  A
    horizon of 64 moves; one environment of scratch gives the same bits as the default budget."""
    H, W = 977, 1030
    kw, R8 = rw.make_scene_world(H, W, True)
    b = _engine(kw, 2, R8, mode)
    from simfire_amd import escape
    assert b.escape_scratch_bytes() == escape.scratch_need(H, W) == (1054 * (16 * 24 + 40) + 255) // 256 * 256 + (4 * H * W + 255) // 256 * 256 + 262400
    b.reset(np.zeros((2, 2), dtype=np.int32))
    rng = np.random.default_rng(3203)
    for e in range(2):
        b.load_fire_map(e, _rooms(H, W, rng))
    if mode == "run":
        b.step(1)
    mins = rng.integers(0, 64, size=(2, H, W)).astype(np.float32)
    mins[rng.random((2, H, W)) < 0.3] = np.inf
    mins[:, H - 1, :] = 5
    pts = np.stack([rng.integers(-2, W + 2, size=(2, 40)), rng.integers(-2, H + 2, size=(2, 40)), rng.integers(0, 3, size=(2, 40))], axis=-1).astype(np.int32)
    pts[:, 0] = (W - 1, H - 1, 1)
    pts[:, 1] = (5, 8, 1)
    for conn, flag in ((4, False), (8, True)):
        r, maps, lay = _ask(b, mins, BURNED, UNBURNED, conn, points=pts, flag=flag)
        wants = _same(r, maps, mins, range(2), BURNED, UNBURNED, conn, (mode, conn), points=pts, flag=flag)
        assert lay == (1 if mode == "run" else 0) and all(w["escapable"] > 100 and w["lost"] > 0 for w in wants)
        one, _, _ = _ask(b, mins, BURNED, UNBURNED, conn, points=pts, flag=flag, scratch_bytes=b.escape_scratch_bytes())
        assert all((one[k] == r[k]).all() for k in r)


def test_largest_move_bound():
    """32768 moves on a tiny grid: deadlines at both ends of the range, most buckets empty - the search jumps between them."""
    H, W = 9, 40
    kw, R8 = rw.make_scene_world(H, W, True)
    b = _engine(kw, 1, R8, "fused0")
    b.reset(np.zeros((1, 2), dtype=np.int32))
    m = np.full((H, W), 3, dtype=np.uint8)
    m[1, 0] = 2
    m[1, 1:W] = 0
    b.load_fire_map(0, m)
    mins = np.full((1, H, W), 5.0, dtype=np.float32)
    mins[0, 1, 1:W] = np.linspace(32767.5, 40.0, W - 1).astype(np.float32)
    mins[0, 1, 7] = 32768.0                                   # the horizon itself: NEVER
    pts = np.array([[[W - 1, 1, 1], [3, 1, 1], [7, 1, 1], [7, 2, 1]]], dtype=np.int32)
    r, maps, _ = _ask(b, mins, BURNED, UNBURNED, points=pts, horizon=32768.0)
    want = _same(r, maps, mins, [0], BURNED, UNBURNED, 4, "bound", points=pts, horizon=32768.0)[0]
    assert want["top"] == 32768 and want["slack"][1, 1] == 32767 and 0 < want["slack"][1, W - 1] < 40
    with pytest.raises(ValueError, match="moves away"):
        b.escape(_dev(mins), target=BURNED, plane=True, horizon_minutes=32768.5)


# ---------------------------------------------------------------------------------------------- 4. lists, chunks, many environments
@pytest.mark.parametrize("mode", ["run", "fused0"])
def test_lists_and_chunks(mode):
    import torch
    kw, R8, E, inits = aw.make_world("24x40")
    b = _engine(kw, E, R8, mode)
    H, W = kw["shape"]
    need = b.escape_scratch_bytes()
    b.reset(inits)
    b.step(7)
    b.apply_mitigation(rw.line_rows(1, E, H, W, inits))
    b.step(2)
    hz = _horizon(b)
    rate = hz / 50
    mins = b.travel(max_minutes=float(np.float32(hz)), plane=True)["minutes"]
    tg = np.zeros((H, W), dtype=np.uint8)
    tg[H - 1, :] = 1
    mem0 = b.memory_bytes()
    kwargs = dict(targets=_dev(tg), plane=True, summary=True, horizon_minutes=hz, minutes_per_move=rate)
    one = b.escape(mins, scratch_bytes=need, **kwargs)        # one environment per chunk: E chunks
    assert b.memory_bytes() - mem0 == need
    full = b.escape(mins, **kwargs)
    assert b.memory_bytes() - mem0 == E * need
    for name in full:
        assert torch.equal(one[name], full[name]), name      # chunking changes no bit
    pts = np.random.default_rng(3204).integers(0, 24, size=(7, 5, 3)).astype(np.int32)
    host = mins.cpu().numpy()
    for envs in ([e for e in reversed(range(E))], [0, E - 1, 0, 0, 2, E - 1, 2], [1, 3], [2]):
        mm = host[envs]
        p = pts[:len(envs)]
        base, maps, _ = _ask(b, mm, (), UNBURNED, 4, envs=envs, targets=tg, points=p, horizon=hz, per_move=rate)
        _same(base, maps, mm, envs, (), UNBURNED, 4, (mode, envs), targets=tg, points=p, horizon=hz, per_move=rate)
        for scratch in (need, 2 * need + 7):
            got, _, _ = _ask(b, mm, (), UNBURNED, 4, envs=envs, targets=tg, points=p, horizon=hz, per_move=rate, scratch_bytes=scratch)
            for name in base:
                assert (got[name] == base[name]).all(), (mode, envs, scratch, name)
    with pytest.raises(ValueError, match="scratch_bytes"):
        b.escape(mins, scratch_bytes=need - 1, **kwargs)
    assert b.escape(mins[:0], envs=[], **kwargs)["slack"].shape == (0, H, W)


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
    hz = _horizon(b)
    rate = hz / 60
    mins = b.travel(max_minutes=float(np.float32(hz)), plane=True)["minutes"]
    tg = np.zeros((64, 64), dtype=np.uint8)
    tg[:, 0] = tg[:, 63] = 1
    r, maps, _ = _ask(b, mins, (), UNBURNED, 8, targets=tg, horizon=hz, per_move=rate, margin=2 * rate)
    wants = _same(r, maps, mins.cpu().numpy(), range(E), (), UNBURNED, 8, "many", targets=tg, horizon=hz, per_move=rate, margin=2 * rate)
    assert len({(w["escapable"], w["lost"]) for w in wants}) > 8


# ---------------------------------------------------------------------------------------------- 5. reads only
@pytest.mark.parametrize("mode", ["run", "fused0"])
def test_reads_only(mode):
    """The same rollout on two handles, arrival recording and a value plane on, one of them with escape calls between its step
    calls: maps, burn amounts, status rows, elapsed times, arrival planes, damage and the ``fire_map_delta`` sequence are the same."""
    import torch
    kw, R8, E, inits = aw.make_world("24x40")
    H, W = kw["shape"]
    a, b = _engine(kw, E, R8, mode), _engine(kw, E, R8, mode)
    rng = np.random.default_rng(3205)
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
                mins = torch.from_numpy(rng.integers(0, 30, size=(E, H, W)).astype(np.float32)).cuda()
                for call in (lambda: h.escape(mins, BURNED, plane=True, summary=True, horizon_minutes=64.0),
                             lambda: h.escape(mins, points=pts, step=True, passable=pas, targets=tgs, horizon_minutes=20.0, unreached_safe=True),
                             lambda: h.escape(mins[:2], connectivity=8, envs=[E - 1, 0], targets=tgs, plane=True, horizon_minutes=64.0,
                                              scratch_bytes=h.escape_scratch_bytes())):
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
    kw, R8, E, inits = aw.make_world("24x40")
    b = _engine(kw, E, R8, "run")
    H, W = kw["shape"]
    L, h = b._L, b._h
    need = b.escape_scratch_bytes()
    top = torch.full((E,), -7, dtype=torch.int32, device="cuda")
    ps = torch.full((E, 3), -7, dtype=torch.int32, device="cuda")
    st = torch.full((E, 3), -7, dtype=torch.int32, device="cuda")
    pts = torch.zeros((E, 3, 3), dtype=torch.int32, device="cuda")
    tg = torch.ones((H, W), dtype=torch.uint8, device="cuda")
    mins = torch.ones((E, H, W), dtype=torch.float32, device="cuda")
    all_envs = np.arange(E, dtype=np.int32)

    def rc(n=E, envs=all_envs, reserved=(0, 0), outs=None, **fields):
        p = _lib.SfEscapeParams(**dict(dict(target_mask=4, through_mask=1, minutes=mins.data_ptr(), minutes_per_move=1.0, horizon_minutes=64.0), **fields))
        p.reserved[0], p.reserved[1] = reserved
        o = _lib.SfEscapeOut(**(dict(top=top.data_ptr()) if outs is None else outs))
        e = None if envs is None else np.ascontiguousarray(envs, dtype=np.int32)
        return L.sf_escape(h, C.byref(p), n, None if e is None else e.ctypes.data_as(C.c_void_p), C.byref(o))

    assert rc() == _lib.SF_ESTATE                             # before reset
    assert b"sf_reset" in L.sf_last_error()
    b.reset(inits)
    b.step(3)
    nan, inf = float("nan"), float("inf")
    bad = [dict(target_mask=0), dict(target_mask=-1), dict(target_mask=64), dict(through_mask=0), dict(through_mask=64),
           dict(target_mask=64, targets=tg.data_ptr()), dict(connectivity=6), dict(connectivity=-1), dict(flags=2), dict(flags=-1),
           dict(k=-1), dict(k=257, points=pts.data_ptr()), dict(k=3), dict(points=pts.data_ptr()),
           dict(outs=dict(top=top.data_ptr(), point_slack=ps.data_ptr())), dict(outs=dict(point_step=ps.data_ptr())),
           dict(outs=dict()), dict(outs=dict(top=top.data_ptr() + 2)), dict(outs=dict(slack=top.data_ptr() + 1)), dict(minutes=mins.data_ptr() + 2),
           dict(k=3, points=pts.data_ptr(), outs=dict(point_slack=ps.data_ptr() + 1)),
           dict(minutes_per_move=0.0), dict(minutes_per_move=-1.0), dict(minutes_per_move=nan), dict(minutes_per_move=inf),
           dict(margin_minutes=-0.5), dict(margin_minutes=nan), dict(margin_minutes=inf),
           dict(horizon_minutes=0.0), dict(horizon_minutes=nan), dict(horizon_minutes=inf),
           dict(horizon_minutes=32769.0), dict(horizon_minutes=64.0, minutes_per_move=0.001), dict(minutes=None),
           dict(reserved=(1, 0)), dict(reserved=(0, 1)),
           dict(envs=[0, E]), dict(envs=[-1, 0], n=2), dict(scratch_bytes=need - 1), dict(scratch_bytes=1), dict(scratch_bytes=-1),
           dict(n=-1), dict(envs=None)]
    for kwargs in bad:
        kwargs = dict(kwargs)
        if "envs" in kwargs and kwargs["envs"] is not None and "n" not in kwargs:
            kwargs["n"] = len(kwargs["envs"])
        assert rc(**kwargs) == _lib.SF_EINVAL, kwargs
        assert b"sf_escape" in L.sf_last_error(), kwargs
    # the documented order: the doubles before the move bound before the minutes
    assert rc(minutes=None, horizon_minutes=nan) == _lib.SF_EINVAL and b"horizon_minutes" in L.sf_last_error()
    assert rc(minutes=None, horizon_minutes=40000.0) == _lib.SF_EINVAL and b"SF_ESCAPE_MAX_MOVES" in L.sf_last_error()
    assert rc(minutes=None, outs=dict()) == _lib.SF_EINVAL and b"every output" in L.sf_last_error()
    b.sync()
    assert (top == -7).all() and (ps == -7).all()             # nothing was enqueued
    assert rc(k=3, points=pts.data_ptr(), connectivity=8, outs=dict(point_slack=ps.data_ptr(), point_step=st.data_ptr())) == _lib.SF_OK
    assert rc(n=0) == _lib.SF_OK
    assert rc(target_mask=0, targets=tg.data_ptr(), horizon_minutes=32768.0) == _lib.SF_OK
    b.sync()
    assert (ps.cpu().numpy() == -2).all() and (st.cpu().numpy() == -1).all() and (top.cpu().numpy() == 0).all()      # (id 0: padding; every cell a target)
    host = mins.cpu().numpy()
    r, maps, _ = _ask(b, host, BURNED, UNBURNED, 4)
    _same(r, maps, host, range(E), BURNED, UNBURNED, 4, "after the errors")
    for kwargs in (dict(points=pts[:, :, :2]), dict(points=pts.cpu()), dict(passable=torch.ones((H, W), dtype=torch.float32, device="cuda")),
                   dict(targets=torch.ones((H, W + 1), dtype=torch.uint8, device="cuda")), dict(minutes=mins[:, :, 1:]), dict(minutes=mins.double()),
                   dict(minutes=mins[:2]), dict(horizon_minutes=None), dict(margin_minutes=-1.0), dict(minutes_per_move=0), dict(step=True),
                   dict(unreached_safe=1), dict(target=())):
        kwargs = dict(dict(minutes=mins, target=BURNED, horizon_minutes=64.0, plane=True), **kwargs)
        with pytest.raises(ValueError, match="escape"):
            b.escape(kwargs.pop("minutes"), **kwargs)


# ---------------------------------------------------------------------------------------------- 7. BatchedFireEnv and the simulation classes
def _config_24x40():
    import yaml
    from simfire_amd.config import Config
    y = yaml.safe_load(open(os.path.join(CFG, "functional_config.yml")))
    y["area"]["screen_size"] = [24, 40]
    y["terrain"]["topography"]["functional"]["function"] = "flat"
    y["simulation"]["headless"] = True
    return Config(config_dict=y)


def test_batched_fire_env_escape():
    """``info["escape_slack"]`` and ``info["escape_move"]`` equal a direct ``escape_routes`` call on the state the observation
    shows, every tick, once through an auto-reset tick; without the option ``info`` has the old keys only."""
    import torch
    import simfire_amd
    from simfire_amd.simulation import BatchedFireSimulation
    cfg = _config_24x40()
    H, W = cfg.area.screen_size
    E, K = 3, 4
    ign = np.array([(10, 10), (W - 5, 7), (3, H - 4)], dtype=np.int32)
    starts = np.array([(W - 1, 16), (W - 2, 11), (12, 12), (5, 9)], dtype=np.int32)
    tg = np.zeros((H, W), dtype=np.uint8)
    tg[H - 1, :] = 1
    option = dict(targets=_dev(tg), horizon_minutes=90.0, margin_minutes=2.0)
    sim = BatchedFireSimulation(cfg, E, ignitions=ign)
    env = simfire_amd.BatchedFireEnv(sim, K, starts, n_updates=1, max_ticks=4, escape=option)
    plain = simfire_amd.BatchedFireEnv(BatchedFireSimulation(cfg, E, ignitions=ign), K, starts, n_updates=1, max_ticks=4)
    env.reset()
    plain.reset()
    actions = torch.zeros((E, K), dtype=torch.int32, device="cuda")
    restarted = False
    for t in range(6):
        obs, reward, done, info = env.step(actions)
        obs_p, reward_p, done_p, info_p = plain.step(actions)
        assert set(info) == set(info_p) | {"escape_slack", "escape_move"} and torch.equal(obs, obs_p) and torch.equal(reward, reward_p)
        assert info["escape_slack"].dtype == torch.int32 and info["escape_slack"].shape == (E, K) and info["escape_move"].shape == (E, K)
        direct = sim.escape_routes(agents=True, step=True, **option)
        assert torch.equal(direct["point_slack"], info["escape_slack"]) and torch.equal(direct["point_step"], info["escape_move"]), t
        restarted = restarted or bool(done.all().item())
        actions = torch.where((info["escape_slack"] >= 0) & (info["escape_slack"] < 40), info["escape_move"], torch.zeros_like(info["escape_move"]))
    assert restarted
    with pytest.raises(ValueError, match="escape"):
        simfire_amd.BatchedFireEnv(sim, K, starts, escape=dict(radius=3))
    with pytest.raises(ValueError, match="horizon_minutes"):
        simfire_amd.BatchedFireEnv(sim, K, starts, escape=dict(targets=_dev(tg)))


def test_simulation_classes_escape_routes():
    import torch
    from simfire_amd.config import Config
    from simfire_amd.enums import BurnStatus
    from simfire_amd.simulation import BatchedFireSimulation, FireSimulation
    sim = FireSimulation(Config(os.path.join(CFG, "test_config_flat_simple.yml")))
    sim.run(2)
    m = np.asarray(sim.fire_map)
    H, W = m.shape
    tg = np.zeros((H, W), dtype=np.uint8)
    tg[:, W - 1] = 1
    t0 = sim.time_to_fire()
    rate = float(sim._engine.params.update_rate)
    horizon = float(np.float32(min(np.percentile(t0[np.isfinite(t0) & (t0 > 0)], 50), 30000 * rate)))
    mins = sim.time_to_fire(max_minutes=horizon)
    sl = sim.escape_routes(targets=_dev(tg), horizon_minutes=horizon)
    want = eo.answer(m, mins, 0, 1, 4, None, tg, None, rate, 0.0, horizon)
    assert sl.dtype == np.int32 and sl.shape == m.shape and (sl == want["slack"]).all()
    assert (sl != eo.BLOCKED).sum() > 0 and want["top"] > 0
    # a host edit closes the only corridor: a wall of line in front of the targets
    sim.fire_map[:, W - 2] = int(BurnStatus.FIRELINE)
    sl = sim.escape_routes(targets=_dev(tg), horizon_minutes=horizon)
    m = np.asarray(sim.fire_map)
    want = eo.answer(m, sim.time_to_fire(max_minutes=horizon), 0, 1, 4, None, tg, None, rate, 0.0, horizon)
    assert (sl == want["slack"]).all() and (sl[:, W - 2] == eo.BLOCKED).all() and (sl[:, W - 1] == eo.SAFE).all()
    assert not ((sl[:, :W - 2] >= 0) & (sl[:, :W - 2] < eo.SAFE)).any() and (sl[:, :W - 2] == eo.LOST).sum() > 0
    given = sim.escape_routes(targets=_dev(tg), horizon_minutes=horizon, minutes=torch.full((H, W), 7.0, device="cuda"), minutes_per_move=1.0)
    assert (given == eo.answer(m, np.full((H, W), 7.0, np.float32), 0, 1, 4, None, tg, None, 1.0, 0.0, horizon)["slack"]).all()
    bat = BatchedFireSimulation(_config_24x40(), 3)
    bat.run(4, return_maps=False)
    tg = np.zeros((24, 40), dtype=np.uint8)
    tg[0, :] = 1
    dev = bat.escape_routes(targets=_dev(tg), horizon_minutes=120.0, envs=[2, 0], plane=True)
    host = bat.escape_routes(targets=_dev(tg), horizon_minutes=120.0, envs=[2, 0], plane=True, device=False)
    assert dev["slack"].is_cuda and set(dev) == {"slack"} | set(SUMMARY) and all((dev[k].cpu().numpy() == host[k]).all() for k in dev)
    mins = bat.time_to_fire(max_minutes=120.0, envs=[2, 0], device=False)["minutes"]
    rate = float(bat._engine.params.update_rate)
    for i, e in enumerate((2, 0)):
        want = eo.answer(bat.fire_map(e), mins[i], 0, 1, 4, None, tg, None, rate, 0.0, 120.0)
        assert (host["slack"][i] == want["slack"]).all() and all(host[k][i] == want[k] for k in SUMMARY)
    pts = torch.tensor([[[0, 0, 1], [50, 0, 1]], [[1, 1, 0], [2, 2, 3]]], dtype=torch.int32, device="cuda")
    got = bat.escape_routes(targets=_dev(tg), horizon_minutes=120.0, envs=[2, 0], agents=pts, step=True, device=False)
    assert got["point_slack"].tolist() == [[eo.SAFE, -2], [-2, int(host["slack"][1][2, 2])]] and got["point_step"][0].tolist() == [0, -1]
