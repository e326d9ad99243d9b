"""Fire behaviour on the GPU (``sf_behavior``).  The engine computes FIRST; the oracle
(``tests/_behavior_oracle.py``) is then fed with ``fire_maps()``, the layers and the handle's own table from ``sf_get_rtable_env``,
fetched afterwards.  Equality for ``head``, ``ros``, ``workable``, the summary, the point form and masked-out cells; relative 1e-5
of the oracle's value - the parity bound of the float32 Rothermel chain - for ``hpa``, ``intensity`` and ``flame_length``, exact 0
where the oracle is 0, no cell left out.  Run with ``pytest -m gpu -s`` to see the largest deviation of every test."""
import ctypes as C
import os

import numpy as np
import pytest

import _behavior_oracle as bo
import _behavior_worlds as bw

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tests", "golden", "configs")
ALL = ("hpa", "ros", "intensity", "flame_length", "head")
RTOL = 1e-5
WORST = {"hpa": 0.0, "intensity": 0.0, "flame_length": 0.0}


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ask(eng, envs=None, status=None, summary=("BURNING",), flame_limit=None, edges=None, points=None, planes=ALL):
    """Every output of ``behavior`` as NumPy arrays; the call neither converts the cell plane nor changes the launch kind."""
    lay, kind = eng.cell_layout(), eng.last_launch_kind()
    r = eng.behavior(envs=envs, status=status, summary=summary, flame_limit=flame_limit, edges=edges, points=_dev(points), planes=planes,
                     workable=flame_limit is not None, stats=True)
    assert (eng.cell_layout(), eng.last_launch_kind()) == (lay, kind)
    assert all(v.is_cuda for v in r.values())
    return {k: v.cpu().numpy() for k, v in r.items()}, lay


def _close(got, want, name, tag):
    """``got`` within RTOL of the oracle's value in every cell, exactly 0 where the oracle is 0."""
    assert got.dtype == np.float32 and got.shape == want.shape, (tag, name, got.dtype, got.shape)
    zero = want == 0
    assert (got[zero] == 0).all(), (tag, name, "not 0 where the oracle is 0", int((got[zero] != 0).sum()))
    if (~zero).any():
        rel = np.abs(got[~zero].astype(np.float64) - want[~zero].astype(np.float64)) / np.abs(want[~zero].astype(np.float64))
        WORST[name] = max(WORST[name], float(rel.max()))
        assert rel.max() <= RTOL, (tag, name, float(rel.max()), int((rel > RTOL).sum()))


def _check(eng, r, envs, layers_of, per_env=True, status=None, summary=("BURNING",), flame_limit=None, edges=None, points=None, tag=""):
    """Every output of a call that asked for ALL planes against the oracle.  The summary and the point form are held against the
    device's OWN unmasked planes (a second call without ``status``) and the fetched status.  Returns the maps."""
    envs = list(range(eng.n_envs)) if envs is None else list(envs)
    n, H, W = len(envs), eng.H, eng.W
    own = r if status is None else _ask(eng, envs=envs, planes=("flame_length", "intensity"))[0]
    want, maps = bw.expect(eng, envs, layers_of, bw.mask_of(status), per_env)
    summask = bw.mask_of(summary)
    for name in ALL:
        assert r[name].shape == (n, H, W), (tag, name, r[name].shape)
    assert r["head"].dtype == np.int8 and r["classes"].shape == (n, 5) and r["classes"].dtype == np.int32 and r["max_flame"].dtype == np.float32
    for i, e in enumerate(envs):
        full, m = want[i]
        t = (tag, i, e)
        assert (r["head"][i] == m["head"]).all(), (t, "head", int((r["head"][i] != m["head"]).sum()))
        assert (r["ros"][i] == m["ros"]).all() and r["ros"].dtype == np.float32, (t, "ros")
        for name in ("hpa", "intensity", "flame_length"):
            _close(r[name][i], m[name], name, t)
        hidden = ~bo.in_mask(maps[e], bw.mask_of(status))
        assert all((r[name][i][hidden] == (-1 if name == "head" else 0)).all() for name in ALL), (t, "a hidden cell shows something")
        if flame_limit is not None:
            assert r["workable"].dtype == np.uint8 and (r["workable"][i] == bo.workable(r["flame_length"][i], flame_limit)).all(), (t, "workable")
        mf, mi, cls = bo.summary(own["flame_length"][i], own["intensity"][i], maps[e], summask, bo.DEFAULT_EDGES if edges is None else edges)
        assert r["max_flame"][i] == mf and r["max_intensity"][i] == mi, (t, float(r["max_flame"][i]), float(mf), float(r["max_intensity"][i]), float(mi))
        assert r["classes"][i].tolist() == cls.tolist() and int(cls.sum()) == int(bo.in_mask(maps[e], summask).sum()), (t, r["classes"][i].tolist(), cls.tolist())
        if points is not None:
            wantp = bo.point_flame(own["flame_length"][i], maps[e], summask, points[i])
            assert r["point_flame"][i].tolist() == wantp.tolist(), (t, r["point_flame"][i].tolist(), wantp.tolist())
    return maps


def _episode(eng, inits, H, W):
    """An episode a few updates old with control lines (three updates: the ignition cell of max_fire_duration = 4 still burns)."""
    eng.reset(inits)
    eng.step(2)
    eng.apply_mitigation(bw.line_rows(eng.n_envs, H, W, inits))
    eng.step(1)


def _report(tag):
    print("largest relative deviation from the oracle (%s):" % tag, {k: "%.3g" % v for k, v in WORST.items()})


# ---------------------------------------------------------------------------------------------- 1. shapes, layouts, lists
@pytest.mark.parametrize("shape", bw.SHAPES, ids=["%dx%d" % s for s in bw.SHAPES])
@pytest.mark.parametrize("mode", ["fused0", "run"])
def test_scenes(shape, mode):
    """Per-environment terrain with different fuels per environment and an unburnable block, an episode a few updates old with
    control lines, both cell layouts (asserted): every plane, ``workable``, the summary and the point form - points on the border,
    in a corner, off the grid, ``id <= 0``, duplicates, on the fire - in order, and for a list with repeats under both masks."""
    H, W = shape
    E = 3
    layers = bw.terrain(2500 + H, H, W, E)
    eng = bw.engine(H, W, layers, mode=mode)
    inits = bw.ignitions(H, W, E)
    _episode(eng, inits, H, W)
    pts = bw.points_near(inits, H, W)
    r, lay = _ask(eng, flame_limit=4.0, points=pts)
    assert lay == (1 if mode == "run" else 0)
    maps = _check(eng, r, None, lambda e: layers[e], flame_limit=4.0, points=pts, tag=(shape, mode, "all"))
    assert (maps == 1).any() and (maps >= 3).any() and r["max_flame"].max() > 0 and (r["point_flame"] > 0).any() and (r["point_flame"] == -1).any()
    dead = np.asarray(layers[0][0]) == 0
    assert dead.sum() == 9 and not r["flame_length"][0][dead].any() and not r["hpa"][0][dead].any() and (r["head"][0][dead] == -1).all()
    assert 0 < r["workable"].sum() and (r["flame_length"] > 0).any()
    envs = [2, 0, 2, 1]
    status, summary, edges = ("BURNING", "BURNED"), ("BURNING", "BURNED", "FIRELINE"), (0.5, 1.5, 3.0, 6.0)
    r, lay = _ask(eng, envs=envs, status=status, summary=summary, flame_limit=1.5, edges=edges, points=pts[envs])
    assert lay == (1 if mode == "run" else 0)
    _check(eng, r, envs, lambda e: layers[e], status=status, summary=summary, flame_limit=1.5, edges=edges, points=pts[envs],
           tag=(shape, mode, "masked"))
    assert (r["flame_length"][0] == r["flame_length"][2]).all() and (r["classes"][0] == r["classes"][2]).all()      # the repeat
    _report("scenes %dx%d %s" % (H, W, mode))


def test_shared_terrain_and_a_list_longer_than_the_grid():
    """One table for all, more environments than CUs at 9 x 9 (cu + 8 of them, each its own fire), then a shuffled list with repeats."""
    import torch
    H, W = 9, 9
    E = torch.cuda.get_device_properties(0).multi_processor_count + 8
    layers = bw.terrain(2511, H, W, 1)
    eng = bw.engine(H, W, layers, per_env=False, n_envs=E, mode="run")
    rng = np.random.default_rng(2512)
    inits = np.stack([rng.integers(0, W, size=E), rng.integers(0, H, size=E)], axis=1).astype(np.int32)
    eng.reset(inits)
    eng.step(2)
    pts = np.stack([bw.points(H, W, e) for e in range(E)])
    r, lay = _ask(eng, flame_limit=2.0, points=pts)
    assert lay == 1
    _check(eng, r, None, lambda e: layers[0], per_env=False, flame_limit=2.0, points=pts, tag="shared, all")
    assert len({tuple(c) for c in r["classes"].tolist()}) > 4
    envs = rng.integers(0, E, size=E + 40).tolist()
    r, _ = _ask(eng, envs=envs, status=("UNBURNED", "BURNING"), points=pts[envs])
    _check(eng, r, envs, lambda e: layers[0], per_env=False, status=("UNBURNED", "BURNING"), points=pts[envs], tag="shared, list")
    _report("shared terrain")


def test_an_environment_with_nothing_burning():
    """Every summary value of an environment without a BURNING cell is 0, and so is the point form on the grid."""
    H, W = 9, 9
    layers = bw.terrain(2513, H, W, 2)
    eng = bw.engine(H, W, layers, mode="fused0")
    eng.reset(np.array([(4, 4), (2, 6)], dtype=np.int32))
    eng.step(2)
    eng.load_fire_map(1, np.zeros((H, W), dtype=np.uint8))
    pts = np.stack([bw.points(H, W, e) for e in range(2)])
    r, _ = _ask(eng, points=pts)
    _check(eng, r, None, lambda e: layers[e], points=pts, tag="nothing burning")
    assert r["max_flame"][1] == 0 and r["max_intensity"][1] == 0 and not r["classes"][1].any() and r["max_flame"][0] > 0
    assert set(r["point_flame"][1].tolist()) == {0.0, -1.0} and (r["flame_length"][1] > 0).any()


# ---------------------------------------------------------------------------------------------- 2. wind and staleness
def test_wind_changes_everything_but_the_heat():
    """After ``set_wind`` on some environments their ``ros``, ``intensity``, ``flame_length`` and ``head`` change and equal the oracle
    fed with the new table; ``hpa`` is bit-identical, and the heat cache was not rebuilt (the lab's count)."""
    H, W, E = 33, 17, 4
    layers = bw.terrain(2520, H, W, E)
    eng = bw.engine(H, W, layers, mode="run")
    _episode(eng, bw.ignitions(H, W, E), H, W)
    assert eng.behavior_builds() == 0
    r0, _ = _ask(eng)
    _check(eng, r0, None, lambda e: layers[e], tag="before the wind")
    assert eng.behavior_builds() == E
    eng.set_wind([2400.0, 0.0], [275.0, 10.0], envs=[3, 1])
    r1, _ = _ask(eng)
    assert eng.behavior_builds() == E
    _check(eng, r1, None, lambda e: layers[e], tag="after the wind")
    assert (r1["hpa"] == r0["hpa"]).all()
    for e in (1, 3):
        assert all((r1[k][e] != r0[k][e]).any() for k in ("ros", "intensity", "flame_length", "head")), e
    for e in (0, 2):
        assert all((r1[k][e] == r0[k][e]).all() for k in ALL), e
    _report("wind")


def test_the_heat_cache_follows_the_terrain():
    """A behaviour call, then each of ``set_layers`` for one environment, ``generate_layers``, ``copy_envs`` with the terrain and a
    restored state, then a second call that equals the oracle on the terrain as it is then; the cache rebuilds exactly the tables
    that changed."""
    H, W, E = 40, 130, 4
    layers = bw.terrain(2530, H, W, E)
    eng = bw.engine(H, W, layers, mode="fused0")
    inits = bw.ignitions(H, W, E)
    _episode(eng, inits, H, W)
    before = eng.memory_bytes()
    r, _ = _ask(eng)
    assert eng.behavior_builds() == E and eng.memory_bytes() == before + 4 * E * H * W      # the cache: 4 bytes per cell and table
    _check(eng, r, None, lambda e: layers[e], tag="first")
    first = r
    layers[2] = bw.terrain(2531, H, W, 1, codes=(3, 6, 7, 11, 12, 13))[0]
    eng.set_layers(*layers[2], env=2)
    r, _ = _ask(eng)
    _check(eng, r, None, lambda e: layers[e], tag="set_layers")
    assert eng.behavior_builds() == E + 1 and (r["hpa"][2] != first["hpa"][2]).any() and (r["hpa"][[0, 1, 3]] == first["hpa"][[0, 1, 3]]).all()
    eng.generate_layers([1], elevation=dict(seed=5, octaves=3, persistence=0.7, lacunarity=2.0, lo=100.0, hi=900.0),
                        fuel=(0.0918, 1.0, 0.15, 2784.0), wind_speed=700.0, wind_direction=120.0)
    a = eng.attribute_data(1)
    layers[1] = [a["w_0"], a["delta"], a["M_x"], a["sigma"].astype(np.float64)]
    r, _ = _ask(eng)
    _check(eng, r, None, lambda e: layers[e], tag="generate_layers")
    assert eng.behavior_builds() == E + 2 and len(np.unique(r["hpa"][1])) == 1 and r["hpa"][1][0, 0] > 0
    eng.copy_envs([2], [3], terrain=True)
    layers[3] = layers[2]
    r, _ = _ask(eng)
    _check(eng, r, None, lambda e: layers[e], tag="copy_envs")
    assert eng.behavior_builds() == E + 3 and (r["hpa"][3] == r["hpa"][2]).all() and (r["flame_length"][3] == r["flame_length"][2]).all()
    blob = eng.save_state([0])
    eng.step(4)
    eng.load_state([0], blob)
    r2, _ = _ask(eng)
    _check(eng, r2, None, lambda e: layers[e], tag="restored")
    assert eng.behavior_builds() == E + 3 and (r2["classes"][0] == r["classes"][0]).all() and (r2["flame_length"][0] == r["flame_length"][0]).all()
    _report("staleness")


# ---------------------------------------------------------------------------------------------- 3. reads only, async
@pytest.mark.parametrize("mode", ["run", "fused0"])
def test_reads_only(mode):
    """The same rollout on two handles, one with behaviour calls between its step calls: status rows, elapsed times, maps and burn
    amounts are the same."""
    H, W, E = 64, 64, 3
    layers = bw.terrain(2540, H, W, E)
    a, b = bw.engine(H, W, layers, mode=mode), bw.engine(H, W, layers, mode=mode)
    inits = bw.ignitions(H, W, E)
    pts = _dev(bw.points_near(inits, H, W))
    for h in (a, b):
        h.reset(inits)
        for i, n in enumerate((1, 2, 3, 5)):
            h.step(n)
            if h is b:
                for kw in (dict(planes=ALL, workable=True, flame_limit=4.0, stats=True), dict(planes=(), points=pts, stats=True),
                           dict(planes=("flame_length",), envs=[2, 0], status=("BURNING",))):
                    lay, kind = h.cell_layout(), h.last_launch_kind()
                    h.behavior(**kw)
                    assert (h.cell_layout(), h.last_launch_kind()) == (lay, kind), (mode, i)
                assert lay == (1 if mode == "run" else 0)
            if i == 1:
                h.apply_mitigation(bw.line_rows(E, H, W, inits))
    sa, ea = a.status()
    sb, eb = b.status()
    assert (sa == sb).all() and (ea == eb).all() and (a.fire_maps() == b.fire_maps()).all()
    for e in range(E):
        assert (a.burn(e) == b.burn(e)).all(), (mode, e)


def test_async_mode():
    """In async mode the call only enqueues; after ``sync()`` the outputs are complete: bit for bit those of the synchronous call."""
    H, W, E = 64, 64, 3
    layers = bw.terrain(2550, H, W, E)
    eng = bw.engine(H, W, layers, mode="run")
    inits = bw.ignitions(H, W, E)
    _episode(eng, inits, H, W)
    envs = [1, 1, 2, 0]
    pts = _dev(bw.points_near(inits, H, W)[envs])
    kw = dict(planes=ALL, workable=True, flame_limit=3.0, stats=True, points=pts, envs=envs)
    eng.set_async(True)
    got = eng.behavior(**kw)                                   # (the first call: the heat cache is built on the stream too)
    eng.sync()
    got = {k: v.cpu().numpy() for k, v in got.items()}
    eng.set_async(False)
    want = {k: v.cpu().numpy() for k, v in eng.behavior(**kw).items()}
    assert set(got) == set(want) == set(ALL) | {"workable", "max_flame", "max_intensity", "classes", "point_flame"}
    assert all((got[k] == want[k]).all() for k in want) and want["max_flame"].max() > 0


# ---------------------------------------------------------------------------------------------- 4. refusals
def test_refusals_through_the_raw_call():
    import torch
    from simfire_amd import _lib
    from simfire_amd.engine import FireEngine
    H, W, E = 33, 17, 3
    layers = bw.terrain(2560, H, W, E)
    eng = FireEngine((H, W), n_envs=E, per_env_terrain=True, pixel_scale=30.0, M_f=bw.M_F, particle=bw.PARTICLE)
    L, h = eng._L, eng._h
    cells = E * H * W
    flame = torch.full((cells + 64,), -7.0, dtype=torch.float32, device="cuda")         # (64 more: what lies behind the plane stays)
    work = torch.full((cells + 64,), 77, dtype=torch.uint8, device="cuda")
    head = torch.full((cells + 64,), 77, dtype=torch.int8, device="cuda")
    mf = torch.full((E,), -7.0, dtype=torch.float32, device="cuda")
    cls = torch.full((E, 5), -7, dtype=torch.int32, device="cuda")
    pf = torch.full((E, 3), -7.0, dtype=torch.float32, device="cuda")
    pts = torch.zeros((E, 3, 3), dtype=torch.int32, device="cuda")
    all_envs = np.arange(E, dtype=np.int32)

    def rc(n=E, envs=all_envs, outs=None, edges=(4.0, 8.0, 11.0, 1e30), null=(), **fields):
        p = _lib.SfBehaviorParams(**dict(dict(status_mask=0, summary_mask=2), **fields))
        for i in range(4):
            p.edges[i] = edges[i]
        o = _lib.SfBehaviorOut(**(dict(max_flame=mf.data_ptr()) if outs is None else outs))
        e = None if envs is None else np.ascontiguousarray(envs, dtype=np.int32)
        return L.sf_behavior(h, None if "params" in null else C.byref(p), None if "out" in null else C.byref(o),
                             None if e is None else e.ctypes.data_as(C.c_void_p), n)

    assert rc() == _lib.SF_ESTATE and b"sf_behavior" in L.sf_last_error()             # before layers
    for e in range(E):
        eng.set_layers(*layers[e], env=e)
    assert rc() == _lib.SF_ESTATE and b"sf_reset" in L.sf_last_error()                # before reset
    eng.reset(bw.ignitions(H, W, E))
    eng.step(2)
    nan = float("nan")
    bad = [dict(null=("params",)), dict(null=("out",)), dict(outs=dict()), dict(envs=None), dict(n=-1), dict(envs=[0, E]), dict(envs=[-1, 0]),
           dict(status_mask=64), dict(status_mask=-1), dict(summary_mask=0), dict(summary_mask=64), dict(summary_mask=-2), dict(reserved=1),
           dict(edges=(4.0, 4.0, 11.0, 1e30)), dict(edges=(8.0, 4.0, 11.0, 1e30)), dict(edges=(4.0, 8.0, 11.0, nan)), dict(edges=(nan, 8.0, 11.0, 12.0)),
           dict(flame_limit=-1.0), dict(flame_limit=nan), dict(k=-1), dict(k=257, points=pts.data_ptr(), outs=dict(point_flame=pf.data_ptr())),
           dict(k=3, outs=dict(point_flame=pf.data_ptr())), dict(points=pts.data_ptr()), dict(outs=dict(point_flame=pf.data_ptr())),
           dict(k=3, points=pts.data_ptr()), dict(outs=dict(max_flame=mf.data_ptr() + 2)), dict(outs=dict(flame_length=flame.data_ptr() + 1)),
           dict(outs=dict(classes=cls.data_ptr() + 2)), dict(k=3, points=pts.data_ptr(), outs=dict(point_flame=pf.data_ptr() + 1)),
           dict(k=3, points=pts.data_ptr() + 2, outs=dict(point_flame=pf.data_ptr()))]
    for kwargs in bad:
        kwargs = dict(kwargs)
        if kwargs.get("envs") is not None and "n" not in kwargs:
            kwargs["n"] = len(kwargs["envs"])
        assert rc(**kwargs) == _lib.SF_EINVAL, kwargs
        assert b"sf_behavior" in L.sf_last_error(), kwargs
    eng.sync()
    assert (mf == -7).all() and (cls == -7).all() and (pf == -7).all() and (flame == -7).all()       # nothing was enqueued
    assert eng.behavior_builds() == 0
    assert rc(n=0) == _lib.SF_OK
    # the call after the errors works; W % 4 != 0, the cell-by-cell path: the planes end where they end
    outs = dict(flame_length=flame.data_ptr(), workable=work.data_ptr(), head=head.data_ptr(), max_flame=mf.data_ptr(), classes=cls.data_ptr(),
                point_flame=pf.data_ptr())
    assert rc(k=3, points=pts.data_ptr(), flame_limit=2.0, outs=outs) == _lib.SF_OK
    eng.sync()
    assert (flame[cells:] == -7).all() and (work[cells:] == 77).all() and (head[cells:] == 77).all() and (pf == -1).all()      # (id 0: padding)
    want = eng.behavior(planes=("flame_length", "head"), workable=True, flame_limit=2.0, stats=True)
    assert torch.equal(flame[:cells].view(E, H, W), want["flame_length"]) and torch.equal(work[:cells].view(E, H, W), want["workable"])
    assert torch.equal(head[:cells].view(E, H, W), want["head"]) and torch.equal(mf, want["max_flame"]) and torch.equal(cls, want["classes"])
    r, _ = _ask(eng)
    _check(eng, r, None, lambda e: layers[e], tag="after the errors")
    # a table that came from sf_set_rtable has no layers to take I_R from
    eng.set_rtable(np.full((8, H, W), 3.0), env=1)
    assert rc(envs=[0, 2], n=2) == _lib.SF_OK
    raw = eng.get_rtable(0)
    other = FireEngine((H, W), n_envs=2, pixel_scale=30.0)
    other.set_rtable(raw)
    other.reset(np.array([(3, 3), (4, 4)], dtype=np.int32))
    p, o, e2 = _lib.SfBehaviorParams(summary_mask=2), _lib.SfBehaviorOut(max_flame=mf.data_ptr()), np.zeros(1, dtype=np.int32)
    for i, v in enumerate((4.0, 8.0, 11.0, 1e30)):
        p.edges[i] = v
    assert other._L.sf_behavior(other._h, C.byref(p), C.byref(o), e2.ctypes.data_as(C.c_void_p), 1) == _lib.SF_ESTATE
    assert b"sf_set_rtable" in L.sf_last_error()
    with pytest.raises(_lib.SimfireHipError, match="sf_set_rtable"):
        other.behavior()
    for kwargs in (dict(points=pts[:, :, :2]), dict(points=torch.zeros((E, 257, 3), dtype=torch.int32, device="cuda")), dict(points=pts.cpu()),
                   dict(planes=("flames",)), dict(workable=True), dict(edges=(3, 2, 1, 0))):
        with pytest.raises(ValueError, match="behavior"):
            eng.behavior(**kwargs)


# ---------------------------------------------------------------------------------------------- 5. composition
def test_workable_is_what_moves_to_takes_as_passable():
    """33 x 17, short grass with one cell of chaparral in a corridor through lines whose other end burns: with ``workable`` (flame
    limit between the two fuels' flame lengths) as ``passable`` the walker at the corridor's end cannot get to the fire
    (``WALK_FAR``); without it the answer is the corridor's length.  The plane goes from one call to the other on the device."""
    from simfire_amd.parameters import Chaparral, ShortGrass
    H, W, length = 33, 17, 12
    f = ShortGrass
    w0, de, mx, sg = (np.full((H, W), v) for v in (f.w_0, f.delta, f.M_x, f.sigma))
    hot = (2, 6)
    w0[hot], de[hot], mx[hot], sg[hot] = Chaparral.w_0, Chaparral.delta, Chaparral.M_x, Chaparral.sigma
    layers = [[w0, de, mx, sg, np.zeros((H, W)), np.full((H, W), 400.0), np.full((H, W), 90.0)]]
    eng = bw.engine(H, W, layers, per_env=False, n_envs=1, mode="fused0")
    eng.reset(np.array([(1, 2)], dtype=np.int32))
    m = np.full((H, W), bw.FL, dtype=np.uint8)
    m[2, 1] = bw.B
    m[2, 2:2 + length] = bw.U
    eng.load_fire_map(0, m)
    L = eng.behavior()["flame_length"][0].cpu().numpy()
    grass = L[2, 2:2 + length][np.arange(2, 2 + length) != hot[1]]
    assert grass.max() < L[hot] and grass.min() > 0
    limit = float((grass.max() + L[hot]) / 2)
    r = eng.behavior(planes=(), workable=True, flame_limit=limit)
    wk = r["workable"]
    assert wk.dtype.is_floating_point is False and wk.is_cuda and int(wk[0][hot].item()) == 0 and int(wk[0].sum().item()) == H * W - 1
    pts = _dev(np.array([[[2 + length, 2, 1], [4, 2, 1], [hot[1] + 1, hot[0], 1]]], dtype=np.int32))
    free = eng.walk(points=pts)["point_moves"][0].tolist()
    shut = eng.walk(points=pts, passable=wk[0])["point_moves"][0].tolist()
    assert free == [length + 1, 3, hot[1]] and shut == [eng.WALK_FAR, 3, eng.WALK_FAR], (free, shut)
    _check(eng, _ask(eng)[0], None, lambda e: layers[0], per_env=False, tag="corridor")


def _config_24x40():
    import yaml
    from simfire_amd.config import Config
    y = yaml.safe_load(open(os.path.join(CFG, "functional_config.yml")))
    y["area"]["screen_size"] = [24, 40]
    y["terrain"]["topography"]["functional"]["function"] = "flat"
    y["simulation"]["headless"] = True
    return Config(config_dict=y)


def test_batched_fire_env_behavior():
    """``info["flame_length"]`` / ``info["max_flame"]`` equal the point form and the summary of a direct call on the same state, on
    every tick and through an auto-reset tick; without the option ``info`` has today's keys."""
    import torch
    import simfire_amd
    from simfire_amd.simulation import BatchedFireSimulation
    cfg = _config_24x40()
    H, W = cfg.area.screen_size
    E, K = 3, 4
    ign = np.array([(10, 10), (W - 5, 7), (3, H - 4)], dtype=np.int32)
    starts = np.array([[(11, 10), (9, 11), (0, 0), (W - 1, H - 1)], [(W - 5, 8), (W - 6, 7), (5, 5), (W - 4, 6)], [(3, H - 4), (4, H - 5), (2, H - 3), (20, 2)]],
                      dtype=np.int32)
    sim = BatchedFireSimulation(cfg, E, ignitions=ign)
    env = simfire_amd.BatchedFireEnv(sim, K, starts, n_updates=1, max_ticks=4, behavior=dict(flame_limit=4.0, summary=("BURNING", "BURNED")))
    plain = simfire_amd.BatchedFireEnv(BatchedFireSimulation(cfg, E, ignitions=ign), K, starts, n_updates=1, max_ticks=4)
    env.reset()
    plain.reset()
    rng = np.random.default_rng(2570)
    restarted, seen = False, 0.0
    for t in range(6):
        actions = torch.from_numpy(rng.integers(0, 5, size=(E, K)).astype(np.int32)).cuda()
        obs, reward, done, info = env.step(actions)
        obs_p, reward_p, done_p, info_p = plain.step(actions)
        assert set(info) == set(info_p) | {"flame_length", "max_flame"} and torch.equal(obs, obs_p) and torch.equal(reward, reward_p)
        direct = sim.fire_behavior(summary=("BURNING", "BURNED"), agents=True, planes=())
        assert info["flame_length"].dtype == torch.float32 and info["flame_length"].shape == (E, K) and info["max_flame"].shape == (E,)
        assert torch.equal(info["flame_length"], direct["point_flame"]) and torch.equal(info["max_flame"], direct["max_flame"]), t
        restarted = restarted or bool(done.all().item())
        seen = max(seen, float(info["flame_length"].max().item()))
    assert restarted and seen > 0
    with pytest.raises(ValueError, match="behavior"):
        simfire_amd.BatchedFireEnv(sim, K, starts, behavior=dict(radius=3))


def test_simulation_classes_fire_behavior():
    from simfire_amd.config import Config
    from simfire_amd.enums import BurnStatus
    from simfire_amd.simulation import BatchedFireSimulation, FireSimulation
    sim = FireSimulation(Config(os.path.join(CFG, "test_config_flat_simple.yml")))
    sim.run(2)
    r = sim.fire_behavior(planes=ALL, flame_limit=4.0)
    m = np.asarray(sim.fire_map)
    assert set(r) == set(ALL) | {"workable"} and all(v.shape == m.shape for v in r.values()) and r["flame_length"].dtype == np.float32
    c = bo.cells(sim._engine.get_rtable(0), r["hpa"])
    assert (r["head"] == c["head"]).all() and (r["ros"] == c["ros"]).all() and np.allclose(r["flame_length"], c["flame_length"], rtol=RTOL, atol=0)
    assert (r["workable"] == bo.workable(r["flame_length"], 4.0)).all() and r["flame_length"].max() > 0
    y, x = np.argwhere(m == 0)[0]
    sim.fire_map[y, x] = int(BurnStatus.FIRELINE)                          # a host edit is pushed first
    only = sim.fire_behavior(status=("FIRELINE",))["flame_length"]
    assert only[y, x] == r["flame_length"][y, x] and (only != 0).sum() <= 1
    bat = BatchedFireSimulation(_config_24x40(), 3)
    bat.run(4, return_maps=False)
    dev = bat.fire_behavior(envs=[2, 0], flame_limit=8.0)
    host = bat.fire_behavior(envs=[2, 0], flame_limit=8.0, device=False)
    assert dev["flame_length"].is_cuda and set(dev) == {"flame_length", "workable", "max_flame", "max_intensity", "classes"}
    assert all((dev[k].cpu().numpy() == host[k]).all() for k in dev)
    for i, e in enumerate((2, 0)):
        sel = bat.fire_map(e) == 1
        assert host["classes"][i].sum() == sel.sum() and host["max_flame"][i] == (host["flame_length"][i][sel].max() if sel.any() else 0)
