"""Distance fields on the GPU (``sf_distance``).  The yardstick is ``tests/_dist_oracle.py`` - the literal minimum
over the selected cells - fed with the maps the older getters return.  ``distance`` is always called FIRST and the maps are fetched
afterwards (a getter may convert the current plane); every comparison is equality, the float output on its raw bits.  Run with
``pytest -m gpu``."""
import ctypes as C
import os

import numpy as np
import pytest

import _arrival_worlds as aw
import _dist_oracle as do
import _dist_worlds as dw

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tests", "golden", "configs")


def _engine(kw, E, R8, mode):
    from simfire_amd.engine import FireEngine
    eng = FireEngine(n_envs=E, **kw)
    m = aw.mode_settings(mode)
    eng.set_fused(m["fused"])
    if m.get("tuning"):
        eng.set_tuning(**m["tuning"])
    eng.set_rtable(R8)
    return eng


def _world(case, mode):
    kw, R8, E, inits = aw.make_world(case)
    return _engine(kw, E, R8, mode), E, inits, kw["shape"]


def _planes(eng, names, max_d2=0, envs=None, **kw):
    """(what ``distance`` returned as NumPy, the oracle on the maps fetched AFTER the call), int32 [n, H, W] each."""
    lay = eng.cell_layout()
    got = eng.distance(names, envs=envs, dtype="int32", max_d2=max_d2 or None, **kw)
    assert eng.cell_layout() == lay
    got = got.cpu().numpy()
    maps = eng.fire_maps()
    envs = range(eng.n_envs) if envs is None else envs
    return got, np.stack([do.dist2(maps[e], do.mask_of(names), max_d2) for e in envs]), lay


def _again(eng, mode):
    """One more update: behind it a ``run*`` mode keeps the cells in its blocked plane again (the getters of the comparison before
    have converted them), which is then the layout the next ``distance`` call reads."""
    eng.step(1)
    if mode.startswith("run"):
        assert eng.cell_layout() == 1
    if mode == "fused0":
        assert eng.cell_layout() == 0


def _same(got, want, tag):
    bad = np.argwhere(got != want)
    assert got.shape == want.shape and got.dtype == want.dtype and not len(bad), (
        tag, len(bad), bad[:5].tolist(), [(int(got[tuple(i)]), int(want[tuple(i)])) for i in bad[:5]])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------------------------------------- 1. planes through an episode
@pytest.mark.parametrize("case,mode", dw.PAIRS, ids=["%s-%s" % p for p in dw.PAIRS])
def test_planes_through_an_episode(case, mode):
    """Behind calls of 1, 2, 3, 5, 7 and 11 updates, the masks and caps of ``_dist_worlds.queries`` in turn: the int32 plane of every
    environment equals the oracle on the maps; the ``run*`` modes were read in the blocked layout, ``fused0`` in the row-major one."""
    b, E, inits, (H, W) = _world(case, mode)
    lays = []

    def on_query(i, n, names, cap):
        got, want, lay = _planes(b, names, cap)
        assert got.shape == (E, H, W)
        _same(got, want, (case, mode, i, n, names, cap))
        lays.append(lay)
    dw.run_episode(case, mode, b, inits, on_query)
    print("layouts behind the calls:", case, mode, lays)
    if mode.startswith("run"):
        assert lays == [1] * len(dw.CALLS), lays
    if mode == "fused0":
        assert lays == [0] * len(dw.CALLS), lays


# ---------------------------------------------------------------------------------------------- 2. edges, padding, empty sets
@pytest.mark.parametrize("case,mode", [("33x17", "fused0"), ("33x17", "run"), ("70x1030_wide", "run_noteam"), ("70x1030_wide", "auto")])
def test_edges_padding_and_empty_sets(case, mode):
    b, E, inits, (H, W) = _world(case, mode)
    dw.edge_scene(b, E, H, W, inits)
    for names in (("FIRELINE",), ("UNBURNED",)):             # UNBURNED: fails if pitch padding (status byte 0) counts as a source
        for cap in (0, 9):
            got, want, _ = _planes(b, names, cap)
            _same(got, want, (case, mode, names, cap))
            _again(b, mode)
    assert (want[:, 0, :] == 0).sum() < E * W                # (some border cell is no UNBURNED cell)
    for cap, value in ((0, do.FAR), (9, 9)):                 # nothing present is selected
        got, want, _ = _planes(b, ("SCRATCHLINE", "WETLINE"), cap)
        assert (want == value).all()
        _same(got, want, (case, mode, "empty", cap))
        _again(b, mode)
    b.load_fire_map(0, dw.lone_corner_map(H, W))
    got, want, _ = _planes(b, ("BURNING",), envs=[0])
    assert want[0, 0, 0] == (H - 1) ** 2 + (W - 1) ** 2 and want[0, H - 1, W - 1] == 0
    _same(got, want, (case, mode, "lone corner"))
    got, want, _ = _planes(b, ("UNBURNED",), envs=[0])
    assert want[0].sum() == 1 and want[0, H - 1, W - 1] == 1
    _same(got, want, (case, mode, "all but the corner"))


# ---------------------------------------------------------------------------------------------- 3. float output
@pytest.mark.parametrize("case,mode", [("24x40", "run"), ("24x40", "fused0"), ("70x1030_wide", "run_noteam")])
def test_float_output_bits(case, mode):
    b, E, inits, (H, W) = _world(case, mode)
    b.reset(inits)
    b.step(5)
    distinct = set()
    for names, d2 in ((("BURNING",), None), (("BURNING", "BURNED"), 25), (("UNBURNED",), None), (("WETLINE",), None), (("WETLINE",), 1000)):
        for scale in (1.0, 7.0):
            got = b.distance(names, dtype="float32", max_d2=d2, scale=scale).cpu().numpy()
            sq = b.distance(names, dtype="int32", max_d2=d2).cpu().numpy()
            maps = b.fire_maps()
            want = np.stack([do.dist2(maps[e], do.mask_of(names), d2 or 0) for e in range(E)])
            _same(sq, want, (case, mode, names, d2))
            assert got.dtype == np.float32
            _same(_bits(got), _bits(do.as_float(want, scale)), (case, mode, names, d2, scale))
            distinct.update(np.unique(want).tolist())
        _again(b, mode)
    assert do.FAR in distinct and len(distinct) >= (200 if W > 1000 else 40), len(distinct)


# ---------------------------------------------------------------------------------------------- 4. points
def _draw_points(rng, n, k, H, W):
    p = np.stack([rng.integers(-2, W + 2, size=(n, k)), rng.integers(-2, H + 2, size=(n, k)), rng.integers(-1, k + 1, size=(n, k))],
                 axis=-1).astype(np.int32)
    p[:, 0] = (W - 1, H - 1, 1)                               # a corner, valid
    if k >= 3:
        p[:, 1] = p[:, 2]                                     # a duplicate
        p[:, k // 2] = (0, 0, 0)                              # id 0 on the grid: padding
    return p


@pytest.mark.parametrize("mode", ["run", "fused0"])
def test_points(mode):
    import torch
    b, E, inits, (H, W) = _world("33x17", mode)
    b.reset(inits)
    b.step(5)
    rng = np.random.default_rng(4404)
    for k in (1, 3, 64, 65, 256):
        pts = _draw_points(rng, E, k, H, W)
        dev = torch.from_numpy(pts).cuda()
        for names, d2 in ((("BURNING",), None), (("UNBURNED",), None), (("BURNING", "BURNED"), 25), (("FIRELINE",), None)):
            lay = b.cell_layout()
            gi = b.distance(names, points=dev, dtype="int32", max_d2=d2)
            gf = b.distance(names, points=dev, dtype="float32", max_d2=d2, scale=7.0)
            assert b.cell_layout() == lay and gi.shape == (E, k) and gf.shape == (E, k)
            gi, gf = gi.cpu().numpy(), gf.cpu().numpy()
            maps = b.fire_maps()
            want = np.stack([do.at_points(do.dist2(maps[e], do.mask_of(names), d2 or 0), pts[e]) for e in range(E)])
            _same(gi, want, (mode, k, names, d2))
            _same(_bits(gf), _bits(do.points_as_float(want, 7.0)), (mode, k, names, d2, "float"))
            assert (want == -1).any() or k == 1
        _again(b, mode)
    # a subset of the environments, in another order: points[i] belongs to envs[i]
    envs = [E - 1, 0, 0]
    pts = _draw_points(rng, 3, 5, H, W)
    gi = b.distance(("BURNING",), envs=envs, points=torch.from_numpy(pts).cuda(), dtype="int32").cpu().numpy()
    maps = b.fire_maps()
    _same(gi, np.stack([do.at_points(do.dist2(maps[e], 2), pts[i]) for i, e in enumerate(envs)]), (mode, "subset"))


@pytest.mark.parametrize("mode", ["run", "fused0"])
def test_points_are_the_agents_of_the_handle(mode):
    """``agents_device()`` of a handle with agents, passed as it is, between ticks of ``agents_step``."""
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
    rng = np.random.default_rng(4405)
    near = 0
    for t in range(6):
        b.agents_step(torch.from_numpy(rng.integers(0, 5, size=(E, c["K"])).astype(np.int32)).cuda())
        for names, R in ((("BURNING",), None), (("BURNING", "BURNED"), 3)):
            got = b.distance(names, points=b.agents_device(), dtype="float32", max_dist=R).cpu().numpy()
            pos = b.agents_device().cpu().numpy()
            maps = b.fire_maps()
            want = np.stack([do.at_points(do.dist2(maps[e], do.mask_of(names), (R or 0) ** 2), pos[e]) for e in range(E)])
            assert (want >= 0).all()
            _same(_bits(got), _bits(do.points_as_float(want)), (mode, t, names))
            near += int(((want > 0) & (want < 9)).sum())
    assert near > 0


# ---------------------------------------------------------------------------------------------- 5. lists and chunks
@pytest.mark.parametrize("mode", ["run", "fused0"])
def test_lists_and_chunks(mode):
    import torch
    b, E, inits, (H, W) = _world("24x40", mode)
    plane = H * ((W + 15) // 16 * 16) * 2
    b.reset(inits)
    b.step(7)
    mem0 = b.memory_bytes()                                  # (no getter between the measurements: they may allocate staging of their own)
    one = b.distance(("BURNING",), dtype="int32", scratch_bytes=plane)               # one environment per chunk: E chunks
    mem1 = b.memory_bytes()
    assert mem1 - mem0 == plane
    full = b.distance(("BURNING",), dtype="int32")
    assert b.memory_bytes() - mem0 == E * plane and torch.equal(one, full)           # grown to what the call needs ...
    b.distance(("BURNING",), dtype="int32", scratch_bytes=plane)
    assert b.memory_bytes() - mem0 == E * plane                                      # ... and never shrunk
    got, want, _ = _planes(b, ("BURNING",), 0, scratch_bytes=plane)
    _same(got, want, (mode, "one plane of scratch"))
    _same(one.cpu().numpy(), want, (mode, "one plane of scratch, first call"))
    lists = ([e for e in reversed(range(E))], [0, E - 1, 0, 0, 2, E - 1, 2], [1, 3], [2])
    for envs in lists:
        for d2 in (0, 25):
            base, want, _ = _planes(b, ("BURNING", "BURNED"), d2, envs=envs)
            _same(base, want, (mode, envs, d2))
            for scratch in (plane, 2 * plane + 7, 3 * plane):
                got, _, _ = _planes(b, ("BURNING", "BURNED"), d2, envs=envs, scratch_bytes=scratch)
                _same(got, base, (mode, envs, d2, scratch))
        _again(b, mode)
    pts = _draw_points(np.random.default_rng(5), 7, 9, H, W)
    dev = torch.from_numpy(pts).cuda()
    a1 = b.distance(2, envs=lists[1], points=dev, dtype="int32")
    a2 = b.distance(2, envs=lists[1], points=dev, dtype="int32", scratch_bytes=plane)
    assert torch.equal(a1, a2)
    out = torch.full((2, H, W), -7, dtype=torch.int32, device="cuda")
    assert b.distance(2, envs=[1, 3], dtype="int32", out=out) is out and torch.equal(out, b.distance(2, envs=[1, 3], dtype="int32"))
    with pytest.raises(ValueError, match="scratch_bytes"):
        b.distance(2, scratch_bytes=plane - 1)
    with pytest.raises(ValueError, match="out must be"):
        b.distance(2, envs=[1, 3], dtype="float32", out=out)
    assert b.distance(2, envs=[]).shape == (0, H, W)


# ---------------------------------------------------------------------------------------------- 6. reads only
@pytest.mark.parametrize("mode", ["run", "fused0"])
def test_reads_only(mode):
    """The same rollout on two handles, arrival recording on, one of them with plane and point calls between its step calls: maps, burn
    amounts, status rows, elapsed times, arrival planes and the ``fire_map_delta`` sequence are the same."""
    import torch
    kw, R8, E, inits = aw.make_world("24x40")
    H, W = kw["shape"]
    a, b = _engine(kw, E, R8, mode), _engine(kw, E, R8, mode)
    pts = torch.from_numpy(_draw_points(np.random.default_rng(6), E, 7, H, W)).cuda()
    deltas = {id(a): [], id(b): []}
    for h in (a, b):
        h.reset(inits)
        h.enable_arrival(True)
        for i, n in enumerate((1, 2, 3, 5)):
            h.step(n)
            if h is b:
                for call in (lambda: h.distance(dw.MASKS[i % 3], dtype="int32"), lambda: h.distance(2, points=pts, max_dist=4),
                             lambda: h.distance(dw.MASKS[i % 3], envs=[E - 1, 0], scratch_bytes=H * 48 * 2, scale=3.0)):
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
    assert (a.fire_maps() == b.fire_maps()).all()
    for e in range(E):
        assert (a.arrival(e) == b.arrival(e)).all() and (a.burn(e) == b.burn(e)).all(), (mode, e)


# ---------------------------------------------------------------------------------------------- 7. errors
def test_errors_through_the_raw_call():
    import torch
    from simfire_amd import _lib
    b, E, inits, (H, W) = _world("24x40", "run")
    L, h = b._L, b._h
    plane = H * 48 * 2
    out = torch.zeros((E, H, W), dtype=torch.int32, device="cuda")
    pts = torch.zeros((E, 3, 3), dtype=torch.int32, device="cuda")
    all_envs = np.arange(E, dtype=np.int32)

    def rc(n=E, envs=all_envs, out_ptr=None, reserved=(0, 0), **fields):
        p = _lib.SfDistParams(**dict(dict(status_mask=2, scale=1.0), **fields))
        p.reserved[0], p.reserved[1] = reserved
        e = None if envs is None else np.ascontiguousarray(envs, dtype=np.int32)
        return L.sf_distance(h, C.byref(p), n, None if e is None else e.ctypes.data_as(C.c_void_p),
                             C.c_void_p(out.data_ptr() if out_ptr is None else out_ptr))

    assert rc() == _lib.SF_ESTATE                             # before reset
    assert b"sf_reset" in L.sf_last_error()
    b.reset(inits)
    b.step(3)
    bad = [dict(status_mask=0), dict(status_mask=64), dict(status_mask=-1), dict(max_d2=-1), dict(dtype=2), dict(dtype=-1), dict(k=-1),
           dict(k=257), dict(k=3), dict(k=3, points=None), dict(scale=0.0), dict(scale=-1.0), dict(scale=float("inf")),
           dict(scale=float("nan")), dict(reserved=(1, 0)), dict(reserved=(0, 1)), dict(out_ptr=out.data_ptr() + 2),
           dict(envs=[0, E]), dict(envs=[-1, 0], n=2), dict(scratch_bytes=plane - 1), dict(scratch_bytes=1), dict(scratch_bytes=-1),
           dict(n=-1), dict(envs=None), dict(out_ptr=0)]
    for kw in bad:
        kw = dict(kw)
        if "envs" in kw and kw["envs"] is not None and "n" not in kw:
            kw["n"] = len(kw["envs"])
        assert rc(**kw) == _lib.SF_EINVAL, kw
        assert b"sf_distance" in L.sf_last_error(), kw
    assert (out == 0).all()                                   # nothing was enqueued
    assert rc(k=3, points=pts.data_ptr(), out_ptr=out.data_ptr()) == _lib.SF_OK          # the call after an error works
    assert rc(n=0) == _lib.SF_OK
    got, want, _ = _planes(b, ("BURNING",))
    _same(got, want, "after the errors")
    with pytest.raises(ValueError, match="points"):
        b.distance(2, points=pts[:, :, :2])
    with pytest.raises(ValueError, match="points"):
        b.distance(2, points=torch.zeros((E, 257, 3), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="points"):
        b.distance(2, points=pts.cpu())


# ---------------------------------------------------------------------------------------------- 8. BatchedFireEnv
def _config_24x40():
    import yaml
    from simfire_amd.config import Config
    y = yaml.safe_load(open(os.path.join(CFG, "functional_config.yml")))
    y["area"]["screen_size"] = [24, 40]
    y["terrain"]["topography"]["functional"]["function"] = "flat"
    y["simulation"]["headless"] = True
    return Config(config_dict=y)


@pytest.mark.parametrize("option", [dict(status=("BURNING",), max_dist=16), dict(status=("BURNING", "BURNED")), dict()])
def test_batched_fire_env_fire_distance(option):
    """``info["fire_distance"]`` equals the oracle on the maps and ``positions()`` the same ``step`` leaves, also on the tick in which
    every environment starts anew (max_ticks = 3); without the option ``info`` has the old keys only."""
    import torch
    import simfire_amd
    from simfire_amd.simulation import BatchedFireSimulation
    cfg = _config_24x40()
    H, W = cfg.area.screen_size
    E, K = 3, 4
    ign = np.array([(10, 10), (W - 5, 7), (3, H - 4)], dtype=np.int32)
    starts = np.array([(0, 0), (W - 1, H - 1), (12, 10), (W // 2, 2)], dtype=np.int32)
    sim = BatchedFireSimulation(cfg, E, ignitions=ign)
    env = simfire_amd.BatchedFireEnv(sim, K, starts, n_updates=1, max_ticks=3, fire_distance=option)
    plain = simfire_amd.BatchedFireEnv(BatchedFireSimulation(cfg, E, ignitions=ign), K, starts, n_updates=1, max_ticks=3)
    names, R = option.get("status", ("BURNING",)), option.get("max_dist")
    rng = np.random.default_rng(8808)
    env.reset()
    plain.reset()
    restarted = False
    for t in range(5):
        actions = torch.from_numpy(rng.integers(0, 20, size=(E, K)).astype(np.int32)).cuda()
        obs, reward, done, info = env.step(actions)
        obs_p, _, done_p, info_p = plain.step(actions)
        assert set(info_p) == {"terms", "final_len", "final_ret"} and set(info) == set(info_p) | {"fire_distance"}
        assert torch.equal(obs, obs_p) and torch.equal(done, done_p)
        fd = info["fire_distance"]
        assert fd.shape == (E, K) and fd.dtype == torch.float32 and fd.is_cuda
        pos = env.positions().cpu().numpy()
        maps = sim._engine.fire_maps()
        want = np.stack([do.at_points(do.dist2(maps[e], do.mask_of(names), (R or 0) ** 2), pos[e]) for e in range(E)])
        _same(_bits(fd.cpu().numpy()), _bits(do.points_as_float(want)), (t, option))
        if bool(done.all().item()):
            restarted = True
            assert t == 2 and (maps == 1).sum() == E and (pos[:, :, :2] == starts[None]).all()      # the new episode's state
    assert restarted
    with pytest.raises(ValueError, match="fire_distance"):
        simfire_amd.BatchedFireEnv(sim, K, starts, fire_distance=dict(radius=3))
    with pytest.raises(ValueError, match="distance"):
        simfire_amd.BatchedFireEnv(sim, K, starts, fire_distance=dict(status=("EMBERS",)))


# ---------------------------------------------------------------------------------------------- 9. the simulation classes
def test_fire_simulation_distance_to():
    from simfire_amd.config import Config
    from simfire_amd.enums import BurnStatus
    from simfire_amd.simulation import BatchedFireSimulation, FireSimulation
    sim = FireSimulation(Config(os.path.join(CFG, "test_config_flat_simple.yml")))
    sim.run(2)
    m = np.asarray(sim.fire_map)
    assert (m == 1).sum() >= 1 and (m == 0).sum() >= 1
    d = sim.distance_to()
    assert d.shape == m.shape and d.dtype == np.float32
    _same(_bits(d), _bits(do.as_float(do.dist2(m, 2))), "plane")
    _same(_bits(sim.distance_to(max_dist=2)), _bits(do.as_float(do.dist2(m, 2, 4))), "capped")
    sq = sim.distance_to(status=(BurnStatus.UNBURNED,), squared=True)
    assert sq.dtype == np.int32
    _same(sq, do.dist2(m, 1), "squared")
    sim.fire_map[0, 0] = int(BurnStatus.FIRELINE)              # a host edit is pushed first, as run() does
    _same(sim.distance_to(status=("FIRELINE",), squared=True), do.dist2(np.asarray(sim.fire_map), 8), "after a host edit")
    bat = BatchedFireSimulation(_config_24x40(), 3)
    bat.run(4, return_maps=False)
    dev = bat.distance_to(("BURNING", "BURNED"), envs=[2, 0], max_dist=5)
    host = bat.distance_to(("BURNING", "BURNED"), envs=[2, 0], max_dist=5, device=False)
    assert dev.is_cuda and (dev.cpu().numpy() == host).all()
    _same(_bits(host), _bits(np.stack([do.as_float(do.dist2(bat.fire_map(e), 6, 25)) for e in (2, 0)])), "batched")
