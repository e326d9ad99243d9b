"""New episodes drawn on the device (``sf_episodes_*``) on the GPU, bit for bit.

Handle A gets every tick through the older API - ``status`` / ``fire_map`` / ``apply_mitigation`` / ``step`` driven by
``tests/_agents_oracle.py`` - and every new episode as ``reset_envs([e], [xy])`` + a host ``set_wind`` with what
``tests/_episode_oracle.py`` draws; handle B makes the same ticks with ``agents_step`` under ``episodes_set``.  Never the new code
against itself.  ``tests/test_episodes_cpu.py`` shows that every case restarts often, rejects dead cells, falls through."""
import ctypes as C

import numpy as np
import pytest

import _episode_oracle as eo
from simfire_amd import _lib

pytestmark = pytest.mark.gpu


def _engine(world, mode=None):
    from simfire_amd.engine import FireEngine
    from test_env_state_gpu import MODES
    layers = "planes" in world
    eng = FireEngine(n_envs=world["E"], per_env_terrain=layers, **world["kw"])
    if mode is not None:
        eng.set_fused(MODES[mode]["fused"])
        if MODES[mode].get("tuning"):
            eng.set_tuning(**MODES[mode]["tuning"])
    if layers:
        for e, p in enumerate(world["planes"]):
            eng.set_layers(*p, env=e)
    else:
        eng.set_rtable(world["R8"])
    eng.reset(world["inits"])
    return eng


@pytest.mark.parametrize("case,mode", eo.PAIRS)
def test_twin_handles(case, mode):
    """A (the two oracles through the old API) and B (``agents_step`` with randomisation set) get the same action tensors.  After
    every tick: outputs, positions, result rows, elapsed times, fire maps and ``episodes_torch()`` (the wind as bits); after the last
    the wind planes and the burn amounts."""
    import torch
    c = eo.CASES[case]
    world = eo.make_world(case)
    a, b = _engine(world, mode), _engine(world, mode)
    b.agents_create(c["K"], world["inits"], n_updates=c["n_updates"], weights=eo.WEIGHTS, only_unburned=True, done_on_burn=False,
                    max_ticks=c["max_ticks"], auto_reset=True)
    b.agents_place(list(range(c["E"])), world["starts"])
    b.episodes_set(**eo.episode_kwargs(case))
    seen = eo.drive(case, a, world, b, torch)
    assert seen["restarts"] >= 3 * c["E"]


def test_episodes_begin_without_agents():
    """``episodes_begin`` with ``all=True``, with a device mask and - after some environments QUIT on the runtime check - with a null
    mask, against ``reset_envs`` on A at the oracle's cells; arrival recording is on on both handles: the plane of a restarted
    environment is a fresh one's (the ignition at update 0, nothing else)."""
    import torch
    case = "24x40_live_agents"
    c = eo.CASES[case]
    world = eo.make_world(case)
    world["kw"].update(max_time=6.0)                         # an episode QUITs with its seventh update
    E, H, W = c["E"], c["H"], c["W"]
    for mode in ("run", "fused0"):
        a, b = _engine(world, mode), _engine(world, mode)
        for h in (a, b):
            h.enable_arrival(True)
        ep = eo.EpisodeOracle(E, 777, world["inits"], ign_box=c["ign_box"], live=True, rt=lambda e: world["R8"])
        on_a = eo._Restarts(a, ep)
        b.episodes_set(777, ignition_box=c["ign_box"], live_cells=True)

        def same(tag, fresh=()):
            sa, ea = a.status()
            sb, eb = b.status()
            assert (sa == sb).all() and ea.tobytes() == eb.tobytes(), (mode, tag, sa, sb)
            assert (a.fire_maps() == b.fire_maps()).all(), (mode, tag)
            got = {k: v.cpu().numpy() for k, v in b.episodes_torch().items()}
            assert (got["index"].view(np.uint32) == ep.index).all() and (got["ignition"] == ep.ign).all(), (mode, tag, got, ep.index, ep.ign)
            assert (got["wind"] == 0.0).all()
            for e in range(E):
                arr = b.arrival(e)
                assert (arr == a.arrival(e)).all(), (mode, tag, "arrival", e)
                if e in fresh:
                    want = np.full((H, W), -1, dtype=np.int32)
                    want[ep.ign[e, 1], ep.ign[e, 0]] = 0
                    assert (arr == want).all(), (mode, tag, "fresh arrival plane", e)

        b.episodes_begin(all=True)                           # the first episodes of a run
        for e in range(E):
            on_a.reset_env(e)
        same("all", fresh=range(E))
        for h in (a, b):
            h.step(4)
        mask = torch.zeros(E, dtype=torch.uint8, device=f"cuda:{b.params.device}")
        mask[[0, 2]] = 1
        b.episodes_begin(mask)
        for e in (0, 2):
            on_a.reset_env(e)
        same("mask", fresh=(0, 2))
        for h in (a, b):
            h.step(4)                                        # 8 updates in 1, 3, 4: they QUIT; 4 in 0, 2: they run
        off = [int(e) for e in np.flatnonzero(a.status()[0][:, 0] != 1)]
        assert {1, 3, 4} <= set(off) and len(off) < E, off
        b.episodes_begin()                                   # null mask: the environments that are not running
        for e in off:
            on_a.reset_env(e)
        same("not running", fresh=off)
        for h in (a, b):
            h.step(3)
        same("after")
        assert (ep.index >= 2).all() and ep.rejected >= 1
        for e in range(E):
            assert (a.burn(e) == b.burn(e)).all(), (mode, "burn", e)


def test_set_then_cleared_equals_never_set():
    """Ticks under randomisation, then ``episodes_set(None)``, a reset and the agents placed anew: from there on the handle equals
    one that never had it - outputs, positions and state blobs."""
    import torch
    case = "24x40_live_agents"
    c = eo.CASES[case]
    world = eo.make_world(case)
    E, K = c["E"], c["K"]
    b, n = _engine(world, "run"), _engine(world, "run")
    for h in (b, n):
        h.agents_create(K, world["inits"], n_updates=1, weights=eo.WEIGHTS, max_ticks=3, auto_reset=True)
        h.agents_place(list(range(E)), world["starts"])
    dev = f"cuda:{b.params.device}"
    rng = np.random.default_rng(5)
    acts = [torch.from_numpy(rng.integers(0, 20, size=(E, K)).astype(np.int32)).to(dev) for _ in range(16)]
    mem0 = b.memory_bytes()
    b.episodes_set(3, ignition_box=c["ign_box"])
    assert b.memory_bytes() > mem0                           # the episode buffers are counted ...
    b.episodes_set(None)
    assert b.memory_bytes() == mem0                          # ... and freed
    b.episodes_set(3, ignition_box=c["ign_box"], live_cells=True, agent_box=c["agent_box"])
    for t in range(6):
        b.agents_step(acts[t])
    assert (b.episodes_torch()["index"].cpu().numpy() >= 2).all()
    b.episodes_set(None)
    with pytest.raises(_lib.SimfireHipError):
        b.episodes_torch()
    b.reset(world["inits"])
    b.agents_place(list(range(E)), world["starts"])
    outs = [dict(reward=torch.empty(E, dtype=torch.float32, device=dev), done=torch.empty(E, dtype=torch.uint8, device=dev),
                 final_ret=torch.empty(E, dtype=torch.float64, device=dev)) for _ in range(2)]
    for t in range(6, 16):
        for h, o in zip((b, n), outs):
            h.agents_step(acts[t], **o)
        for k in outs[0]:
            assert outs[0][k].cpu().numpy().tobytes() == outs[1][k].cpu().numpy().tobytes(), (t, k)
        assert torch.equal(b.agents_device(), n.agents_device()), t
        sb, sn = b.save_state(list(range(E))), n.save_state(list(range(E)))
        assert all(sb[i].tobytes() == sn[i].tobytes() for i in range(E)), t


def test_refusals():
    """What ``sf_episodes_set`` / ``sf_episodes_begin`` refuse, as the Python exceptions the codes map to; a refused call changes
    nothing."""
    from simfire_amd.engine import FireEngine
    from test_wind_change_gpu import _planes
    H, W = 24, 40
    planes = _planes(5, H, W, 3)
    eng = FireEngine((H, W), n_envs=3, per_env_terrain=True, pixel_scale=30.0)
    for e in (0, 1):
        eng.set_layers(*planes[e], env=e)
    eng.set_rtable(np.full((8, H, W), 5.0), env=2)            # a table without layers
    L, h = eng._L, eng._h
    with pytest.raises(_lib.SimfireHipError):
        eng.episodes_begin(all=True)                          # before episodes_set
    with pytest.raises(_lib.SimfireHipError):
        eng.episodes_torch()
    with pytest.raises(_lib.SimfireHipError):
        eng.episodes_set(1)                                   # no ignition drawn, and the handle has neither agents nor been reset
    box = (2, 2, 30, 20)
    eng.episodes_set(1, ignition_box=box)
    with pytest.raises(_lib.SimfireHipError):
        eng.episodes_begin(all=True)                          # the handle was never reset
    eng.reset([(5, 5), (6, 6), (7, 7)])
    p = _lib.SfEpisodeParams(seed=1, flags=16)
    assert L.sf_episodes_set(h, C.byref(p)) == _lib.SF_EINVAL                                    # unknown flag bits
    p = _lib.SfEpisodeParams(seed=1, flags=_lib.SF_EP_IGNITION, reserved=1)
    p.ign_box[:] = box
    assert L.sf_episodes_set(h, C.byref(p)) == _lib.SF_EINVAL                                    # reserved
    p = _lib.SfEpisodeParams(seed=1, flags=_lib.SF_EP_LIVE_CELL)
    assert L.sf_episodes_set(h, C.byref(p)) == _lib.SF_EINVAL                                    # live cells without an ignition box
    for bad in ((0, 0, W, 5), (-1, 0, 5, 5), (6, 0, 5, 5), (0, 0, 5, H), (0, 9, 5, 8)):
        p = _lib.SfEpisodeParams(seed=1, flags=_lib.SF_EP_AGENTS)
        p.agent_box[:] = bad
        assert L.sf_episodes_set(h, C.byref(p)) == _lib.SF_EINVAL, bad
        with pytest.raises(ValueError):
            eng.episodes_set(1, ignition_box=bad)
    for U, D in (((-1.0, 5.0), (0.0, 1.0)), ((6.0, 5.0), (0.0, 1.0)), ((1.0, 5.0), (2.0, 1.0)), ((1.0, float("inf")), (0.0, 1.0)),
                 ((1.0, 5.0), (float("nan"), 1.0))):
        p = _lib.SfEpisodeParams(seed=1, flags=_lib.SF_EP_WIND)
        p.U[:], p.U_dir[:] = U, D
        assert L.sf_episodes_set(h, C.byref(p)) == _lib.SF_EINVAL, (U, D)
        with pytest.raises(ValueError):
            eng.episodes_set(1, wind_speed=U, wind_direction=D)
    with pytest.raises(ValueError):
        eng.episodes_set(1, live_cells=True)
    with pytest.raises(ValueError):
        eng.episodes_set(1, wind_speed=(1.0, 2.0))
    # the refused calls left the setting alone
    assert eng.episodes_torch()["index"].cpu().numpy().tolist() == [0, 0, 0]
    with pytest.raises(_lib.SimfireHipError):
        eng.episodes_set(1, wind_speed=(100.0, 200.0), wind_direction=(0.0, 90.0))               # table 2 has no layers
    eng.set_layers(*planes[2], env=2)
    eng.set_wind_schedule([1], [(0, 100.0, 0.0), (5, 900.0, 90.0)])
    with pytest.raises(_lib.SimfireHipError):
        eng.episodes_set(1, wind_speed=(100.0, 200.0), wind_direction=(0.0, 90.0))               # a schedule is set
    eng.set_wind_schedule([1], [])
    eng.episodes_set(1, wind_speed=(100.0, 200.0), wind_direction=(0.0, 90.0))
    with pytest.raises(_lib.SimfireHipError):
        eng.set_wind_schedule([1], [(0, 100.0, 0.0)])                                            # ... and the other way round
    eng.episodes_begin(all=True)
    w = eng.episodes_torch()["wind"].cpu().numpy()
    assert ((w[:, 0] >= 100.0) & (w[:, 0] < 200.0) & (w[:, 1] >= 0.0) & (w[:, 1] < 90.0)).all()
    eng.episodes_set(None)
    eng.set_wind_schedule([1], [(0, 100.0, 0.0)])
    shared = FireEngine((H, W), n_envs=2, pixel_scale=30.0)
    shared.set_layers(*planes[0])
    shared.reset([(5, 5), (6, 6)])
    with pytest.raises(_lib.SimfireHipError):
        shared.episodes_set(1, wind_speed=(100.0, 200.0), wind_direction=(0.0, 90.0))            # one terrain for all environments
    shared.episodes_set(1, ignition_box=box, live_cells=True)                                    # (the shared table serves every draw)
    shared.episodes_begin(all=True)
    ign = shared.episodes_torch()["ignition"].cpu().numpy()
    rt = shared.get_rtable(0)
    for e in range(2):
        assert tuple(ign[e]) == eo.ignition(1, e, 0, box, rt)[:2]


def test_batched_fire_env():
    """``BatchedFireEnv`` for 20 ticks with ignition, wind and agent cells drawn: every return equals a second simulation driven
    by the oracles (``observe`` by hand with the oracle's positions), and the observation of a tick with an auto-reset shows the
    drawn ignition as the one BURNING cell and the agents on the drawn cells."""
    import torch
    import simfire_amd
    from simfire_amd.config import Config
    from simfire_amd.simulation import BatchedFireSimulation
    from _agents_oracle import AgentsOracle
    from test_wind_change_gpu import _simple_dict
    H, W, E, K, seed = 24, 40, 3, 2, 4242
    ign = [[5, 5], [20, 12], [30, 8]]
    make = lambda: BatchedFireSimulation(Config(config_dict=_simple_dict(H, W, 7, 90.0), simplex_topography=True), E, ignitions=ign,
                                         per_env_terrain=True)
    sim, sim_a = make(), make()
    a = sim_a._engine
    starts = np.array([[0, 0], [W - 1, H - 1]], dtype=np.int32)
    channels = ["fire_map", "agent_positions", "wind_speed"]
    box, abox, mph, deg = (4, 3, 35, 20), (0, 0, W - 1, H - 1), (5.0, 15.0), (0.0, 360.0)
    env = simfire_amd.BatchedFireEnv(sim, K, starts, n_updates=1, max_ticks=3, auto_reset=True, obs=dict(channels=channels, normalize=False))
    assert env.reset().shape == (E, 3, H, W)                # randomisation off: sim.reset()
    assert not sim.episodes_randomized
    sim.randomize_episodes(seed, ignition_box=box, live_cells=True, wind_speed_mph=mph, wind_direction=deg, agent_box=abox)
    assert sim.episodes_randomized
    ep = eo.EpisodeOracle(E, seed, ign, ign_box=box, live=True, wind=((mph[0] * 88, mph[1] * 88), deg), agent_box=abox, K=K,
                          rt=lambda e: a.get_rtable(e))
    on_a = eo._Restarts(a, ep)
    o = AgentsOracle(on_a, E, H, W, K, ign, n_updates=1, max_ticks=3)
    on_a.agents = o

    def check(obs, tag, fresh):
        by_hand = sim_a.observe(channels, agents=o.xyid(), normalize=False)
        a.sync()
        assert torch.equal(obs, by_hand), tag
        info = {k: v.cpu().numpy() for k, v in env.episode_info().items()}
        assert (info["index"].view(np.uint32) == ep.index).all() and (info["ignition"] == ep.ign).all(), tag
        assert info["wind"].tobytes() == ep.wind.tobytes(), tag
        fm, ag, ws = (obs[:, i].cpu().numpy() for i in range(3))
        for e in fresh:
            assert fm[e].sum() == 1 and fm[e, ep.ign[e, 1], ep.ign[e, 0]] == 1, (tag, e)
            assert {(int(x), int(y)) for y, x in np.argwhere(ag[e] != 0)} == {(int(x), int(y)) for x, y in o.start[e]}, (tag, e)
            assert (ws[e] == np.float32(ep.wind[e, 0])).all(), (tag, e)
        assert (env.positions().cpu().numpy() == o.xyid()).all(), tag

    obs = env.reset()                                        # drawn episodes everywhere (all = True)
    for e in range(E):
        on_a.reset_env(e)
    o.place(list(range(E)), o.start.copy())
    check(obs, "reset", range(E))
    rng = np.random.default_rng(seed)
    restarts = 0
    for t in range(20):
        actions = rng.integers(0, 20, size=(E, K)).astype(np.int32)
        obs, reward, done, info = env.step(torch.from_numpy(actions).cuda())
        want = o.step(actions)
        assert (done.cpu().numpy().astype(np.uint8) == want["done"]).all(), t
        assert reward.cpu().numpy().tobytes() == want["reward"].tobytes(), t
        assert (info["final_len"].cpu().numpy() == want["final_len"]).all(), t
        check(obs, t, np.flatnonzero(want["done"]))
        restarts += int(want["done"].sum())
    assert restarts >= 6 * E and len({v[:2] for v in ep.episodes[0]}) >= 2
    sim.randomize_episodes(None)
    assert not sim.episodes_randomized
    env.close()


def test_agent_box_before_agents_create_and_the_fixed_ignition():
    """``SF_EP_AGENTS`` set before the agents exist takes effect once they do, and without ``SF_EP_IGNITION`` a new episode ignites
    where the environment last did: at the last ``reset``'s cells, then at the ignitions a later ``agents_create`` brings."""
    import torch
    case = "24x40_live_agents"
    c = eo.CASES[case]
    world = eo.make_world(case)
    E, K, H, W = c["E"], 3, c["H"], c["W"]
    box = (2, 3, 30, 20)
    b = _engine(world, "fused0")
    b.episodes_set(9, agent_box=box)
    assert (b.episodes_torch()["ignition"].cpu().numpy() == world["inits"]).all()
    ign2 = np.clip(world["inits"] + 2, 0, [W - 1, H - 1]).astype(np.int32)
    b.agents_create(K, ign2, n_updates=1, max_ticks=1, auto_reset=True)
    b.agents_place(list(range(E)), world["starts"][:, :K])
    assert (b.episodes_torch()["ignition"].cpu().numpy() == ign2).all()
    act = torch.zeros((E, K), dtype=torch.int32, device=f"cuda:{b.params.device}")
    for ep in range(2):                                      # max_ticks = 1: every tick ends every episode
        b.agents_step(act)
        want = np.stack([eo.agent_starts(9, e, ep, box, K) for e in range(E)])
        assert (b.agents_device().cpu().numpy()[:, :, :2] == want).all(), ep
        maps = b.fire_maps()
        for e in range(E):
            assert (maps[e] == 1).sum() == 1 and maps[e][ign2[e, 1], ign2[e, 0]] == 1, (ep, e)
    info = b.episodes_torch()
    assert info["index"].cpu().numpy().tolist() == [2] * E and (info["ignition"].cpu().numpy() == ign2).all()
