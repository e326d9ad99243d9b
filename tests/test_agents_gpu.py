"""Agents on the GPU (``sf_agents_*``, ``BatchedFireEnv``).  The yardstick is the API that existed before: a twin
handle A driven by the NumPy restatement of a tick (``tests/_agents_oracle.py``) through ``status`` / ``fire_map`` /
``apply_mitigation`` / ``step`` / ``reset_env``; handle B makes the same ticks with ``agents_step``.  Never the new code against
itself.  Run with ``pytest -m gpu``."""
import ctypes as C

import numpy as np
import pytest

import _agents_worlds as aw
from _agents_oracle import AgentsOracle
from test_env_state_gpu import CFG, MODES, RESIDENT

pytestmark = pytest.mark.gpu


def _engine(kw, E, mode, R8, inits):
    from simfire_amd.engine import FireEngine
    eng = FireEngine(n_envs=E, **kw)
    m = MODES[mode]
    eng.set_fused(m["fused"])
    if m.get("tuning"):
        eng.set_tuning(**m["tuning"])
    eng.set_rtable(R8)
    eng.reset(inits)
    return eng


class _Outs:
    """The five output tensors of ``agents_step``, filled with junk before every tick."""

    def __init__(self, E, dev="cuda:0"):
        import torch
        self.reward = torch.empty(E, dtype=torch.float32, device=dev)
        self.done = torch.empty(E, dtype=torch.uint8, device=dev)
        self.terms = torch.empty((E, 4), dtype=torch.int32, device=dev)
        self.final_len = torch.empty(E, dtype=torch.int32, device=dev)
        self.final_ret = torch.empty(E, dtype=torch.float64, device=dev)

    def kwargs(self):
        for t in (self.reward, self.done, self.terms, self.final_len, self.final_ret):
            t.fill_(77)
        return dict(reward=self.reward, done=self.done, terms=self.terms, final_len=self.final_len, final_ret=self.final_ret)

    def host(self):
        return dict(reward=self.reward.cpu().numpy(), done=self.done.cpu().numpy(), terms=self.terms.cpu().numpy(),
                    final_len=self.final_len.cpu().numpy(), final_ret=self.final_ret.cpu().numpy())


def _same_result(got, want, tag):
    for k in ("terms", "done", "final_len"):
        assert (got[k] == want[k]).all(), (tag, k, got[k], want[k])
    assert got["reward"].tobytes() == want["reward"].tobytes(), (tag, "reward", got["reward"], want["reward"])
    assert got["final_ret"].tobytes() == want["final_ret"].tobytes(), (tag, "final_ret", got["final_ret"], want["final_ret"])


def _same_state(a, b, tag, blobs):
    sa, ea = a.status()
    sb, eb = b.status()
    assert (sa == sb).all() and ea.tobytes() == eb.tobytes(), (tag, sa, sb)
    if blobs:
        envs = list(range(a.n_envs))
        ba, bb = a.save_state(envs), b.save_state(envs)
        for e in envs:
            assert ba[e].tobytes() == bb[e].tobytes(), (tag, "state blob of environment", e)


def _create(b, c, inits):
    b.agents_create(c["K"], inits, n_updates=c["n_updates"], weights=c["weights"], only_unburned=c["only_unburned"],
                    done_on_burn=c["done_on_burn"], max_ticks=c["max_ticks"], auto_reset=c["auto_reset"])


# ------------------------------------------------------------------ 1. twin handles
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", list(aw.CASES))
def test_twin_handles(case, mode):
    """A (the oracle through the old API) and B (``agents_step``) get the same action tensors for 25 - 40 ticks.  After every tick:
    positions, terms, done, final_len equal, reward and final_ret bitwise, the result block equal; at three random ticks and at the
    end every state blob byte for byte.  The cell plane under the agents is the one the mode names.  What the case covers (an
    auto-reset - without auto_reset a done report and an environment that is not running -, an agent in the fire, a blocked
    move) is asserted on A alone."""
    import torch
    c = aw.CASES[case]
    kw, R8, E, inits, starts = aw.make_world(case)
    a, b = (_engine(kw, E, mode, R8, inits) for _ in range(2))
    _create(b, c, inits)
    b.agents_place(list(range(E)), starts)
    outs = _Outs(E)
    resident = mode in RESIDENT
    blob_at = set(np.random.default_rng(c["seed"] + 2).choice(c["ticks"] - 1, size=3, replace=False).tolist()) | {c["ticks"] - 1}

    def on_tick(t, actions, want, o):
        tag = (case, mode, t)
        b.agents_step(torch.from_numpy(actions).cuda(), **outs.kwargs())
        for x in (a, b):                       # straight after the tick: the launch's plane is current, nothing converts it below
            if mode != "run_kwin":             # (the automatic choice may step a small grid with the per-step kernels)
                assert x.cell_layout() == (1 if resident else 0), (tag, x.cell_layout())
        _same_result(outs.host(), want, tag)
        assert (b.agents_device().cpu().numpy() == o.xyid()).all(), (tag, "positions")
        _same_state(a, b, tag, t in blob_at)

    seen = aw.drive(case, a, on_tick)
    assert seen["in_fire"] and seen["blocked"] and seen["emitted"], (case, seen)
    assert seen["reset"] if c["auto_reset"] else (seen["done"] and seen["off"]), (case, seen)
    assert a.fire_maps().tobytes() == b.fire_maps().tobytes()
    for e in range(E):
        assert a.burn(e).tobytes() == b.burn(e).tobytes(), (case, mode, e)


# ------------------------------------------------------------------ 2. an environment that is not running, auto_reset = 0
@pytest.mark.parametrize("mode", ["fused0", "run"])
def test_not_running_without_auto_reset(mode):
    """Environments 0 and 2 cannot spread: their fires are out after max_fire_duration updates.  From then on their state blobs do
    not change from tick to tick whatever their agents are told, and they report done = 1, reward = 0, terms = 0.  (The blob's
    header records the HANDLE's bound on the rows a fire can span, which grows by two per update until it is the grid's height,
    whoever is stepped: twelve updates come first, so that on these 24 rows it has stopped growing and the whole blob compares.)"""
    import torch
    H, W, E, K = 24, 40, 4, 5
    kw = dict(shape=(H, W), max_fire_duration=4, pixel_scale=50.0, update_rate=1.0, max_time=None, attenuate_line_ros=True,
              diagonal_spread=True)
    from simfire_amd.engine import FireEngine
    b = FireEngine(n_envs=E, per_env_terrain=True, **kw)
    b.set_fused(MODES[mode]["fused"])
    for e in range(E):
        b.set_rtable(np.full((8, H, W), 0.0 if e in (0, 2) else 30.0), env=e)
    inits = np.array([(5, 5), (20, 10), (39, 23), (0, 0)], dtype=np.int32)
    b.reset(inits)
    b.step(12)
    st = b.status()[0]
    assert st[:, 0].tolist() == [0, 1, 0, 1]
    b.agents_create(K, None, n_updates=2, weights=(-1.0, 1.0, 1.0, 1.0), only_unburned=False, auto_reset=False)
    starts = np.tile(np.array([(5, 5), (6, 5), (0, 0), (39, 23), (20, 12)], dtype=np.int32), (E, 1, 1))
    b.agents_place(list(range(E)), starts)
    outs = _Outs(E)
    was = b.save_state([0, 2])
    rng = np.random.default_rng(92000)
    for t in range(4):
        actions = rng.integers(0, 20, size=(E, K)).astype(np.int32)
        b.agents_step(torch.from_numpy(actions).cuda(), **outs.kwargs())
        r = outs.host()
        now = b.save_state([0, 2])
        assert now.tobytes() == was.tobytes(), t
        for e in (0, 2):
            assert r["done"][e] == 1 and r["reward"][e].tobytes() == np.float32(0).tobytes() and (r["terms"][e] == 0).all()
            assert r["final_len"][e] == 0 and r["final_ret"][e] == 0.0
        assert (b.agents_device().cpu().numpy()[[0, 2], :, :2] == starts[[0, 2]]).all()        # their agents stay
        assert r["done"][1] == 0 and r["done"][3] == 0 and r["terms"][1, 1] > 0               # the others live on
    assert b.status()[0][:, 0].tolist() == [0, 1, 0, 1] and b.status()[0][1, 1] == 12 + 8


# ------------------------------------------------------------------ 3. async mode
def test_async_mode_equals_the_synchronous_run():
    """20 ticks enqueued with one ``sync()`` at the end leave what 20 synchronous ticks leave: outputs of every tick, positions,
    blobs."""
    import torch
    case = "24x40_k5_u1_att"
    c = aw.CASES[case]
    kw, R8, E, inits, starts = aw.make_world(case)
    rng = np.random.default_rng(93000)
    acts = [torch.from_numpy(rng.integers(-1, 21, size=(E, c["K"])).astype(np.int32)).cuda() for _ in range(20)]
    res = {}
    for asyn in (False, True):
        b = _engine(kw, E, "run", R8, inits)
        _create(b, c, inits)
        b.agents_place(list(range(E)), starts)
        b.set_async(asyn)
        outs = [_Outs(E) for _ in acts]
        for act, o in zip(acts, outs):
            b.agents_step(act, **o.kwargs())
        b.sync()
        res[asyn] = ([o.host() for o in outs], b.agents_device().cpu().numpy(), b.save_state(list(range(E))), b.status())
    for x, y in zip(res[False][0], res[True][0]):
        _same_result(y, x, "async")
    assert (res[False][1] == res[True][1]).all()
    assert res[False][2].tobytes() == res[True][2].tobytes()
    assert (res[False][3][0] == res[True][3][0]).all()
    assert sum(int(r["done"].sum()) for r in res[True][0]) > 0 and res[True][3][0][:, 1].max() > 0


# ------------------------------------------------------------------ 4. BatchedFireEnv
def test_batched_fire_env():
    """Shapes and dtypes of ``step``'s returns; the ``agent_positions`` channel equals ``observe`` called by hand with the oracle's
    positions; after a tick with an auto-reset the observation is the fresh episode's (one BURNING cell at the ignition, the
    agents on their start cells)."""
    import torch
    import os
    import yaml
    import simfire_amd
    from simfire_amd.config import Config
    from simfire_amd.simulation import BatchedFireSimulation
    y = yaml.safe_load(open(os.path.join(CFG, "functional_config.yml")))
    y["area"]["screen_size"] = [64, 64]
    y["terrain"]["topography"]["functional"]["function"] = "flat"
    y["simulation"]["headless"] = True
    cfg = Config(config_dict=y)
    E, K = 4, 5
    H, W = cfg.area.screen_size
    ign = np.array([(10, 10), (W - 5, 7), (3, H - 4), (W // 2, H // 2)], dtype=np.int32)
    sim = BatchedFireSimulation(cfg, E, ignitions=ign)
    starts = np.array([(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (12, 10)], dtype=np.int32)
    channels = ["fire_map", "agent_positions", "burn_status:BURNING"]
    env = simfire_amd.BatchedFireEnv(sim, K, starts, n_updates=1, weights=(-1, 0, 0, 0), max_ticks=3, obs=dict(channels=channels))
    # handle A: a second simulation built alike, driven by the oracle
    sim_a = BatchedFireSimulation(cfg, E, ignitions=ign)
    o = AgentsOracle(sim_a._engine, E, H, W, K, ign, n_updates=1, weights=(-1, 0, 0, 0), max_ticks=3)
    o.place(list(range(E)), np.broadcast_to(starts, (E, K, 2)))
    obs = env.reset()
    assert obs.shape == (E, 3, H, W) and obs.dtype == torch.float32 and obs.is_cuda
    rng = np.random.default_rng(94000)
    for t in range(4):
        actions = rng.integers(0, 20, size=(E, K)).astype(np.int32)
        obs, reward, done, info = env.step(torch.from_numpy(actions).cuda())
        want = o.step(actions)
        assert obs.shape == (E, 3, H, W) and obs.dtype == torch.float32 and obs.is_cuda
        assert reward.shape == (E,) and reward.dtype == torch.float32 and reward.is_cuda
        assert done.shape == (E,) and done.dtype == torch.bool and done.is_cuda
        assert info["terms"].shape == (E, 4) and info["terms"].dtype == torch.int32
        assert info["final_len"].shape == (E,) and info["final_len"].dtype == torch.int32
        assert info["final_ret"].shape == (E,) and info["final_ret"].dtype == torch.float64
        got = dict(reward=reward.cpu().numpy(), done=done.cpu().numpy().astype(np.uint8), terms=info["terms"].cpu().numpy(),
                   final_len=info["final_len"].cpu().numpy(), final_ret=info["final_ret"].cpu().numpy())
        _same_result(got, want, ("env", t))
        by_hand = sim_a.observe(channels, agents=o.xyid())
        sim_a._engine.sync()                   # (A's handle is in async mode on a stream of its own: observe only enqueued)
        assert sim._engine.async_mode          # step() itself has waited for B's stream: its returns are complete here
        assert torch.equal(obs, by_hand), t
        if t == 2:                             # max_ticks = 3: every environment is done and starts anew inside this step
            assert done.all() and (got["final_len"] == 3).all()
            fm = obs[:, 0].cpu().numpy()
            for e in range(E):
                assert fm[e].sum() == 1 and fm[e, ign[e, 1], ign[e, 0]] == 1
            assert (env.positions().cpu().numpy()[:, :, :2] == starts[None]).all()
    env.close()


# ------------------------------------------------------------------ 5. argument errors
def test_argument_errors_leave_the_handle_usable():
    import torch
    from simfire_amd import _lib
    case = "24x40_k5_u1_att"
    c = aw.CASES[case]
    kw, R8, E, inits, starts = aw.make_world(case)
    H, W, K = c["H"], c["W"], c["K"]
    b = _engine(kw, E, "fused0", R8, inits)
    L, h = b._L, b._h
    acts = torch.zeros((E, K), dtype=torch.int32, device="cuda:0")
    with pytest.raises(_lib.SimfireHipError):                      # a step before create
        b.agents_step(acts)
    assert L.sf_agents_step(h, C.c_void_p(acts.data_ptr()), None) == _lib.SF_ESTATE

    def create_rc(k=K, n_updates=1, ign=inits):
        p = _lib.SfAgentParams(k=k, n_updates=n_updates, only_unburned=1, done_on_burn=0, max_ticks=0, auto_reset=1)
        ign = np.ascontiguousarray(ign, dtype=np.int32)
        return L.sf_agents_create(h, C.byref(p), ign.ctypes.data_as(C.c_void_p))
    bad_ign = inits.copy()
    bad_ign[1] = (W, 0)
    for kwargs in (dict(k=65), dict(k=-1), dict(n_updates=0), dict(ign=bad_ign)):
        assert create_rc(**kwargs) == _lib.SF_EINVAL, kwargs
    for kwargs in (dict(n_agents=65), dict(n_agents=-1), dict(n_agents=K, n_updates=0), dict(n_agents=K, ignitions=bad_ign)):
        with pytest.raises(ValueError):
            b.agents_create(**{"ignitions": inits, **kwargs})
    _create(b, c, inits)
    envs = np.arange(E, dtype=np.int32)
    xy = np.ascontiguousarray(starts)

    def place_rc(envs, xy):
        return L.sf_agents_place(h, len(envs), envs.ctypes.data_as(C.c_void_p), xy.ctypes.data_as(C.c_void_p), 1)
    bad_xy = xy.copy()
    bad_xy[2, K - 1] = (3, H)
    bad_envs = envs.copy()
    bad_envs[0] = E
    assert place_rc(envs, bad_xy) == _lib.SF_EINVAL and place_rc(bad_envs, xy) == _lib.SF_EINVAL
    neg = xy.copy()
    neg[0, 0] = (-1, 0)
    for e_, x_ in ((envs, bad_xy), (bad_envs, xy), (envs, neg), ([-1] + list(range(1, E)), xy)):
        with pytest.raises(ValueError):
            b.agents_place(e_, x_)
    with pytest.raises(ValueError):
        b.agents_step(acts[:, :-1].contiguous())
    # the handle is usable afterwards: a tick equal to the oracle's on a twin
    a = _engine(kw, E, "fused0", R8, inits)
    o = AgentsOracle(a, E, H, W, K, inits, n_updates=c["n_updates"], weights=c["weights"], only_unburned=c["only_unburned"],
                     done_on_burn=c["done_on_burn"], max_ticks=c["max_ticks"], auto_reset=c["auto_reset"])
    o.place(list(range(E)), starts)
    b.agents_place(envs, xy)
    outs = _Outs(E)
    actions = np.random.default_rng(95000).integers(0, 20, size=(E, K)).astype(np.int32)
    b.agents_step(torch.from_numpy(actions).cuda(), **outs.kwargs())
    _same_result(outs.host(), o.step(actions), "after the errors")
    _same_state(a, b, "after the errors", True)
