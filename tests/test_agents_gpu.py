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

ALL_MODES = dict(MODES, auto=aw.AUTO)


def _engine(kw, E, mode, R8, inits, per_env=False):
    from simfire_amd.engine import FireEngine
    eng = FireEngine(n_envs=E, per_env_terrain=per_env, **kw)
    m = ALL_MODES[mode]
    eng.set_fused(m["fused"])
    if m.get("tuning"):
        eng.set_tuning(**m["tuning"])
    if per_env:
        for e in range(E):
            eng.set_rtable(R8[e], env=e)
    else:
        eng.set_rtable(R8)
    eng.reset(inits)
    return eng


def _n_envs(case):
    """The E of a case whose ``E`` key is the device's CU count + 8; None for every other case (its seed or its key decides)."""
    if aw.CASES[case].get("E") == "cu+8":
        import torch
        return torch.cuda.get_device_properties(0).multi_processor_count + 8
    return None


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


def _same_result(got, want, tag, keys=("terms", "done", "final_len", "reward", "final_ret")):
    for k in ("terms", "done", "final_len"):
        if k in keys:
            assert (got[k] == want[k]).all(), (tag, k, got[k], want[k])
    for k in ("reward", "final_ret"):
        if k in keys:
            assert got[k].tobytes() == want[k].tobytes(), (tag, k, got[k], want[k])


def _same_state(a, b, tag, blobs, envs=None):
    sa, ea = a.status()
    sb, eb = b.status()
    assert (sa == sb).all() and ea.tobytes() == eb.tobytes(), (tag, sa, sb)
    if blobs:
        envs = list(range(a.n_envs)) if envs is None else envs
        ba, bb = a.save_state(envs), b.save_state(envs)
        for i, e in enumerate(envs):
            assert ba[i].tobytes() == bb[i].tobytes(), (tag, "state blob of environment", e)


def _create(b, c, inits, **over):
    p = dict(n_updates=c["n_updates"], weights=c["weights"], only_unburned=c["only_unburned"], done_on_burn=c["done_on_burn"],
             max_ticks=c["max_ticks"], auto_reset=c["auto_reset"])
    p.update(over)
    k = p.pop("K", c["K"])
    b.agents_create(k, inits, **p)


def _oracle(a, c, E, inits, **over):
    p = dict(n_updates=c["n_updates"], weights=c["weights"], only_unburned=c["only_unburned"], done_on_burn=c["done_on_burn"],
             max_ticks=c["max_ticks"], auto_reset=c["auto_reset"])
    p.update(over)
    return AgentsOracle(a, E, c["H"], c["W"], p.pop("K", c["K"]), inits, **p)


def _twins(case, mode, **over):
    """(c, E, inits, starts, A, B, the oracle on A) of a case: B has its agents created and placed; ``over``: agent parameters
    that differ from the case's."""
    c = aw.CASES[case]
    kw, R8, E, inits, starts = aw.make_world(case, _n_envs(case))
    a, b = (_engine(kw, E, mode, R8, inits, c.get("per_env", False)) for _ in range(2))
    _create(b, c, inits, **over)
    b.agents_place(list(range(E)), starts)
    o = _oracle(a, c, E, inits, **over)
    o.place(list(range(E)), starts)
    return c, E, inits, starts, a, b, o


def _tick(a, b, o, c, rng, outs, tag, actions=None):
    """One tick on both handles from one action draw: outputs, positions and result rows compared.  Returns (actions, A's result)."""
    import torch
    if actions is None:
        actions = aw.draw_actions(rng, o.pos, [a.fire_map(e) for e in range(o.E)], c["H"], c["W"])
    want = o.step(actions)
    b.agents_step(torch.from_numpy(np.ascontiguousarray(actions, dtype=np.int32)).cuda(), **outs.kwargs())
    _same_result(outs.host(), want, tag)
    assert (b.agents_device().cpu().numpy() == o.xyid()).all(), (tag, "positions")
    _same_state(a, b, tag, False)
    return actions, want


# What a mode's launches leave on handle B after a tick made by agents_step: (last_launch_kind(), cell_layout()).  The lines call
# of a tick is resident wherever the handle offers the resident launch at all (fused = 2; the automatic choice with lines).
_DEFAULT_AFTER = {"fused0": (0, 0), "fused1": (1, 0), "run": (2, 1), "run_win": (2, 1), "run_team": (2, 1), "run_kwin": (2, 1)}


# ------------------------------------------------------------------ 1. twin handles
@pytest.mark.parametrize("case,mode", aw.PAIRS, ids=["%s-%s" % p for p in aw.PAIRS])
def test_twin_handles(case, mode):
    """A (the oracle through the old API) and B (``agents_step``) get the same action tensors for 8 - 40 ticks.  After every tick:
    positions, terms, done, final_len equal, reward and final_ret bitwise, the result block equal; at three random ticks and at the
    end every state blob byte for byte (with more environments than CUs: the first, the last and those around multiples of the CU
    count).  What the case covers (an auto-reset - without auto_reset a done report and an environment that is not running -, an
    agent in the fire, a blocked move, agents either side of the case's ``split``) is asserted on A alone.

    The launch structure is read from B straight after every tick made by ``agents_step``: ``last_launch_kind()`` and
    ``cell_layout()`` are the mode's (``_DEFAULT_AFTER``, or the case's ``expect`` with the reason from ``plan_step`` in
    ``tests/_agents_worlds.py``), and the case's ``engage`` is proved: team - ``team_sizes().max() >= 2``; window -
    ``counters()["window_updates"]`` grows; kwin / many - kind 4 (k_win runs in the plain call of a tick: ``win_first`` needs
    ``!lines``, which ``step_impl(n_updates - 1)`` offers for n_updates = 3 while ``fire_rows <= 62``); wide - pitch / 16 > 64
    vectors, i.e. two bitmap words per row; switch - both layouts occur; generic - kind 3.  Under "run_kwin" the four small first
    cases (H < 64: ``win_first`` is off) run the plain resident launch on B; on A, whose single updates come through ``step(1)``
    without lines, the automatic choice may take the per-step kernels, so A's plane is the one its own last launch names."""
    import torch
    assert tuple(MODES) == aw.BASE_MODES
    c = aw.CASES[case]
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    kw, R8, E, inits, starts = aw.make_world(case, _n_envs(case))
    a, b = (_engine(kw, E, mode, R8, inits, c.get("per_env", False)) for _ in range(2))
    _create(b, c, inits)
    b.agents_place(list(range(E)), starts)
    outs = _Outs(E)
    engage = c.get("engage")
    want_after = c.get("expect", {}).get(mode, _DEFAULT_AFTER.get(mode))
    assert want_after is not None, (case, mode, "no expectation for this mode")
    blob_at = set(np.random.default_rng(c["seed"] + 2).choice(c["ticks"] - 1, size=3, replace=False).tolist()) | {c["ticks"] - 1}
    blob_envs = None
    if E > n_cu:
        blob_envs = sorted({0, 1, E - 1} | {e for m in range(n_cu, E, n_cu) for e in (m - 1, m, m + 1) if e < E})
    if engage == "window":
        b.enable_counters(True)
        b.counters(reset=True)
    if engage == "wide":
        assert b.geometry()["pitch"] // 16 > 64          # more vectors than one 64-bit bitmap word holds: g.VW == 2
    log = dict(kinds=[], layouts=[], team=0, window=[], resets=[], steps_layouts=[])

    def on_steps(t):                           # plain step(n >= 2) calls of the case: the automatic choice and fused = 2 run them resident
        log["steps_layouts"].append(b.cell_layout())

    def on_tick(t, actions, want, o):
        tag = (case, mode, t)
        b.agents_step(torch.from_numpy(actions).cuda(), **outs.kwargs())
        # straight after the tick: the launch's plane is current, nothing converts it below
        kind, layout = b.last_launch_kind(), b.cell_layout()
        log["kinds"].append(kind)
        log["layouts"].append(layout)
        if engage in ("kwin", "many"):         # k_win while the bound on the fires' rows allows it, the plain resident launch after
            assert (kind, layout) in ((4, 1), (2, 1)), (tag, kind, layout)
            assert kind == 4 or 1 + 2 * c["n_updates"] * t + 2 > 62, (tag, kind)
        else:
            assert (kind, layout) == want_after, (tag, kind, layout, want_after)
        assert a.cell_layout() == (1 if a.last_launch_kind() in (2, 4) else 0), (tag, a.last_launch_kind(), a.cell_layout())
        if mode in aw.BASE_MODES and mode != "run_kwin":      # (A steps without lines; with a fixed structure that changes nothing)
            assert a.cell_layout() == (1 if mode in RESIDENT else 0), (tag, a.cell_layout())
        if engage == "team":
            log["team"] = max(log["team"], int(b.team_sizes().max()))
        if engage == "window":
            log["window"].append(b.counters()["window_updates"])
            log["resets"].append(bool(want["done"].any()))       # (auto_reset: every done report lights a new fire)
        _same_result(outs.host(), want, tag)
        assert (b.agents_device().cpu().numpy() == o.xyid()).all(), (tag, "positions")
        if E > n_cu:                           # the last environment, explicitly
            assert (b.agents_device().cpu().numpy()[E - 1] == o.xyid()[E - 1]).all() and outs.host()["terms"][E - 1].tolist() == want["terms"][E - 1].tolist()
        _same_state(a, b, tag, t in blob_at, blob_envs)

    seen = aw.drive(case, a, on_tick, _n_envs(case), twins=(b,), on_steps=on_steps)
    assert seen["in_fire"] and seen["blocked"] and seen["emitted"], (case, seen)
    assert seen["reset"] if c["auto_reset"] else (seen["done"] and seen["off"]), (case, seen)
    if "split" in c:
        assert seen["lo"] and seen["hi"], (case, seen["lo"], seen["hi"])
    print("launch kinds seen on B:", case, mode, sorted(set(log["kinds"])), "layouts", sorted(set(log["layouts"])))
    if engage == "team":
        assert log["team"] >= 2, (case, mode, log["team"])
    elif engage == "window":
        # The window holds blockDim / 16 rows: four per wave, and k_run gives 72 rows two waves (plan_step: nw <= (H + 63) / 64) - a
        # window of 8 rows.  A fire on this terrain gains a row per side and update, so it has left its window for the general loop
        # after four updates at the latest and the counter rests until an auto-reset lights a new fire of one cell: the counter grows
        # in the first tick and in every tick that follows one with a reset, and such ticks occur (max_ticks = 6 of 14).
        w, young = log["window"], [t + 1 for t, r in enumerate(log["resets"][:-1]) if r]
        print("window_updates after every tick:", case, mode, w, "ticks behind a reset:", young)
        assert w[0] > 0 and young, (case, mode, w, young)
        assert all(w[t] > w[t - 1] for t in young) and all(y >= x for x, y in zip(w, w[1:])), (case, mode, w, young)
    elif engage in ("kwin", "many"):
        assert log["kinds"][0] == 4 and log["kinds"].count(4) >= 2, (case, mode, log["kinds"])
    elif engage == "switch":
        assert log["steps_layouts"] and set(log["steps_layouts"]) == {1} and set(log["layouts"]) == {0}, (case, mode, log)
    elif engage == "generic":
        assert set(log["kinds"]) == {3}
    assert a.fire_maps().tobytes() == b.fire_maps().tobytes()
    for e in (range(E) if blob_envs is None else blob_envs):
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


# ------------------------------------------------------------------ 6. the statements of DESIGN.md section 16, one by one
@pytest.mark.parametrize("auto_reset", [True, False])
def test_fire_map_delta_around_ticks(auto_reset):
    """A host mirror of every map kept through ``fire_map_delta`` (``None``: fetch the whole map) equals the oracle's twin's map
    after every tick.  With ``auto_reset`` the mask form of the reset cannot tell the host whose map was cleared: after a tick
    every environment's next delta is ``None`` exactly once - a second query right behind it is an (empty) list, and the deltas
    over plain ``step`` calls behind it are lists that reproduce A's changes.  Without ``auto_reset`` no reference point is ever
    lost: after the first query every delta over ``agents_step`` ticks is a list."""
    case = "24x40_k1_u1_att_t6"
    c, E, inits, starts, a, b, o = _twins(case, "run", auto_reset=auto_reset)
    outs = _Outs(E)
    rng = np.random.default_rng(96100)
    mirror = np.zeros((E, c["H"], c["W"]), dtype=np.uint8)

    def follow(e):
        d = b.fire_map_delta(e)
        if d is None:
            mirror[e] = b.fire_map(e)
            return None
        mirror[e].reshape(-1)[d[0]] = d[1]
        return len(d[0])

    assert [follow(e) for e in range(E)] == [None] * E          # the first query of every environment: no reference point yet
    n_lists = resets = 0
    for t in range(9):
        _, want = _tick(a, b, o, c, rng, outs, ("delta", auto_reset, t))
        resets += int(want["done"].sum())
        got = [follow(e) for e in range(E)]
        if auto_reset:
            assert got == [None] * E, (t, got)
            assert [follow(e) for e in range(E)] == [0] * E, t   # exactly once
            for x in (a, b):
                x.step(1)
            got = [follow(e) for e in range(E)]
        assert None not in got, (t, got)
        n_lists += sum(1 for g in got if g)
        for e in range(E):
            assert (mirror[e] == a.fire_map(e)).all(), (t, e)
    assert n_lists > 0 and resets > 0


def test_agents_step_ends_a_running_loop():
    """``loop_start(k)`` leaves k_run resident; ``agents_step`` ends it like every other entry point (``loop_step`` afterwards is
    ``SF_ESTATE``) and its tick equals the oracle's."""
    from simfire_amd import _lib
    case = "24x40_k5_u1_att"
    c, E, inits, starts, a, b, o = _twins(case, "run")
    outs = _Outs(E)
    rng = np.random.default_rng(96200)
    _tick(a, b, o, c, rng, outs, "before the loop")
    b.loop_start(c["K"])
    b.loop_step(None)
    a.step(1)
    _tick(a, b, o, c, rng, outs, "behind loop_start")
    with pytest.raises(_lib.SimfireHipError):
        b.loop_step(None)
    _tick(a, b, o, c, rng, outs, "one more")
    _same_state(a, b, "loop", True)


@pytest.mark.parametrize("mode", ["fused0", "run"])
def test_prune_after_quit(mode):
    """``set_prune_after_quit`` with a ``max_time`` that makes environments QUIT (their result rows say not running while cells
    still burn), no auto_reset: the agents of a QUIT environment do not move and it reports done = 1, reward 0, terms 0, while its map keeps being pruned exactly as on the twin
    that the oracle steps with ``step`` (maps, rows and blobs equal after every tick; a QUIT environment's map is seen to change)."""
    case = "33x17_k5_u3_noreset"
    c = aw.CASES[case]
    kw, R8, E, inits, starts = aw.make_world(case)
    a, b = (_engine(kw, E, mode, R8, inits) for _ in range(2))
    for x in (a, b):
        x.set_prune_after_quit(True)
    _create(b, c, inits, max_ticks=0)
    b.agents_place(list(range(E)), starts)
    o = _oracle(a, c, E, inits, max_ticks=0)
    o.place(list(range(E)), starts)
    outs = _Outs(E)
    rng = np.random.default_rng(96300)
    quit_ticks = pruned = 0
    for t in range(10):
        st0 = a.status()[0].copy()
        maps0 = a.fire_maps()
        pos0 = b.agents_device().cpu().numpy().copy()
        _tick(a, b, o, c, rng, outs, ("prune", mode, t))
        r = outs.host()
        for e in np.flatnonzero(st0[:, 0] == 0):              # not running; with cells still BURNING: QUIT on the runtime check
            quit_ticks += int(st0[e, 3] > 0)
            assert r["done"][e] == 1 and r["reward"][e].tobytes() == np.float32(0).tobytes() and (r["terms"][e] == 0).all()
            assert (b.agents_device().cpu().numpy()[e] == pos0[e]).all()
            pruned += int((a.fire_map(e) != maps0[e]).any())
        assert a.fire_maps().tobytes() == b.fire_maps().tobytes(), t
        _same_state(a, b, ("prune", mode, t), True)
    assert quit_ticks > 0 and pruned > 0, (quit_ticks, pruned)


def test_any_output_may_be_null():
    """``agents_step`` with no outputs and with every single output: the state (blobs, positions) and the outputs that are given
    equal those of the call with all five, which itself is compared with the oracle."""
    import torch
    case = "24x40_k5_u1_att"
    c, E, inits, starts, a, full, o = _twins(case, "run")
    kw, R8 = aw.make_world(case)[:2]
    outs = _Outs(E)
    rng = np.random.default_rng(96400)
    acts, res = [], []
    for t in range(8):
        act, _ = _tick(a, full, o, c, rng, outs, ("full", t))
        acts.append(act)
        res.append(outs.host())
    assert sum(int(r["done"].sum()) for r in res) > 0
    names = ("reward", "done", "terms", "final_len", "final_ret")
    for given in (None,) + names:
        b = _engine(kw, E, "run", R8, inits)
        _create(b, c, inits)
        b.agents_place(list(range(E)), starts)
        part = _Outs(E)
        for t, act in enumerate(acts):
            kwargs = {} if given is None else {given: part.kwargs()[given]}
            b.agents_step(torch.from_numpy(act).cuda(), **kwargs)
            if given is not None:
                _same_result(part.host(), res[t], (given, t), keys=(given,))
        assert (b.agents_device().cpu().numpy() == full.agents_device().cpu().numpy()).all(), given
        _same_state(full, b, ("outputs", given), True)


def test_create_again_replaces_and_zero_frees():
    """``agents_create`` again with another K mid-run replaces the state (the agents stand at (0, 0) with fresh statistics until
    placed): ticks equal a fresh oracle's.  ``agents_create(0)`` frees it: ``agents_step`` is ``SF_ESTATE`` and the handle still
    steps."""
    import torch
    from simfire_amd import _lib
    case = "24x40_k5_u1_att"
    c, E, inits, starts, a, b, o = _twins(case, "run")
    outs = _Outs(E)
    rng = np.random.default_rng(96500)
    for t in range(4):
        _tick(a, b, o, c, rng, outs, ("K = 5", t))
    K2 = 3
    _create(b, c, inits, K=K2, n_updates=2)
    o2 = _oracle(a, c, E, inits, K=K2, n_updates=2)                 # fresh: every agent at (0, 0), statistics cleared
    assert (b.agents_device().cpu().numpy() == o2.xyid()).all()
    _tick(a, b, o2, c, rng, outs, "K = 3 before place")
    b.agents_place(list(range(E)), starts[:, :K2])
    o2.place(list(range(E)), starts[:, :K2])
    for t in range(5):
        _tick(a, b, o2, c, rng, outs, ("K = 3", t))
    _same_state(a, b, "K = 3", True)
    b.agents_create(0)
    acts = torch.zeros((E, K2), dtype=torch.int32, device="cuda:0")
    with pytest.raises(_lib.SimfireHipError):
        b.agents_step(acts)
    assert b._L.sf_agents_step(b._h, C.c_void_p(acts.data_ptr()), None) == _lib.SF_ESTATE
    for x in (a, b):
        x.step(2)
    _same_state(a, b, "after agents_create(0)", True)


def test_place_twice_and_without_start():
    """An environment named twice in ``agents_place`` keeps its last entry.  ``also_start = False`` moves the agents but not their
    start cells and leaves ``ep_len`` / ``ep_ret`` alone: the auto-reset at max_ticks = 6 comes at the sixth tick of the episode,
    not of the placement, reports its whole length and return, and sends the agents to the OLD start cells."""
    case = "24x40_k1_u1_att_t6"
    c, E, inits, starts, a, b, o = _twins(case, "fused0")
    K, H, W = c["K"], c["H"], c["W"]
    outs = _Outs(E)
    rng = np.random.default_rng(96600)
    first = np.full((1, K, 2), 7, dtype=np.int32)
    last = np.array([[(W - 2, H - 2)] * K], dtype=np.int32)
    other = np.array([[(3, 4)] * K], dtype=np.int32)
    xy = np.concatenate([first, other, last])
    b.agents_place([0, 1, 0], xy)
    o.place([0, 1, 0], xy)
    got = b.agents_device().cpu().numpy()
    assert (got[0, :, :2] == last[0]).all() and (got[1, :, :2] == other[0]).all() and (got == o.xyid()).all()
    starts = starts.copy()
    starts[0], starts[1] = last[0], other[0]
    for t in range(2):
        _tick(a, b, o, c, rng, outs, ("twice", t))
    moved = np.array([[(W // 2, H // 2)] * K] * E, dtype=np.int32)
    b.agents_place(list(range(E)), moved, also_start=False)
    o.place(list(range(E)), moved, also_start=False)
    assert (b.agents_device().cpu().numpy()[:, :, :2] == moved).all()
    whole = 0
    for t in range(2, 6):
        _, want = _tick(a, b, o, c, rng, outs, ("moved", t))
        r = outs.host()
        if t < 5:
            continue
        for e in np.flatnonzero(r["done"]):
            assert (b.agents_device().cpu().numpy()[e, :, :2] == starts[e]).all(), e          # the old start cells
            whole += int(r["final_len"][e] == 6)
    assert whole > 0                       # an episode that ran all six ticks across the placement


def test_agents_are_not_carried_by_copy_or_load():
    """``copy_envs`` and ``save_state`` / ``load_state`` between ticks change the environment's blob and leave the agents where
    they are; after the harness places them itself the ticks equal the oracle's."""
    case = "24x40_k5_u1_att"
    c, E, inits, starts, a, b, o = _twins(case, "run")
    outs = _Outs(E)
    rng = np.random.default_rng(96700)
    _tick(a, b, o, c, rng, outs, "tick 0")
    saved = [x.save_state([2]) for x in (a, b)]
    assert saved[0].tobytes() == saved[1].tobytes()
    for t in range(1, 4):
        _tick(a, b, o, c, rng, outs, ("tick", t))
    pos = b.agents_device().cpu().numpy().copy()
    before = b.save_state([1, 3])
    for x, blob in zip((a, b), saved):
        x.copy_envs([0], [1])
        x.load_state([3], blob)
    after = b.save_state([1, 3])
    assert after[0].tobytes() != before[0].tobytes() and after[1].tobytes() != before[1].tobytes()
    assert (b.agents_device().cpu().numpy() == pos).all()              # neither call moved an agent
    _same_state(a, b, "after copy and load", True)
    b.agents_place([1, 3], pos[[0, 2], :, :2])                           # the harness: the fork's agents beside their source's
    o.place([1, 3], pos[[0, 2], :, :2])
    for t in range(4, 9):
        _tick(a, b, o, c, rng, outs, ("tick", t))
    _same_state(a, b, "end", True)
