"""The fifth reward term of ``sf_agents_step`` (values at risk) on the GPU, bit for bit.  Handle A gets every
tick through the older API, driven by ``tests/_agents_oracle.py`` one update at a time so that its maps give the expected arrival;
``tests/_values_oracle.py`` turns that into damage, the tick's loss and the reward with the fifth product.  Handle B makes the same
ticks with ``agents_step`` under a value plane.  Never the new code against itself.  Run with ``pytest -m gpu``."""
import numpy as np
import pytest

import _episode_oracle as eo
import _values_oracle as vo
from _agents_oracle import AgentsOracle
from _agents_worlds import draw_actions
from _arrival_oracle import MapArrival

pytestmark = pytest.mark.gpu

E, K, TICKS = 5, 3, 60
WEIGHTS = (-1.0, 0.25, -10.0, -0.5)
W_VALUE = -0.01                               # not exact in binary: the rounding of the fifth product is part of the comparison
SIZES = {"24x40": (24, 40, 93100), "72x80": (72, 80, 93200)}


def _make(size):
    """(engine kwargs, R table, ignitions [E, 2], agent starts [E, K, 2], value plane int32 [H, W]) of a size, functions of its seed:
    fires that go on around cells that never burn; towns around the ignition of environment 0 and at three other places, some
    negative cells."""
    from test_env_state_gpu import _world
    H, W, seed = SIZES[size]
    rng = np.random.default_rng(seed)
    kw, R8 = _world(rng, H, W, 4, True)
    R8 = np.where(R8.sum(axis=0) == 0.0, 0.0, np.maximum(R8, 12.0))
    kw.update(max_time=None, update_rate=1.0, pixel_scale=10.0)
    inits = np.stack([rng.integers(W // 4, W - W // 4, size=E), rng.integers(H // 4, H - H // 4, size=E)], axis=1).astype(np.int32)
    starts = np.stack([np.clip(inits[:, None, 0] + rng.integers(-4, 5, size=(E, K)), 0, W - 1),
                       np.clip(inits[:, None, 1] + rng.integers(-4, 5, size=(E, K)), 0, H - 1)], axis=2).astype(np.int32)
    values = np.zeros((H, W), dtype=np.int32)
    x0, y0 = int(inits[0, 0]), int(inits[0, 1])
    boxes = [(max(0, x0 - 4), max(0, y0 - 4), min(W, x0 + 5), min(H, y0 + 5))]
    for _ in range(3):
        w, h = int(rng.integers(4, 12)), int(rng.integers(4, 12))
        x, y = int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1))
        boxes.append((x, y, x + w, y + h))
    for (xa, ya, xb, yb) in boxes:
        values[ya:yb, xa:xb] = rng.integers(1, 1001, size=(yb - ya, xb - xa))
    neg = rng.random((H, W)) < 0.03
    values[neg] = -rng.integers(1, 201, size=int(neg.sum()))
    return kw, R8, inits, starts, values


def _engine(kw, R8, inits, mode):
    from simfire_amd.engine import FireEngine
    from test_env_state_gpu import MODES
    eng = FireEngine(n_envs=E, **kw)
    eng.set_fused(MODES[mode]["fused"])
    if MODES[mode].get("tuning"):
        eng.set_tuning(**MODES[mode]["tuning"])
    eng.set_rtable(R8)
    eng.reset(inits)
    return eng


class _Watched:
    """Handle A as ``AgentsOracle`` (and ``_episode_oracle._Restarts``) sees it: a tick's updates are made one at a time and the map
    after each goes to ``MapArrival``; ``after`` is the damage behind the tick's updates, in front of its resets."""

    def __init__(self, a, H, W, values):
        self.a, self.values, self.exp, self.after = a, values, MapArrival(E, H, W), None
        for e in range(E):
            self.exp.see(e, a.fire_map(e), 0)

    def damage(self):
        return vo.damage(self.values, self.exp.exp)

    def status(self):
        return self.a.status()

    def fire_map(self, e):
        return self.a.fire_map(e)

    def fire_maps(self):
        return self.a.fire_maps()

    def apply_mitigation(self, rows):
        self.a.apply_mitigation(rows)

    def step(self, n):
        for _ in range(n):
            self.a.step(1)
            m, st = self.a.fire_maps(), self.a.status()[0]
            for e in range(E):
                self.exp.see(e, m[e], st[e, 1])
        self.after = self.damage()

    def reset_env(self, e, x, y):
        self.a.reset_env(e, x, y)
        self.exp.restart(e)
        self.exp.see(e, self.a.fire_map(e), 0)

    def reset_envs(self, envs, xy):
        for e, p in zip(envs, xy):
            self.reset_env(int(e), int(p[0]), int(p[1]))


def _outs(torch):
    return dict(reward=torch.empty(E, dtype=torch.float32, device="cuda:0"), done=torch.empty(E, dtype=torch.uint8, device="cuda:0"),
                terms=torch.empty((E, 4), dtype=torch.int32, device="cuda:0"), final_len=torch.empty(E, dtype=torch.int32, device="cuda:0"),
                final_ret=torch.empty(E, dtype=torch.float64, device="cuda:0"))


# auto_reset on and off, n_updates 1 and 6 (6 > max_fire_duration = 4: several pieces and passes per tick); checked plain and - where
# an auto-reset exists to draw them - with the episodes drawn on the device
COMBOS = [(size, auto_reset, n_updates, randomize) for size in SIZES for auto_reset in (True, False) for n_updates in (1, 6)
          for randomize in ((False, True) if auto_reset else (False,))]


@pytest.mark.parametrize("size,auto_reset,n_updates,randomize", COMBOS,
                         ids=["%s-%s-u%d-%s" % (s, "reset" if r else "noreset", u, "drawn" if d else "fixed") for s, r, u, d in COMBOS])
def test_reward_with_the_value_term(size, auto_reset, n_updates, randomize):
    """60 ticks of random actions.  After every tick ``reward``, ``terms``, ``done``, ``final_len``, ``final_ret`` and ``value_lost``
    (``values_torch()[1]``) equal the NumPy restatement - reward and return as bits - and ``damage()`` equals the plane summed over
    A's arrival: after an auto-reset tick the new episode's ``value[ignition]`` while ``value_lost`` still reports the finished
    episode's last tick."""
    import torch
    H, W, seed = SIZES[size]
    kw, R8, inits, starts, values = _make(size)
    a, b = _engine(kw, R8, inits, "fused0"), _engine(kw, R8, inits, "run")
    agent_kw = dict(n_updates=n_updates, weights=WEIGHTS, only_unburned=False, done_on_burn=False, max_ticks=7 if auto_reset else 0,
                    auto_reset=auto_reset)
    b.enable_arrival(True)
    b.values_set(values)
    b.agents_create(K, inits, **agent_kw)
    b.agents_place(list(range(E)), starts)
    b.agents_set_value_weight(W_VALUE)
    watched = _Watched(a, H, W, values)
    proxy, ep = watched, None
    if randomize:
        box = (W // 4, H // 4, W - W // 4, H - H // 4)
        b.episodes_set(seed, ignition_box=box, agent_box=(0, 0, W - 1, H - 1))
        ep = eo.EpisodeOracle(E, seed, inits, ign_box=box, agent_box=(0, 0, W - 1, H - 1), K=K)
        proxy = eo._Restarts(watched, ep)
    o = AgentsOracle(proxy, E, H, W, K, inits, **agent_kw)
    if randomize:
        proxy.agents = o
    o.place(list(range(E)), starts)
    book = vo.RewardBook(E, WEIGHTS, W_VALUE, auto_reset)
    outs = _outs(torch)
    rng = np.random.default_rng(seed + 1)
    assert (b.damage() == watched.damage()).all() and watched.damage()[0] != 0           # the ignition of environment 0 lies in a town
    log = dict(loss_ticks=0, resets=0, off=0, ignition_value=0, on_burning=0)
    for t in range(TICKS):
        tag = (size, auto_reset, n_updates, randomize, t)
        running = a.status()[0][:, 0] == 1
        base = watched.damage()
        maps = a.fire_maps()
        actions = draw_actions(rng, o.pos, maps, H, W)
        want = o.step(actions)
        loss = vo.tick_loss(base, watched.after, running)
        rew, final_ret = book.tick(running, want["terms"], want["done"], loss)
        for v in outs.values():
            v.fill_(77)
        b.agents_step(torch.from_numpy(np.ascontiguousarray(actions, dtype=np.int32)).cuda(), **outs)
        dmg, lost = b.values_torch()
        got = {k: v.cpu().numpy() for k, v in outs.items()}
        for k in ("terms", "done", "final_len"):
            assert (got[k] == want[k]).all(), (tag, k, got[k], want[k])
        assert (lost.cpu().numpy() == loss).all(), (tag, "value_lost", lost.cpu().numpy(), loss)
        assert got["reward"].tobytes() == rew.tobytes(), (tag, "reward", got["reward"], rew)
        assert got["final_ret"].tobytes() == final_ret.tobytes(), (tag, "final_ret", got["final_ret"], final_ret)
        now = watched.damage()
        assert (dmg.cpu().numpy() == now).all() and (b.damage() == now).all(), (tag, "damage", b.damage(), now)
        assert (a.status()[0] == b.status()[0]).all(), (tag, "status")
        log["loss_ticks"] += int((loss != 0).any())
        log["off"] += int((~running).sum())
        pts = want["points"]
        log["on_burning"] += sum(int(pts[e, j, 2] != 0 and maps[e][pts[e, j, 1], pts[e, j, 0]] == 1) for e in range(E) for j in range(K))
        if auto_reset:
            fresh = np.flatnonzero(want["done"])
            log["resets"] += len(fresh)
            log["ignition_value"] += int((now[fresh] != 0).sum())
            assert all((watched.exp.exp[e] >= 0).sum() == 1 for e in fresh), tag
    print("seen:", size, auto_reset, n_updates, randomize, log)
    # ticks that lost value: many - except where six updates per tick and no reset let a fire cross the 24 rows in about four ticks
    assert log["loss_ticks"] >= (10 if auto_reset or n_updates == 1 else 3) and log["on_burning"] >= 1, log
    if auto_reset:
        assert log["resets"] >= E and log["ignition_value"] >= 1, log
    else:
        assert log["off"] >= 1 or n_updates == 1, log            # the fires of the long ticks burn out: ticks of environments that are off


@pytest.mark.parametrize("weights", [WEIGHTS, (-0.0, -0.0, -0.0, -0.0)], ids=["plain", "minus_zero"])
def test_weight_off_leaves_the_reward_bits(weights):
    """A plane set and the weight OFF against a twin handle without values: every output bit-identical over 25 ticks.  With weights
    whose products are all -0.0 the reward is -0.0 on both: a fifth product added as ``+ 0.0`` would make it +0.0 - the term is a
    branch."""
    import torch
    size = "24x40"
    H, W, seed = SIZES[size]
    kw, R8, inits, starts, values = _make(size)
    agent_kw = dict(n_updates=2, weights=weights, only_unburned=False, done_on_burn=False, max_ticks=7, auto_reset=True)
    plain, valued = (_engine(kw, R8, inits, "run") for _ in range(2))
    valued.enable_arrival(True)
    valued.values_set(values)
    for h in (plain, valued):
        h.agents_create(K, inits, **agent_kw)
        h.agents_place(list(range(E)), starts)
    valued.agents_set_value_weight(W_VALUE)
    valued.agents_set_value_weight(None)                        # on, then off again
    outs = [_outs(torch) for _ in range(2)]
    rng = np.random.default_rng(seed + 7)
    minus_zero = np.float32(-0.0).tobytes()
    n_lost = 0
    for t in range(25):
        actions = torch.from_numpy(rng.integers(0, 20, size=(E, K)).astype(np.int32)).cuda()
        for h, o in zip((plain, valued), outs):
            h.agents_step(actions, **o)
        p, v = ({k: x.cpu().numpy() for k, x in o.items()} for o in outs)
        for k in p:
            assert p[k].tobytes() == v[k].tobytes(), (t, k, p[k], v[k])
        n_lost += int((valued.values_torch()[1] != 0).any())
        if weights[0] == 0.0:
            assert all(v["reward"][e].tobytes() == minus_zero for e in range(E)), (t, v["reward"])      # (every environment runs: auto_reset)
    assert n_lost >= 5                                           # the plane was live all along: value_lost is reported with the weight off


def test_batched_fire_env_reports_value_lost():
    """``BatchedFireEnv(values=, value_weight=)``: ``info["value_lost"]`` is an int64 CUDA tensor, equal to what the tick added to
    ``sim.damage()`` (no episode ends in these ticks), the reward carries the fifth product, and the damage is the plane summed over
    the simulation's arrival; with both arguments left out ``info`` has no such key."""
    import os
    import torch
    import yaml
    import simfire_amd
    from simfire_amd.config import Config
    from simfire_amd.simulation import BatchedFireSimulation
    from test_env_state_gpu import CFG
    y = yaml.safe_load(open(os.path.join(CFG, "functional_config.yml")))
    y["area"]["screen_size"] = [64, 64]
    y["terrain"]["topography"]["functional"]["function"] = "flat"
    y["simulation"]["headless"] = True
    cfg = Config(config_dict=y)
    n, k = 4, 2
    H, W = cfg.area.screen_size
    ign = np.array([(10, 10), (W - 5, 7), (3, H - 4), (W // 2, H // 2)], dtype=np.int32)
    starts = np.array([(0, 0), (W - 1, H - 1)], dtype=np.int32)
    rng = np.random.default_rng(97000)
    values = rng.integers(-20, 1001, size=(H, W)).astype(np.int32)
    weights, wv = (-1.0, 0.0, 0.0, 0.0), -0.5
    sim = BatchedFireSimulation(cfg, n, ignitions=ign)
    env = simfire_amd.BatchedFireEnv(sim, k, starts, n_updates=2, weights=weights, values=values, value_weight=wv)
    env.reset()
    assert sim.damage().tolist() == [int(values[yy, xx]) for xx, yy in ign]
    for t in range(4):
        before = sim.damage()
        obs, reward, done, info = env.step(torch.zeros((n, k), dtype=torch.int32, device="cuda:0"))
        lost = info["value_lost"]
        assert lost.is_cuda and lost.dtype == torch.int64 and tuple(lost.shape) == (n,)
        assert not done.any()
        lost, terms = lost.cpu().numpy(), info["terms"].cpu().numpy()
        assert (sim.damage() - before == lost).all() and (lost != 0).any(), (t, lost)
        assert (sim.damage() == vo.damage(values, sim.arrival())).all()
        want = np.array([vo.reward(weights, terms[e], wv, lost[e]) for e in range(n)], dtype=np.float32)
        assert reward.cpu().numpy().tobytes() == want.tobytes(), (t, reward, want)
    env.close()
    plain_sim = BatchedFireSimulation(cfg, n, ignitions=ign)
    plain = simfire_amd.BatchedFireEnv(plain_sim, k, starts, n_updates=2, weights=weights)
    plain.reset()
    info = plain.step(torch.zeros((n, k), dtype=torch.int32, device="cuda:0"))[3]
    assert sorted(info) == ["final_len", "final_ret", "terms"]
    with pytest.raises(ValueError):
        simfire_amd.BatchedFireEnv(plain_sim, k, starts, value_weight=1.0)          # a weight without a plane
    plain.close()
