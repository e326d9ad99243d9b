"""The cases of ``tests/test_agents_gpu.py``: worlds, agent starts and action draws, all functions of the case's seed, and the loop
that drives handle A - any engine with the pre-agent API - through ``tests/_agents_oracle.py``.  ``tests/test_agents_cpu.py`` runs
the same loop with ``oracle/fire_dense`` standing in for A to check that every case sees what it claims to cover."""
import numpy as np

from _agents_oracle import AgentsOracle

# Grids: 24 x 40 (pitch 48) and 33 x 17 (pitch 32: cells with x % 16 in {0, 15} and the pitch padding next to the agents).
# Every switch of sf_agent_params is on in one case and off in another; K = 1, 5 and the full wave of 64.
CASES = {
    "24x40_k5_u1_att": dict(H=24, W=40, K=5, n_updates=1, att=True, only_unburned=True, done_on_burn=True, max_ticks=0,
                            auto_reset=True, weights=(-1.0, 0.25, -10.0, -0.5), ticks=36, seed=91003),
    "33x17_k64_u3": dict(H=33, W=17, K=64, n_updates=3, att=False, only_unburned=False, done_on_burn=False, max_ticks=0,
                         auto_reset=True, weights=(-0.1, 0.0, -3.0, 0.0), ticks=25, seed=91100),
    "24x40_k1_u1_att_t6": dict(H=24, W=40, K=1, n_updates=1, att=True, only_unburned=False, done_on_burn=False, max_ticks=6,
                               auto_reset=True, weights=(-1.0, 1.0, 1.0, 1.0), ticks=40, seed=91200),
    "33x17_k5_u3_noreset": dict(H=33, W=17, K=5, n_updates=3, att=False, only_unburned=True, done_on_burn=True, max_ticks=6,
                                auto_reset=False, weights=(-0.3, 0.7, -1.1, -0.01), ticks=25, seed=91300),
}


def make_world(case):
    """(engine kwargs without n_envs, R table, E, ignitions [E, 2], starts [E, K, 2]) of a case."""
    from test_env_state_gpu import _world
    c = CASES[case]
    H, W, K = c["H"], c["W"], c["K"]
    rng = np.random.default_rng(c["seed"])
    E = int(rng.integers(4, 9))
    kw, R8 = _world(rng, H, W, 4, c["att"], diag=True)
    kw.update(max_time=float(rng.integers(6, 12)), update_rate=1.0)       # every fire that keeps spreading QUITs on the runtime check
    R8[:, : H // 2] = np.maximum(R8[:, : H // 2], 30.0)                    # (the upper half always passes its fire on)
    # starts on corners and edges; the ignition a few cells from an agent, so that the fire is in reach
    edge = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, 0), (0, H // 2), (W - 1, H // 2), (W // 2, H - 1),
            (15, 0), (16, 0), (min(W - 1, 31), H - 1)]
    starts = np.zeros((E, K, 2), dtype=np.int32)
    inits = np.zeros((E, 2), dtype=np.int32)
    for e in range(E):
        for j in range(K):
            starts[e, j] = edge[int(rng.integers(len(edge)))]
        ax, ay = starts[e, int(rng.integers(K))]
        inits[e] = (int(np.clip(ax + rng.integers(-3, 4), 0, W - 1)), int(np.clip(ay + rng.integers(-3, 4), 0, H - 1)))
    return kw, R8, E, inits, starts


def draw_actions(rng, pos, maps, H, W):
    """int32 [E, K] action words: biased towards the nearest BURNING cell and towards the nearest edge (and past it), with a few
    words outside 0..19."""
    E, K = pos.shape[:2]
    out = np.zeros((E, K), dtype=np.int32)
    for e in range(E):
        ys, xs = np.nonzero(maps[e] == 1)
        for j in range(K):
            x, y = int(pos[e, j, 0]), int(pos[e, j, 1])
            u = rng.random()
            if u < 0.45 and len(xs):
                i = int(np.argmin(np.abs(xs - x) + np.abs(ys - y)))
                dx, dy = int(xs[i]) - x, int(ys[i]) - y
                if abs(dx) >= abs(dy):
                    move = 0 if dx == 0 else (4 if dx > 0 else 3)
                else:
                    move = 2 if dy > 0 else 1
            elif u < 0.7:
                d = [y, H - 1 - y, x, W - 1 - x]             # rows above, below, columns left, right
                move = 1 + int(np.argmin(d))
            else:
                move = int(rng.integers(5))
            word = move + 5 * int(rng.choice([0, 0, 1, 2, 3]))
            if rng.random() < 0.05:
                word = int(rng.choice([-7, -1, 20, 23, 1000]))
            out[e, j] = word
    return out


def drive(case, a, on_tick=None):
    """Drives engine ``a`` (reset at the case's ignitions) through the case with the oracle; ``on_tick(t, actions, result, oracle)``
    after every tick.  Returns what the case saw on handle A alone: ticks with an auto-reset, with ``terms[2] > 0``, with
    ``terms[3] > 0``, with a done report, with an environment found not running, with a point emitted, with one refused."""
    c = CASES[case]
    kw, R8, E, inits, starts = make_world(case)
    rng = np.random.default_rng(c["seed"] + 1)
    o = AgentsOracle(a, E, c["H"], c["W"], c["K"], inits, n_updates=c["n_updates"], weights=c["weights"],
                     only_unburned=c["only_unburned"], done_on_burn=c["done_on_burn"], max_ticks=c["max_ticks"],
                     auto_reset=c["auto_reset"])
    o.place(list(range(E)), starts)
    seen = dict(reset=0, in_fire=0, blocked=0, done=0, off=0, emitted=0, refused=0)
    for t in range(c["ticks"]):
        maps = [a.fire_map(e) for e in range(E)]
        running = a.status()[0][:, 0] == 1
        actions = draw_actions(rng, o.pos, maps, c["H"], c["W"])
        r = o.step(actions)
        seen["done"] += int(r["done"].any())
        seen["reset"] += int(r["done"].any() and c["auto_reset"])
        seen["in_fire"] += int((r["terms"][:, 2] > 0).any())
        seen["blocked"] += int((r["terms"][:, 3] > 0).any())
        seen["off"] += int((~running).sum())
        seen["emitted"] += int(r["terms"][:, 1].sum())
        seen["refused"] += int(((actions >= 5) & (actions <= 19) & (r["points"][:, :, 2] == 0))[running].sum())
        if on_tick is not None:
            on_tick(t, actions, r, o)
    return seen
