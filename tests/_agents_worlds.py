"""The cases of ``tests/test_agents_gpu.py``: worlds, agent starts and action draws, all functions of the case's seed, and the loop
that drives handle A - any engine with the pre-agent API - through ``tests/_agents_oracle.py``.  ``tests/test_agents_cpu.py`` runs
the same loop with ``oracle/fire_dense`` standing in for A to check that every case sees what it claims to cover."""
import numpy as np

from _agents_oracle import AgentsOracle

# The mode names of tests/test_env_state_gpu.py (MODES, asserted equal in the GPU test) and one more: "auto" is the automatic choice
# (set_fused(-1)) with every knob at its default.
BASE_MODES = ("fused0", "fused1", "run", "run_win", "run_team", "run_kwin")
AUTO = dict(fused=-1)

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
OLD_CASES = tuple(CASES)

# ---- Cases at the smallest grids where a launch structure engages (plan_step / plan_modes / team_geometry of simfire_hip.hip).
# Optional keys: ``modes`` (the modes the case runs under; default: BASE_MODES), ``engage`` (what the GPU test proves ran on handle B
# during agents_step ticks), ``expect`` (mode -> (last_launch_kind, cell_layout) of B after every tick where the mode's default does
# not hold), ``md`` / ``diag`` / ``per_env`` / ``E`` (E = "cu+8": the device's CU count + 8), ``spots`` (the cells agents start on,
# instead of corners and edges), ``split`` (("row" | "col", v): agents are seen on both sides of it), ``pre_steps`` (updates both
# handles make through step() before the first tick), ``between`` ((every, n): step(n) on both handles in front of every
# ``every``-th tick), ``one_fetch`` (handle A answers fire_map(e) from one fire_maps() per query point), ``max_time`` (False: none).
# Wave tiles are 64 x 32 cells on grids of >= 49 columns: tile rows start at multiples of 32.
_TEAM_SPOTS = [(0, 63), (10, 64), (63, 64), (32, 31), (32, 32), (5, 95), (20, 96), (0, 0), (63, 135), (32, 70), (31, 60), (40, 66)]
_WIDE_SPOTS = [(1023, 0), (1024, 0), (1029, 0), (1023, 35), (1024, 36), (1029, 69), (1022, 40), (1025, 30), (1029, 34), (1024, 69)]
_team = dict(H=136, W=64, K=5, att=True, only_unburned=True, done_on_burn=False, max_ticks=7, auto_reset=True,
             weights=(-1.0, 0.25, -10.0, -0.5), modes=("run_team",), engage="team", spots=_TEAM_SPOTS, split=("row", 64))
CASES.update({
    # run_team = 2 is honoured from two tile rows on (team_forced: team_knob <= g.TY); 136 rows are five.  The bands are cut behind
    # the tile row that holds half of the fire's vectors (cut_bands): fires lit around row 64 are cut at row 64 or 96.
    "136x64_k5_u1_team": dict(_team, n_updates=1, ticks=14, seed=91400),
    "136x64_k5_u3_team": dict(_team, n_updates=3, ticks=10, seed=91410),
    # the window phase of k_run (fused = 2; run_window = 3 in "run_win", the default 1 in "run"): H >= 64; young fires recur with
    # max_ticks = 6.  Weights that are not exact in binary and terms in the hundreds (the reward arithmetic, test_agents_cpu.py).
    "72x80_k5_u2_win": dict(H=72, W=80, K=5, n_updates=2, att=False, only_unburned=True, done_on_burn=False, max_ticks=6,
                            auto_reset=True, weights=(-0.1, 1.0 / 3.0, -1e-3, 0.7), ticks=14, seed=91500, modes=("run_win", "run"),
                            engage="window", max_time=False, hot=400.0),
    # k_win in front of k_run: only the plain call of a tick (step_impl(n_updates - 1), no lines) can have it: win_first needs
    # !lines, H >= 64, PV >= 4, fire_rows <= 62.  run_compact = 2 offers it at any batch size.
    "64x64_k3_u3_kwin": dict(H=64, W=64, K=3, n_updates=3, att=True, only_unburned=True, done_on_burn=True, max_ticks=5,
                             auto_reset=True, weights=(-1.0, 0.25, -10.0, -0.5), ticks=10, seed=91600, modes=("run_kwin",),
                             engage="kwin", expect={"run_kwin": (4, 1)}),
    # rows of two bitmap words (pitch 1040 = 65 vectors): in the automatic mode the lines call of a tick runs on the per-step
    # kernels (team_wide is off with lines) and the plain call as a team launch of k_run (team_wide): both planes inside every tick.
    "70x1030_k5_u3_wide": dict(H=70, W=1030, K=5, n_updates=3, att=True, only_unburned=True, done_on_burn=True, max_ticks=5,
                               auto_reset=True, weights=(-1.0, 0.25, -10.0, -0.5), ticks=10, seed=91700, modes=("auto", "fused0"),
                               engage="wide", E=3, spots=_WIDE_SPOTS, split=("col", 1024), expect={"auto": (2, 1)}),
    # the plane switches inside a tick: automatic mode, n_updates = 2.  plan_step: the lines call is resident (lines, VW == 1), the
    # single plain update is not (n_steps == 1, and the lines call has cleared step1_polls) and runs fused (E * TY * TX <= 12288).
    # Expected cell_layout(): 1 after the pre-steps (step(4) is resident), 0 after every tick, 1 after every step(2) in between.
    "40x48_k5_u2_switch": dict(H=40, W=48, K=5, n_updates=2, att=True, only_unburned=True, done_on_burn=True, max_ticks=0,
                               auto_reset=True, weights=(-1.0, 0.25, -10.0, -0.5), ticks=16, seed=91800, modes=("auto",),
                               engage="switch", pre_steps=4, between=(3, 2), expect={"auto": (1, 0)}),
    # the per-cell kernel (sprite planes of two bytes): row-major plane only
    "24x40_k5_u2_md8": dict(H=24, W=40, K=5, n_updates=2, att=True, only_unburned=True, done_on_burn=True, max_ticks=0,
                            auto_reset=True, weights=(-1.0, 0.25, -10.0, -0.5), ticks=16, seed=91900, modes=("auto",), md=8,
                            engage="generic", expect={"auto": (3, 0)}),
    "24x40_k5_u2_nodiag": dict(H=24, W=40, K=5, n_updates=2, att=False, only_unburned=True, done_on_burn=True, max_ticks=8,
                               auto_reset=True, weights=(-1.0, 0.25, -10.0, -0.5), ticks=20, seed=92000, modes=("fused0", "run"),
                               diag=False),
    "24x40_k5_u2_perenv": dict(H=24, W=40, K=5, n_updates=2, att=True, only_unburned=True, done_on_burn=True, max_ticks=5,
                               auto_reset=True, weights=(-1.0, 0.25, -10.0, -0.5), ticks=16, seed=92100, modes=("fused0", "run"),
                               per_env=True),
    # more environments than CUs: blockIdx.x beyond the CU count in both agent kernels and the reset mask; the automatic mode puts
    # k_win in front of the plain call (win_first: g.E > n_cu while fire_rows <= 62: 1 + 6 per tick).
    "64x64_k3_u3_many": dict(H=64, W=64, K=3, n_updates=3, att=True, only_unburned=True, done_on_burn=False, max_ticks=3,
                             auto_reset=True, weights=(-1.0, 0.25, -10.0, -0.5), ticks=8, seed=92200, modes=("auto",),
                             engage="many", E="cu+8", one_fetch=True, expect={"auto": (4, 1)}),
})
E_STAND_IN = 264      # "cu+8" where there is no device to ask (test_agents_cpu.py)


def case_modes(case):
    return tuple(CASES[case].get("modes", BASE_MODES))


PAIRS = [(case, mode) for case in CASES for mode in case_modes(case)]


class OneFetch:
    """Handle A of a case with many environments: ``fire_map(e)`` out of one ``fire_maps()`` per query point (whatever changes the
    maps drops the copy)."""

    def __init__(self, eng):
        self.eng, self._maps = eng, None

    def fire_map(self, e):
        if self._maps is None:
            if hasattr(self.eng, "fire_maps"):
                self._maps = self.eng.fire_maps()
            else:
                self._maps = np.stack([self.eng.fire_map(i) for i in range(self.eng.n_envs)])
        return self._maps[e]

    def status(self):
        return self.eng.status()

    def apply_mitigation(self, rows):
        self._maps = None
        self.eng.apply_mitigation(rows)

    def step(self, n):
        self._maps = None
        self.eng.step(n)

    def reset_env(self, e, x, y):
        self._maps = None
        self.eng.reset_env(e, x, y)


def make_world(case, n_envs=None):
    """(engine kwargs without n_envs, R table - [E, 8, H, W] with ``per_env`` -, E, ignitions [E, 2], starts [E, K, 2]) of a case.
    ``n_envs``: the value of E = "cu+8"."""
    from test_env_state_gpu import _world
    c = CASES[case]
    H, W, K = c["H"], c["W"], c["K"]
    rng = np.random.default_rng(c["seed"])
    E = int(rng.integers(4, 9))
    if "E" in c:
        E = int(c["E"]) if c["E"] != "cu+8" else int(n_envs if n_envs is not None else E_STAND_IN)
    kw, R8 = _world(rng, H, W, c.get("md", 4), c["att"], diag=c.get("diag", True))
    kw.update(max_time=float(rng.integers(6, 12)), update_rate=1.0)       # every fire that keeps spreading QUITs on the runtime check
    if c.get("max_time") is False:
        kw.update(max_time=None)
    R8[:, : H // 2] = np.maximum(R8[:, : H // 2], 30.0)                    # (the upper half always passes its fire on)
    if "hot" in c:
        R8 = np.maximum(R8, c["hot"])                                      # (fires that take a cell per side and update: large terms)
    # starts on corners and edges; the ignition a few cells from an agent, so that the fire is in reach
    edge = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, 0), (0, H // 2), (W - 1, H // 2), (W // 2, H - 1),
            (15, 0), (16, 0), (min(W - 1, 31), H - 1)]
    edge = c.get("spots", edge)
    starts = np.zeros((E, K, 2), dtype=np.int32)
    inits = np.zeros((E, 2), dtype=np.int32)
    for e in range(E):
        for j in range(K):
            starts[e, j] = edge[int(rng.integers(len(edge)))]
        ax, ay = starts[e, int(rng.integers(K))]
        inits[e] = (int(np.clip(ax + rng.integers(-3, 4), 0, W - 1)), int(np.clip(ay + rng.integers(-3, 4), 0, H - 1)))
    if c.get("per_env"):                                                   # a table of its own for every environment
        tabs = [R8]
        for _ in range(1, E):
            t = _world(rng, H, W, c.get("md", 4), c["att"], diag=c.get("diag", True))[1]
            t[:, : H // 2] = np.maximum(t[:, : H // 2], 30.0)
            tabs.append(t)
        R8 = np.stack(tabs)
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


def drive(case, a, on_tick=None, n_envs=None, twins=(), on_steps=None):
    """Drives engine ``a`` (reset at the case's ignitions) through the case with the oracle; ``on_tick(t, actions, result, oracle)``
    after every tick.  ``twins``: engines that make the case's plain ``step`` calls (``pre_steps``, ``between``) along with ``a``;
    ``on_steps(t)`` after each of those (t = -1: the pre-steps).  Returns what the case saw on handle A alone: ticks with an
    auto-reset, with ``terms[2] > 0``, with ``terms[3] > 0``, with a done report, with an environment found not running, with a
    point emitted, with one refused; agents of running environments below / from the case's ``split`` on; the terms of every tick
    of a running environment."""
    c = CASES[case]
    kw, R8, E, inits, starts = make_world(case, n_envs)
    rng = np.random.default_rng(c["seed"] + 1)
    eng = OneFetch(a) if c.get("one_fetch") else a
    o = AgentsOracle(eng, E, c["H"], c["W"], c["K"], inits, n_updates=c["n_updates"], weights=c["weights"],
                     only_unburned=c["only_unburned"], done_on_burn=c["done_on_burn"], max_ticks=c["max_ticks"],
                     auto_reset=c["auto_reset"])
    o.place(list(range(E)), starts)
    seen = dict(reset=0, in_fire=0, blocked=0, done=0, off=0, emitted=0, refused=0, lo=0, hi=0, terms=[])

    def steps(t, n):
        for x in (eng,) + tuple(twins):
            x.step(n)
        if on_steps is not None:
            on_steps(t)
    if c.get("pre_steps"):
        steps(-1, c["pre_steps"])
    for t in range(c["ticks"]):
        if c.get("between") and t and t % c["between"][0] == 0:
            steps(t, c["between"][1])
        maps = [eng.fire_map(e) for e in range(E)]
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
        seen["terms"] += [tuple(int(v) for v in r["terms"][e]) for e in np.flatnonzero(running)]
        if "split" in c:
            v = r["points"][running][:, :, 1 if c["split"][0] == "row" else 0]          # (where the agents stood after their moves)
            seen["lo"] += int((v < c["split"][1]).sum())
            seen["hi"] += int((v >= c["split"][1]).sum())
        if on_tick is not None:
            on_tick(t, actions, r, o)
    return seen
