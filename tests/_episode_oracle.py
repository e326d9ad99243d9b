"""NumPy ``uint64`` restatement of the draw of DESIGN.md section 19 (``sf_episodes_*``: the parameters of a new episode as a function
of (seed, environment, episode index)), the cases of ``tests/test_episodes_gpu.py`` and the loop that drives them.

Handle A is the reference: any engine with the older, already pinned API, driven by ``tests/_agents_oracle.py``; whenever that
oracle finds an environment done, ``EpisodeOracle`` computes the draw here and A gets ``reset_envs([e], [xy])``, a host
``set_wind`` with the drawn doubles and the oracle's agents their new start cells.  Handle B makes the same ticks with
``agents_step`` under ``episodes_set``.  ``tests/test_episodes_cpu.py`` runs the same loop with ``DenseHandle`` (``oracle/fire_dense``)
standing in for A and no B, to check that every case sees what it claims to cover.  Test infrastructure only."""
import numpy as np

from _agents_oracle import AgentsOracle

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
C1, C2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
SLOT_AGENT, SLOT_U, SLOT_DIR, ATTEMPTS = 64, 128, 129, 64


# ---- the draw with Python integers ...
def mix_int(z):
    z &= M64
    z ^= z >> 30
    z = (z * C1) & M64
    z ^= z >> 27
    z = (z * C2) & M64
    z ^= z >> 31
    return z


def word_int(seed, env, ep, slot):
    return mix_int(mix_int(seed + G * (env + 1)) + G * ((ep << 8) | slot))


# ---- ... and with NumPy uint64 (arrays or scalars; arithmetic wraps modulo 2^64)
def _u64(v):
    if isinstance(v, np.ndarray):
        return v.astype(np.uint64)
    return np.asarray(int(v) & M64, dtype=np.uint64)


def mix(z):
    with np.errstate(over="ignore"):
        z = _u64(z)
        z = z ^ (z >> np.uint64(30))
        z = z * np.uint64(C1)
        z = z ^ (z >> np.uint64(27))
        z = z * np.uint64(C2)
        z = z ^ (z >> np.uint64(31))
    return z


def word(seed, env, ep, slot):
    with np.errstate(over="ignore"):
        inner = mix(_u64(seed) + np.uint64(G) * (_u64(env) + np.uint64(1)))
        return mix(inner + np.uint64(G) * ((_u64(ep) << np.uint64(8)) | _u64(slot)))


def to_int(h, lo, hi):
    """An integer of [lo, hi] from a 32-bit half (uint64 holding a value < 2^32): lo + ((h * (hi - lo + 1)) >> 32)."""
    return lo + ((_u64(h) * np.uint64(hi - lo + 1)) >> np.uint64(32)).astype(np.int64)


def to_double(w, a, b):
    """A double of [a, b) from a word: a + (b - a) * ((w >> 11) * 2^-53), the product rounded before the sum."""
    u = (_u64(w) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    d = np.float64(b - a) * u
    return np.float64(a) + d


def cell(w, box):
    """(x, y) of a box (x0, y0, x1, y1): x from the word's high half over its columns, y from its low half over its rows."""
    w = _u64(w)
    return to_int(w >> np.uint64(32), box[0], box[2]), to_int(w & np.uint64(0xFFFFFFFF), box[1], box[3])


def ignition(seed, env, ep, box, rt=None):
    """The sequential loop the kernel's ballot stands for: attempt a = 0 .. 63 in turn, the first whose cell is not dead (one of the
    eight entries rt[k][y][x] is not 0.0) wins; without a table attempt 0 wins; if none succeeds, attempt 63's cell as it is.
    Returns (x, y, attempts rejected as dead, fell through)."""
    x = y = 0
    for a in range(ATTEMPTS):
        x, y = (int(v) for v in cell(word(seed, env, ep, a), box))
        if rt is None or bool((rt[:, y, x] != 0.0).any()):
            return x, y, a, False
    return x, y, ATTEMPTS, True


def agent_starts(seed, env, ep, box, K):
    xs, ys = cell(word(seed, env, ep, SLOT_AGENT + np.arange(K, dtype=np.uint64)), box)
    return np.stack([xs, ys], axis=1).astype(np.int32)


def wind(seed, env, ep, U, D):
    """(U ft/min, U_dir degrees) as Python floats (IEEE doubles)."""
    return float(to_double(word(seed, env, ep, SLOT_U), U[0], U[1])), float(to_double(word(seed, env, ep, SLOT_DIR), D[0], D[1]))


class EpisodeOracle:
    """The episode buffers of a handle, restated: ``index`` uint32 [E], ``ign`` int32 [E, 2], ``wind`` float64 [E, 2], and what the
    draws saw.  ``rt(e)``: the [8, H, W] table of environment e (``live`` only)."""

    def __init__(self, E, seed, inits, ign_box=None, live=False, wind=None, agent_box=None, K=0, rt=None):
        self.E, self.seed, self.ign_box, self.live, self.wind_rng, self.agent_box, self.K, self.rt = E, int(seed), ign_box, live, wind, agent_box, K, rt
        self.index = np.zeros(E, dtype=np.uint32)
        self.ign = np.array(inits, dtype=np.int32).reshape(E, 2).copy() if ign_box is None else np.zeros((E, 2), dtype=np.int32)
        self.wind = np.zeros((E, 2), dtype=np.float64)
        self.rejected = self.fell = 0
        self.episodes = [[] for _ in range(E)]           # per environment: (x, y, U, U_dir) of every episode drawn

    def draw(self, e):
        """Draws episode ``index[e]`` of environment e.  Returns (x, y, (U, U_dir) or None, starts [K, 2] or None)."""
        ep = int(self.index[e])
        if self.ign_box is not None:
            x, y, rej, fell = ignition(self.seed, e, ep, self.ign_box, self.rt(e) if self.live else None)
            self.rejected += rej
            self.fell += int(fell)
            self.ign[e] = (x, y)
        w = None
        if self.wind_rng is not None:
            w = wind(self.seed, e, ep, *self.wind_rng)
            self.wind[e] = w
        starts = agent_starts(self.seed, e, ep, self.agent_box, self.K) if self.agent_box is not None and self.K else None
        self.index[e] = np.uint32((ep + 1) & 0xFFFFFFFF)
        self.episodes[e].append((int(self.ign[e, 0]), int(self.ign[e, 1])) + (w if w is not None else (None, None)))
        return int(self.ign[e, 0]), int(self.ign[e, 1]), w, starts


class _Restarts:
    """What ``AgentsOracle`` takes for its engine: everything goes to handle A, except that the reset of a done environment is a
    drawn episode - ``reset_envs`` at the drawn cell, the host ``set_wind``, the agents' new start cells."""

    def __init__(self, a, ep):
        self.a, self.ep, self.agents, self.count = a, ep, None, 0

    def status(self):
        return self.a.status()

    def fire_map(self, e):
        return self.a.fire_map(e)

    def apply_mitigation(self, rows):
        self.a.apply_mitigation(rows)

    def step(self, n):
        self.a.step(n)

    def reset_env(self, e, x=None, y=None):               # (x, y: the oracle's fixed ignition - replaced by the draw)
        x, y, w, starts = self.ep.draw(e)
        self.a.reset_envs([e], [[x, y]])
        if w is not None:
            self.a.set_wind(w[0], w[1], envs=[e])
        if starts is not None:
            self.agents.start[e] = starts                 # (the oracle sends the agents there right behind this call: agents_place)
        self.count += 1


# ------------------------------------------------------------------------------------------------------------ cases
# ``world``: "table" - one R table for all environments (tests/test_env_state_gpu.py: _world), "layers" - per-environment layers
# (tests/test_wind_change_gpu.py: _planes).  ``dead``: (x0, y0, x1, y1) whose cells get an all-zero table.  ``few``: the
# environments whose maps and burn amounts are read back (default: all).
CASES = {
    # a dead band over the left half of the ignition box's columns: about every second attempt is rejected
    "24x40_live_agents": dict(H=24, W=40, E=5, K=5, world="table", modes=("fused0", "run"), ign_box=(8, 4, 31, 19), live=True,
                              agent_box=(0, 0, 39, 23), dead=(8, 0, 19, 23), max_ticks=4, n_updates=1, ticks=40, seed=19001),
    "72x80_ign_wind": dict(H=72, W=80, E=4, K=3, world="layers", modes=("run_win",), ign_box=(20, 18, 59, 53),
                           wind=((200.0, 2200.0), (0.0, 360.0)), max_ticks=5, n_updates=2, ticks=40, seed=19002),
    # wind only: the ignition stays, the box is unused
    "33x17_wind": dict(H=33, W=17, E=7, K=2, world="layers", modes=("fused0",), wind=((88.0, 1760.0), (90.0, 270.0)), max_ticks=3,
                       n_updates=1, ticks=40, seed=19003),
    # more environments than one row of 64 of the mask kernels; many restarts fall in one tick
    "24x40_many": dict(H=24, W=40, E=70, K=1, world="table", modes=("run",), ign_box=(0, 0, 39, 23), max_ticks=3, n_updates=1, ticks=14,
                       seed=19004, few=(0, 1, 63, 64, 69)),
    # every cell of the ignition box is dead: attempt 63's cell is taken as it is, and the fire goes out by itself
    "16x16_all_dead": dict(H=16, W=16, E=3, K=2, world="table", modes=("fused0",), ign_box=(4, 4, 11, 11), live=True, dead=(4, 4, 11, 11),
                           max_ticks=6, n_updates=1, ticks=40, seed=19005),
}
PAIRS = [(case, mode) for case in CASES for mode in CASES[case]["modes"]]
WEIGHTS = (-1.0, 0.25, -10.0, -0.5)
LAYER_KW = dict(pixel_scale=30.0, max_fire_duration=4, M_f=0.03)


def make_world(case):
    """dict(kw: engine keyword arguments without n_envs, E, inits [E, 2], starts [E, K, 2], and R8 [8, H, W] or planes [E][7])."""
    from test_env_state_gpu import _world
    c = CASES[case]
    H, W, E, K = c["H"], c["W"], c["E"], c["K"]
    rng = np.random.default_rng(c["seed"])
    out = dict(E=E)
    if c["world"] == "table":
        kw, R8 = _world(rng, H, W, 4, True)
        R8 = np.where(R8.sum(axis=0) == 0.0, 0.0, np.maximum(R8, 12.0))          # fires that go on, around cells that never burn
        if "dead" in c:
            x0, y0, x1, y1 = c["dead"]
            R8[:, y0:y1 + 1, x0:x1 + 1] = 0.0
        kw.update(max_time=None, update_rate=1.0, pixel_scale=10.0)                  # (every live neighbour ignites within an update)
        out.update(kw=kw, R8=R8)
    else:
        from test_wind_change_gpu import _planes
        out.update(kw=dict(LAYER_KW, shape=(H, W), update_rate=1.0, max_time=None, attenuate_line_ros=True, diagonal_spread=True),
                   planes=_planes(c["seed"], H, W, E))
    out["inits"] = np.stack([rng.integers(W // 4, W - W // 4, size=E), rng.integers(H // 4, H - H // 4, size=E)], axis=1).astype(np.int32)
    out["starts"] = np.stack([rng.integers(W, size=(E, K)), rng.integers(H, size=(E, K))], axis=2).astype(np.int32)
    return out


class DenseHandle:
    """Handle A without a device: one ``oracle/fire_dense`` of one environment per environment, with the calls the driver makes.
    In a "layers" world the tables are the oracle's own (libm) tables of the planes and the wind: not the device's bits, which
    does not matter for what the CPU test asks of it."""

    def __init__(self, world):
        from oracle import fire_dense
        self.n_envs, self.planes = world["E"], world.get("planes")
        kw = {k: v for k, v in world["kw"].items() if k != "M_f"}
        self.M_f = world["kw"].get("M_f", 0.03)
        self.o = [fire_dense.DenseOracle(n_envs=1, **kw) for _ in range(self.n_envs)]
        for e, o in enumerate(self.o):
            if self.planes is None:
                o.set_rtable(world["R8"])
            else:
                o.build_rtable(*self.planes[e], self.M_f)
                o.set_rtable(o.get_rtable())

    def reset(self, xy):
        for e, o in enumerate(self.o):
            o.reset([(int(xy[e][0]), int(xy[e][1]))])

    def reset_envs(self, envs, xy):
        for e, p in zip(envs, xy):
            self.o[e].reset([(int(p[0]), int(p[1]))])

    def set_wind(self, U, D, envs):
        for e in envs:
            self.o[e].build_rtable(*self.planes[e][:5], U, D, self.M_f)
            self.o[e].set_rtable(self.o[e].get_rtable())

    def apply_mitigation(self, rows):
        for (e, x, y, t) in rows:
            self.o[e].apply_mitigation([(0, x, y, t)])

    def step(self, n):
        for o in self.o:
            o.step(n)

    def fire_map(self, e):
        return self.o[e].fire_map(0)

    def fire_maps(self):
        return np.stack([o.fire_map(0) for o in self.o])

    def burn(self, e):
        return self.o[e].burn(0)

    def status(self):
        st, el = zip(*(o.status() for o in self.o))
        return np.concatenate(st), np.concatenate(el)


def episode_kwargs(case):
    """The keyword arguments of ``FireEngine.episodes_set`` for a case (the seed is the case's)."""
    c = CASES[case]
    w = c.get("wind")
    return dict(seed=c["seed"], ignition_box=c.get("ign_box"), live_cells=c.get("live", False), wind_speed=None if w is None else w[0],
                wind_direction=None if w is None else w[1], agent_box=c.get("agent_box"))


def drive(case, a, world, b=None, torch=None):
    """Drives A (reset at the world's ignitions) through the case's ticks with the two oracles, B - reset, its agents created and
    placed, ``episodes_set`` called - with ``agents_step``.  After every tick on B: outputs, agent positions, result rows and
    elapsed times, fire maps (of ``few``), ``episodes_torch()`` against the episode oracle with the wind compared as bits; after the
    last tick the wind planes and the burn amounts.  Returns what the case saw."""
    from _agents_worlds import draw_actions
    c = CASES[case]
    H, W, E, K = c["H"], c["W"], c["E"], c["K"]
    rng = np.random.default_rng(c["seed"] + 1)
    rt = None
    if c.get("live"):
        rt = lambda e: world["R8"]
    ep = EpisodeOracle(E, c["seed"], world["inits"], ign_box=c.get("ign_box"), live=c.get("live", False), wind=c.get("wind"),
                       agent_box=c.get("agent_box"), K=K, rt=rt)
    proxy = _Restarts(a, ep)
    o = AgentsOracle(proxy, E, H, W, K, world["inits"], n_updates=c["n_updates"], weights=WEIGHTS, only_unburned=True, done_on_burn=False,
                     max_ticks=c["max_ticks"], auto_reset=True)
    proxy.agents = o
    o.place(list(range(E)), world["starts"])
    few = list(c.get("few", range(E)))
    outs = None
    if b is not None:
        dev = f"cuda:{b.params.device}"
        outs = dict(reward=torch.empty(E, dtype=torch.float32, device=dev), done=torch.empty(E, dtype=torch.uint8, device=dev),
                    terms=torch.empty((E, 4), dtype=torch.int32, device=dev), final_len=torch.empty(E, dtype=torch.int32, device=dev),
                    final_ret=torch.empty(E, dtype=torch.float64, device=dev))
    for t in range(c["ticks"]):
        maps = a.fire_maps() if hasattr(a, "fire_maps") else [a.fire_map(e) for e in range(E)]
        actions = draw_actions(rng, o.pos, maps, H, W)
        want = o.step(actions)
        if b is None:
            continue
        tag = (case, t)
        for v in outs.values():
            v.fill_(77)
        b.agents_step(torch.from_numpy(np.ascontiguousarray(actions, dtype=np.int32)).to(dev), **outs)
        for k in ("terms", "done", "final_len"):
            assert (outs[k].cpu().numpy() == want[k]).all(), (tag, k, outs[k].cpu().numpy(), want[k])
        for k in ("reward", "final_ret"):
            assert outs[k].cpu().numpy().tobytes() == want[k].tobytes(), (tag, k, outs[k].cpu().numpy(), want[k])
        assert (b.agents_device().cpu().numpy() == o.xyid()).all(), (tag, "positions")
        sa, ea = a.status()
        sb, eb = b.status()
        assert (sa == sb).all() and ea.tobytes() == eb.tobytes(), (tag, "status", sa, sb)
        ma, mb = a.fire_maps(), b.fire_maps()
        for e in few:
            assert (ma[e] == mb[e]).all(), (tag, "fire map", e)
        got = {k: v.cpu().numpy() for k, v in b.episodes_torch().items()}
        assert (got["index"].view(np.uint32) == ep.index).all(), (tag, "episode index", got["index"], ep.index)
        assert (got["ignition"] == ep.ign).all(), (tag, "ignition", got["ignition"], ep.ign)
        assert got["wind"].tobytes() == ep.wind.tobytes(), (tag, "wind", got["wind"], ep.wind)
    if b is not None:
        for e in few:
            if c["world"] == "layers":
                da, db = a.attribute_data(e), b.attribute_data(e)
                for k in ("wind_speed", "wind_direction"):
                    assert da[k].tobytes() == db[k].tobytes(), (case, "plane", k, e)
                if ep.episodes[e]:
                    assert (db["wind_speed"] == ep.wind[e, 0]).all() and (db["wind_direction"] == ep.wind[e, 1]).all(), (case, "drawn wind", e)
            assert (a.burn(e) == b.burn(e)).all(), (case, "burn", e)
    return dict(restarts=proxy.count, rejected=ep.rejected, fell=ep.fell, episodes=ep.episodes)
