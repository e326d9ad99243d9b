"""Wind changes during an episode on the GPU (``sf_set_wind``, ``sf_set_wind_schedule``).

- tables: after ``set_wind`` the table of every listed environment equals, bit for bit, that of a fresh handle given the same
  planes through ``set_layers(env=e)``; unlisted tables keep their bytes; the wind planes show the new wind;
- episodes: step, ``set_wind``, step - in every launch structure, against ``_per_env_oracle`` fed the device's own tables at each
  stage (the common-table protocol): map, burn_amounts, status rows and elapsed time, bit for bit;
- schedules against the oracle applying the call-boundary rule, through resets, forks, restores and ``BatchedFireEnv`` restarts;
- the refusals, and the Python surface."""
import numpy as np
import pytest

from _per_env_oracle import PerEnvOracle
from simfire_amd import _lib
from simfire_amd.engine import FireEngine
from simfire_amd.parameters import fuel_planes
from simfire_amd.workloads import perlin_elevation

pytestmark = pytest.mark.gpu

M_F = 0.03


def _planes(seed, H, W, E):
    """Per environment (w_0, delta, M_x, sigma, elevation, U, U_dir): different fuel mosaics with a patch of w_0 = 0, perlin
    elevation, a wind field."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    out = []
    for e in range(E):
        codes = rng.choice([1, 2, 4, 5, 8, 9, 10], size=(H, W))
        w0, de, mx, sg = fuel_planes(codes)
        w0 = w0.copy()
        py, px = int(rng.integers(0, H - 3)), int(rng.integers(0, W - 3))
        w0[py:py + 3, px:px + 3] = 0.0
        el = perlin_elevation(H, W, 3, 0.7, 2.0, 800 + e, 100.0, 900.0)
        U = 600.0 + 300.0 * np.sin(x / 7.0 + e)
        Ud = 40.0 * e + 25.0 * np.cos(y / 5.0)
        out.append([w0, de, mx, sg, el, U, Ud])
    return out


def _engine(H, W, planes, **kw):
    kw = dict(dict(pixel_scale=30.0, max_fire_duration=4, M_f=M_F), **kw)
    eng = FireEngine((H, W), n_envs=len(planes), per_env_terrain=True, **kw)
    for e, p in enumerate(planes):
        eng.set_layers(*p, env=e)
    return eng


def _fresh_table(H, W, p, U, Ud, **kw):
    """The table a fresh handle builds from environment planes ``p`` with wind (U, Ud), through set_layers(env=e)."""
    kw = dict(dict(pixel_scale=30.0, max_fire_duration=4, M_f=M_F), **kw)
    ref = FireEngine((H, W), n_envs=2, per_env_terrain=True, **kw)
    ref.set_layers(*p[:5], U, Ud, env=1)
    return ref.get_rtable(1)


def _winds(kind, n, H, W, seed):
    """``n`` winds: uniform (U, U_dir) pairs - with U = 0 and the directions -30 and 725 degrees among them - or fields that hold
    those values in places."""
    rng = np.random.default_rng(seed)
    U = rng.uniform(200.0, 2500.0, n)
    D = rng.uniform(0.0, 360.0, n)
    U[0], D[0] = 0.0, 10.0
    if n > 1:
        D[1] = -30.0
    if n > 2:
        D[2] = 725.0
    if kind == "uniform":
        return U, D
    y, x = np.mgrid[0:H, 0:W]
    FU = np.stack([np.abs(u * np.sin(x / 9.0 + i) + 40.0 * np.cos(y / 3.0)) for i, u in enumerate(U)])
    FD = np.stack([d + 200.0 * np.sin(y / 11.0) * np.cos(x / 6.0 + i) for i, d in enumerate(D)])
    FU[:, : H // 3, : W // 4] = 0.0
    FD[:, 0, 0], FD[:, -1, -1] = -30.0, 725.0
    return np.ascontiguousarray(FU), np.ascontiguousarray(FD)


def _give(eng, U, D, envs, source):
    if source == "cuda":
        import torch
        dev = f"cuda:{eng.params.device}"
        eng.set_wind(torch.tensor(U, dtype=torch.float64, device=dev), torch.tensor(D, dtype=torch.float64, device=dev), envs)
    else:
        eng.set_wind(U, D, envs)


def _check_tables(eng, planes, envs, U, D, before, tag):
    H, W = eng.H, eng.W
    for i, e in enumerate(envs):
        want = _fresh_table(H, W, planes[e], U[i], D[i])
        got = eng.get_rtable(e)
        assert (got == want).all(), (tag, e, int((got != want).sum()))
        a = eng.attribute_data(e)
        assert (a["wind_speed"] == np.broadcast_to(U[i], (H, W))).all() and (a["wind_direction"] == np.broadcast_to(D[i], (H, W))).all(), (tag, e)
    for e in range(eng.n_envs):
        if e not in envs:
            assert (eng.get_rtable(e) == before[e]).all(), (tag, e, "an unlisted table changed")


@pytest.mark.parametrize("source", ["host", "cuda"])
@pytest.mark.parametrize("kind", ["uniform", "field"])
@pytest.mark.parametrize("shape", [(37, 101), (19, 300), (225, 225)], ids=lambda s: "%dx%d" % s)
def test_tables_bit_for_bit(shape, kind, source):
    """37x101: pitch pad columns; 19x300: a row wider than one 256-thread block; 225x225.  Five tables, an out-of-order subset."""
    H, W = shape
    planes = _planes(11, H, W, 5)
    eng = _engine(H, W, planes)
    before = [eng.get_rtable(e) for e in range(5)]
    envs = [3, 0, 4]
    U, D = _winds(kind, 3, H, W, 5)
    _give(eng, U, D, envs, source)
    _check_tables(eng, planes, envs, U, D, before, "first")
    for e, i in ((3, 0), (0, 1), (4, 2)):           # the planes as they stand now
        planes[e][5], planes[e][6] = np.broadcast_to(U[i], (H, W)).copy(), np.broadcast_to(D[i], (H, W)).copy()
    if shape != (225, 225):
        return
    # once more with the cell-major copy live: a resident launch (its window phase reads that copy) ran before ...
    kw = dict(shape=(H, W), max_fire_duration=4, pixel_scale=30.0, update_rate=1.0, max_time=None, attenuate_line_ros=True, diagonal_spread=True)
    o = PerEnvOracle(n_envs=5, **kw)
    xy = np.array([[100, 100], [20, 30], [200, 50], [112, 180], [64, 64]], dtype=np.int32)
    for e in range(5):
        o.set_rtable(eng.get_rtable(e), env=e)
    eng.set_fused(2)
    eng.set_tuning(run_window=3)
    eng.reset(xy)
    o.reset(xy)
    eng.step(3)
    o.step(3)
    assert eng.last_launch_kind() == 2
    before = [eng.get_rtable(e) for e in range(5)]
    envs = [4, 1]
    U, D = _winds(kind, 2, H, W, 6)
    _give(eng, U, D, envs, source)
    _check_tables(eng, planes, envs, U, D, before, "rtc live")
    for e in envs:
        o.set_rtable(eng.get_rtable(e), env=e)
    eng.step(5)                                     # ... then a resident launch must match the oracle (a stale cell-major copy would not)
    o.step(5)
    assert eng.last_launch_kind() == 2
    for e in range(5):
        assert (eng.fire_map(e) == o.fire_map(e)).all() and (eng.burn(e) == o.burn(e)).all(), e
    # ... and once more after generate_layers changed the fuel of one listed table (a stale cache)
    for i, e in enumerate(envs):
        planes[e][5], planes[e][6] = np.broadcast_to(U[i], (H, W)).copy(), np.broadcast_to(D[i], (H, W)).copy()
    eng.generate_layers([1], fuel=(0.3, 2.5, 0.25, 1600.0))
    for k, v in enumerate((0.3, 2.5, 0.25, 1600.0)):
        planes[1][k] = np.full((H, W), v)
    before = [eng.get_rtable(e) for e in range(5)]
    envs = [1, 2]
    U, D = _winds(kind, 2, H, W, 7)
    _give(eng, U, D, envs, source)
    _check_tables(eng, planes, envs, U, D, before, "stale cache")


def test_shared_terrain_handle():
    H, W = 37, 101
    p = _planes(3, H, W, 1)[0]
    eng = FireEngine((H, W), n_envs=3, pixel_scale=30.0, max_fire_duration=4, M_f=M_F)
    eng.set_layers(*p)
    eng.set_wind(1234.5, 300.0)
    want = _fresh_table(H, W, p, 1234.5, 300.0)
    assert (eng.get_rtable(0) == want).all() and (eng.get_rtable(2) == want).all()
    assert (eng.attribute_data(1)["wind_speed"] == 1234.5).all()
    with pytest.raises(_lib.SimfireHipError):
        eng.set_wind(100.0, 0.0, envs=[0])            # a list on a shared-terrain handle
    with pytest.raises(_lib.SimfireHipError):
        eng.set_wind_schedule([0], [(0, 100.0, 0.0)])
    assert (eng.get_rtable(0) == want).all()


# ------------------------------------------------------------------------------------------------------------ episodes
MODES = {"fused0": dict(fused=0), "fused1": dict(fused=1), "run": dict(fused=2),
         "kwin": dict(fused=-1, tuning=dict(run_compact=2, run_window=1))}        # (as tests/test_hip_resident.py forces them)
EH, EW, EE = 72, 80, 4
EKW = dict(shape=(EH, EW), max_fire_duration=4, pixel_scale=30.0, update_rate=1.0, max_time=None, attenuate_line_ros=True, diagonal_spread=True)
EXY = np.array([[40, 36], [10, 12], [60, 50], [33, 20]], dtype=np.int32)


def _lines(seed):
    rng = np.random.default_rng(seed)
    pts = []
    for e in range(EE):
        x0, y0 = EXY[e]
        pts += [(e, int(np.clip(x0 + 3, 0, EW - 1)), int(np.clip(y0 + d, 0, EH - 1)), int(rng.integers(3, 6))) for d in range(-4, 5)]
        pts += [(e, int(np.clip(x0 + d, 0, EW - 1)), int(np.clip(y0 - 3, 0, EH - 1)), int(rng.integers(3, 6))) for d in range(-4, 5)]
    return pts


def _mode(eng, mode):
    eng.set_fused(MODES[mode]["fused"])
    if "tuning" in MODES[mode]:
        eng.set_tuning(**MODES[mode]["tuning"])


def _same(eng, o, tag):
    for e in range(eng.n_envs):
        assert (eng.fire_map(e) == o.fire_map(e)).all(), (tag, e, "map")
        assert (eng.burn(e) == o.burn(e)).all(), (tag, e, "burn")
    st, el = eng.status()
    so, eo = o.status()
    assert (st == so).all() and (el == eo).all(), (tag, "status")


@pytest.mark.parametrize("variant", ["plain", "arrival", "async"])
@pytest.mark.parametrize("mode", list(MODES))
def test_episode_step_set_wind_step(mode, variant):
    planes = _planes(21, EH, EW, EE)
    eng = _engine(EH, EW, planes, **{k: v for k, v in EKW.items() if k not in ("shape", "max_fire_duration", "pixel_scale")})
    _mode(eng, mode)
    if variant == "arrival":
        eng.enable_arrival(True)
    if variant == "async":
        eng.set_async(True)
    o = PerEnvOracle(n_envs=EE, **EKW)
    for e in range(EE):
        o.set_rtable(eng.get_rtable(e), env=e)
    eng.reset(EXY)
    o.reset(EXY)
    pts = _lines(5)
    eng.apply_mitigation(pts)
    o.apply_mitigation(pts)
    kinds = []
    for n in (2, 2):                               # a = 4 updates
        eng.step(n)
        o.step(n)
        kinds.append(eng.last_launch_kind())
    _same(eng, o, "before")
    envs = [2, 0, 3]
    U, D = _winds("uniform" if mode in ("fused0", "run") else "field", 3, EH, EW, 31)
    U = U + 1500.0                                  # (winds that move the fire on)
    eng.set_wind(U, D, envs)
    for e in envs:
        o.set_rtable(eng.get_rtable(e), env=e)
    for n in (2, 3, 2):                            # b = 7 updates
        eng.step(n)
        o.step(n)
        kinds.append(eng.last_launch_kind())
    _same(eng, o, "after")
    want = {"fused0": {0, 1}, "fused1": {1}, "run": {2}, "kwin": {2, 4}}[mode]
    assert set(kinds) <= want and (mode != "kwin" or variant == "arrival" or 4 in kinds), kinds
    if variant == "arrival":
        for e in range(EE):
            a, m = eng.arrival(e), eng.fire_map(e)
            assert ((a >= 0) == ((m == 1) | (m == 2))).all(), e


# ------------------------------------------------------------------------------------------------------------ schedules
SH, SW = 40, 48
SKW = dict(shape=(SH, SW), max_fire_duration=4, pixel_scale=30.0, update_rate=1.0, max_time=None, attenuate_line_ros=True, diagonal_spread=True)
SCHED = [[(0, 900.0, 90.0), (4, 2200.0, 270.0), (9, 1500.0, 0.0)],
         [(0, 1800.0, 180.0), (2, 700.0, 45.0), (13, 2500.0, 300.0)],
         [(0, 0.0, 0.0), (5, 2000.0, -30.0), (6, 1200.0, 725.0)],
         [(0, 2400.0, 10.0), (7, 2400.0, 190.0), (16, 600.0, 100.0)]]
SXY = np.array([[20, 20], [8, 30], [40, 10], [24, 5]], dtype=np.int32)


class _Sched:
    """The oracle side of a scheduled handle: the call-boundary rule.  In front of every stepping call the segment of each
    environment's update count decides its table (built by a fresh handle through set_layers); the call then runs under it."""

    def __init__(self, planes, sched):
        self.planes, self.sched = planes, [list(s) for s in sched]
        self.o = PerEnvOracle(n_envs=len(planes), **SKW)
        self.seg = [None] * len(planes)
        self._tab = {}

    def table(self, e, k):
        if (e, k) not in self._tab:
            _, U, D = self.sched[e][k]
            self._tab[(e, k)] = _fresh_table(SH, SW, self.planes[e], U, D)
        return self._tab[(e, k)]

    def step(self, n):
        steps = self.o.status()[0][:, 1]
        for e in range(len(self.planes)):
            k = max(i for i, r in enumerate(self.sched[e]) if r[0] <= steps[e])
            if k != self.seg[e]:
                self.seg[e] = k
                self.o.set_rtable(self.table(e, k), env=e)
        self.o.step(n)


def _sched_pair(mode="fused0"):
    planes = _planes(41, SH, SW, 4)
    eng = _engine(SH, SW, planes, attenuate_line_ros=True)
    _mode(eng, mode)
    eng.set_wind_schedule(None, SCHED)
    s = _Sched(planes, SCHED)
    for e in range(4):
        s.o.set_rtable(eng.get_rtable(e), env=e)       # (until its first stepping call a table is what the layers made it)
    eng.reset(SXY)
    s.o.reset(SXY)
    return eng, s


def _sched_same(eng, s, tag):
    _same(eng, s.o, tag)
    for e in range(eng.n_envs):
        assert (eng.get_rtable(e) == s.table(e, s.seg[e])).all(), (tag, e, "table")


@pytest.mark.parametrize("mode", ["fused0", "run"])
def test_schedule_follows_the_call_boundary_rule(mode):
    eng, s = _sched_pair(mode)
    t = 0
    for i, n in enumerate((1, 3, 7, 1, 3, 7)):      # calls of 1, 3 and 7 updates across the boundaries
        eng.step(n)
        s.step(n)
        t += n
        _sched_same(eng, s, (mode, t))
        if i == 2:                                 # an environment reset in the middle returns to segment 0
            eng.reset_envs([1, 3], SXY[[1, 3]])
            for e in (1, 3):
                s.o.reset_env(e, *SXY[e])
    assert s.seg[1] < 2 and s.seg[0] == 2, s.seg
    # a wind set by hand ends the schedule of that environment only
    eng.set_wind(1000.0, 33.0, envs=[2])
    s.sched[2] = [(0, 1000.0, 33.0)]
    s.seg[2] = None
    s._tab = {k: v for k, v in s._tab.items() if k[0] != 2}
    eng.step(4)
    s.step(4)
    _sched_same(eng, s, (mode, "by hand"))


def test_schedule_clone_and_restore():
    eng, s = _sched_pair("run")
    for n in (3, 3):
        eng.step(n)
        s.step(n)
    # with the terrain: environment 2 becomes environment 0 - state, table, schedule and the segment the table stands for
    eng.copy_envs([0], [2], terrain=True)
    s.o.copy_env(0, 2, terrain=True)
    s.planes[2], s.sched[2], s.seg[2] = s.planes[0], list(s.sched[0]), s.seg[0]
    s._tab = {k: v for k, v in s._tab.items() if k[0] != 2}
    # without: environment 3 goes on from environment 1's state over its own terrain, under its own schedule
    eng.copy_envs([1], [3], terrain=False)
    s.o.copy_env(1, 3, terrain=False)
    # get_state / set_state: environment 1 goes back to an earlier update count, the next call decides its segment anew
    blob = eng.save_state([1])
    log = list(s.o._log[1])
    for n in (2, 5):
        eng.step(n)
        s.step(n)
        _sched_same(eng, s, ("clone", n))
    eng.step(7)
    s.step(7)
    assert s.seg[1] == 2
    eng.load_state([1], blob)
    twin = PerEnvOracle(n_envs=4, **SKW)
    twin._log[1] = log
    s.o.copy_env(1, 1, terrain=True, source=twin)
    s.seg[1] = None
    eng.step(2)
    s.step(2)
    assert s.seg[1] == 1
    _sched_same(eng, s, "restore")


def _simple_dict(H, W, mph, deg):
    import test_layer_gen_gpu as TL
    d = TL._dict(H, W)
    d["wind"] = {"function": "simple", "simple": {"speed": mph, "direction": deg}}
    return d


def test_vecenv_restart_returns_to_the_first_segment():
    """An episode that ends and restarts inside ``BatchedFireEnv.step`` runs its next episode under segment 0's wind: the restart is
    picked up by the next tick (table read-back after it)."""
    import torch
    from simfire_amd.config import Config
    from simfire_amd.simulation import BatchedFireSimulation
    from simfire_amd.vecenv import BatchedFireEnv
    H, W, E = 24, 40, 3
    sim = BatchedFireSimulation(Config(config_dict=_simple_dict(H, W, 7, 90.0), simplex_topography=True), E, ignitions=[[5, 5], [20, 12], [30, 8]],
                                per_env_terrain=True)
    env = BatchedFireEnv(sim, 2, np.array([[0, 0], [39, 23]]), n_updates=1, max_ticks=3, auto_reset=True)
    rows = [(0, 10, 90.0), (2, 25, 270.0)]
    env.set_wind_schedule(None, rows)
    eng = sim._engine
    built = lambda mph, deg: BatchedFireSimulation(Config(config_dict=_simple_dict(H, W, mph, deg), simplex_topography=True), 1,
                                                   ignitions=[[5, 5]])._engine.get_rtable(0)
    tabs = [built(r[1], r[2]) for r in rows]
    act = torch.zeros((E, 2), dtype=torch.int32, device=f"cuda:{eng.params.device}")
    seen = []
    for tick in range(1, 6):
        _, _, done, _ = env.step(act)
        seen.append(int(0 if (eng.get_rtable(1) == tabs[0]).all() else (1 if (eng.get_rtable(1) == tabs[1]).all() else -1)))
        assert bool(done.all().item()) == (tick == 3), tick
    # ticks 1, 2 start at update counts 0, 1 (segment 0), tick 3 at 2 (segment 1); the restart inside tick 3 is seen by tick 4
    assert seen == [0, 0, 1, 0, 0], seen
    env.set_wind(12, 45.0, envs=[1])                # the pass-through; it ends the schedule of environment 1
    env.step(act)                                   # (tick 3 of the second episode: update count 2)
    assert (eng.get_rtable(1) == built(12, 45.0)).all() and (eng.get_rtable(0) == tabs[1]).all()


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    import torch
    H, W = 24, 40
    planes = _planes(5, H, W, 3)
    eng = FireEngine((H, W), n_envs=3, per_env_terrain=True, pixel_scale=30.0)
    for e in (0, 1):
        eng.set_layers(*planes[e], env=e)
    eng.set_rtable(np.full((8, H, W), 5.0), env=2)   # a table without layers
    before = [eng.get_rtable(e) for e in range(3)]
    with pytest.raises(ValueError):
        eng.set_wind([1.0, 2.0], [0.0, 0.0], envs=[1, 1])                 # repeated environment
    with pytest.raises(ValueError):
        eng.set_wind([1.0], [0.0], envs=[3])                              # out of range
    with pytest.raises(_lib.SimfireHipError):
        eng.set_wind([1.0, 2.0], [0.0, 0.0], envs=[0, 2])                 # no layers
    with pytest.raises(ValueError):
        eng.set_wind_schedule([0], [(i, 100.0, 0.0) for i in range(17)])  # K = 17
    with pytest.raises(ValueError):
        eng.set_wind_schedule([0], [(0, 100.0, 0.0), (3, 100.0, 0.0), (3, 200.0, 0.0)])      # not increasing
    with pytest.raises(ValueError):
        eng.set_wind_schedule([0], [(1, 100.0, 0.0)])                     # does not start at update 0
    L = eng._L
    u = np.zeros(2)
    e01 = np.array([0, 1], dtype=np.int32)
    assert L.sf_set_wind(eng._h, 2, e01.ctypes.data, u.ctypes.data, u.ctypes.data, 4) == _lib.SF_EINVAL        # unknown flag bits
    assert L.sf_set_wind(eng._h, 2, e01.ctypes.data, None, u.ctypes.data, 0) == _lib.SF_EINVAL                 # null pointer
    assert L.sf_set_wind(eng._h, 2, None, u.ctypes.data, u.ctypes.data, 0) == _lib.SF_EINVAL                   # no list: n must be 3
    assert L.sf_set_wind(eng._h, 0, None, None, None, 0) == _lib.SF_OK                                         # n == 0 does nothing
    dev = f"cuda:{eng.params.device}"
    t = torch.zeros((2, H, 2 * W), dtype=torch.float64, device=dev)
    with pytest.raises(ValueError):
        eng.set_wind(t[:, :, ::2], t[:, :, ::2], envs=[0, 1])            # not contiguous
    f = torch.zeros((2, H, W), dtype=torch.float32, device=dev)
    with pytest.raises(ValueError):
        eng.set_wind(f, f, envs=[0, 1])                                   # float32
    for e in range(3):
        assert (eng.get_rtable(e) == before[e]).all(), e
    # the closed loop is refused while a schedule is set, and allowed again once it is cleared
    eng.set_layers(*planes[2], env=2)
    eng.reset([(5, 5), (6, 6), (7, 7)])
    eng.set_wind_schedule([1], [(0, 100.0, 0.0), (5, 900.0, 90.0)])
    with pytest.raises(NotImplementedError):
        eng.loop_start(1)
    eng.set_wind_schedule([1], [])
    eng.loop_start(1)
    eng.loop_stop()


# ------------------------------------------------------------------------------------------------------------ Python surface
def test_batched_set_wind_equals_a_batch_built_from_configs():
    from simfire_amd.config import Config
    from simfire_amd.simulation import BatchedFireSimulation
    H, W, E = 37, 53, 3
    winds = [(7, 90.0), (23.5, 200.0), (11, 355.0)]
    cfgs = lambda ws: [Config(config_dict=_simple_dict(H, W, *w), simplex_topography=True) for w in ws]
    want = BatchedFireSimulation(cfgs(winds), E, ignitions=[[5, 5]] * E)
    sim = BatchedFireSimulation(cfgs([(3, 10.0)] * E), E, ignitions=[[5, 5]] * E)
    sim.set_wind([w[0] for w in winds], [w[1] for w in winds])
    for e in range(E):
        assert (sim._engine.get_rtable(e) == want._engine.get_rtable(e)).all(), e
    sim.set_wind(5, 60.0, envs=[2])
    one = BatchedFireSimulation(cfgs([(5, 60.0)] * 2), 2, ignitions=[[5, 5]] * 2)
    assert (sim._engine.get_rtable(2) == one._engine.get_rtable(0)).all()
    assert (sim._engine.get_rtable(1) == want._engine.get_rtable(1)).all()


def test_fire_simulation_set_wind_then_run():
    from oracle import fire_dense
    from simfire_amd.config import Config
    from simfire_amd.simulation import FireSimulation
    H, W = 37, 53
    d = _simple_dict(H, W, 20, 90.0)
    sim = FireSimulation(Config(config_dict=d, simplex_topography=True))
    eng = sim._engine
    kw = dict(shape=(H, W), n_envs=1, max_fire_duration=4, pixel_scale=50.0, update_rate=1.0, max_time=24 * 60.0,
              attenuate_line_ros=True, diagonal_spread=True)
    o = fire_dense.DenseOracle(**kw)
    o.set_rtable(eng.get_rtable(0))
    o.reset([(5, 5)])
    sim.run(3)
    o.step(3)
    y, x = np.mgrid[0:H, 0:W]
    sp, dr = 1500.0 + 10.0 * x, 270.0 + 0.0 * y
    sim.set_wind(sp, dr)
    o.set_rtable(eng.get_rtable(0))
    cfg2 = Config(config_dict=d, simplex_topography=True)
    cfg2.wind.speed, cfg2.wind.direction = sp.astype(np.float64), dr
    assert (eng.get_rtable(0) == FireSimulation(cfg2)._engine.get_rtable(0)).all()       # a simulation built with that wind
    fm, _ = sim.run(1)
    o.step(1)
    assert (np.asarray(fm) == o.fire_map(0)).all() and (sim.fire_manager.burn_amounts == o.burn(0)).all()
    data = sim.get_attribute_data()
    assert (data["wind_speed"] == sp).all() and (data["wind_direction"] == dr).all()
    assert (sim.fire_manager.U == sp).all() and (sim.fire_manager.U_dir == dr).all()
    assert (sim.config.wind.speed == sp).all() and (sim.environment.U_dir == dr).all()
    h = eng._h.value
    sim.reset()
    assert sim._engine._h.value == h and (sim._engine.get_rtable(0) == o.get_rtable()).all()      # the handle is kept, the new wind with it
