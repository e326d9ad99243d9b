"""The cases of ``tests/test_ensemble_gpu.py``: worlds of ``tests/_arrival_worlds.py`` at the shapes at which ``k_ensemble`` can go
wrong, the member layouts, the horizons, and the loop that builds the expected arrival without a device
(``tests/test_ensemble_cpu.py`` checks with it that every case sees what it claims)."""
import numpy as np

from _arrival_oracle import MapArrival
from _arrival_worlds import DenseStandIn, make_world, mode_settings      # noqa: F401  (re-exported for the tests)
from _values_worlds import make_values                                   # noqa: F401

CALLS = (1, 2, 3, 5, 7, 11)               # updates per call; the statistics are taken behind each: after 1, 3, 6, 11, 18, 29 updates
MID = 12                                  # a horizon inside the episode
BEYOND = 1000                             # a horizon beyond every member's update count

# shape -> what it exercises: W % 4 == 0 (16-byte stores) | W % 4 == 1, pitch 32, narrow rows | W % 4 == 2, pitch over 1024, E = 3 |
# behind the window launch | behind the team launch
CASES = {
    "24x40": dict(modes=("fused0", "run")),
    "33x17": dict(modes=("fused0", "run")),
    "70x1030_wide": dict(modes=("auto",)),
    "72x80_win": dict(modes=("run_win",)),
    "136x64_team": dict(modes=("run_team",)),
}
PAIRS = [(case, mode) for case in CASES for mode in CASES[case]["modes"]]

# the wide world's own ignitions lie hundreds of columns apart: its fires never meet.  These are within a dozen cells of each other.
WIDE_IGNITIONS = np.array([[512, 34], [520, 30], [507, 39]], dtype=np.int32)

HORIZONS = {
    1: ((-1,), (MID,)),
    3: ((0, MID, -1), (0, 6, BEYOND)),
    8: ((0, 1, 3, 6, MID, 20, BEYOND, -1), (0, 2, 4, 6, 9, MID, 21, BEYOND)),
}


def world(case):
    """``_arrival_worlds.make_world`` with the ignitions this file uses."""
    kw, R8, E, inits = make_world(case)
    if case == "70x1030_wide":
        assert E == len(WIDE_IGNITIONS)
        inits = WIDE_IGNITIONS.copy()
    return kw, R8, E, inits


def layouts(E):
    """name -> int32 [G, K]: one group of all; three groups of five with an environment in two groups and a duplicate inside one;
    K = 1; K = 3, 6, 7 (the tail of the unrolled loop); K = 67 by listing environments again and again (more members than a wave
    has lanes, counts above E)."""
    out = {"all": np.arange(E).reshape(1, E)}
    out["g3k5"] = np.array([[0, 1, 2 % E, 3 % E, 1], [(2 * i + 1) % E for i in range(5)], [E - 1, 0, 0, 1, 2 % E]])
    out["k1"] = np.arange(E).reshape(E, 1)
    for K in (3, 6, 7):
        out["k%d" % K] = np.array([[(i * i + g) % E for i in range(K)] for g in range(2)])
    out["k67"] = np.array([[(5 * i + i // E) % E for i in range(67)]])
    return {k: np.ascontiguousarray(v, dtype=np.int32) for k, v in out.items()}


def horizons_at(moment, j):
    """The horizons of layout number ``j`` behind call ``moment``: T cycles through 1, 3, 8 so that every layout meets every T."""
    T = (1, 3, 8)[(moment + j) % 3]
    return HORIZONS[T][(moment // 3) % 2]


def expected_arrivals(case):
    """[(updates made, int32 [E, H, W])] behind every call of ``CALLS``, from ``oracle/fire_dense`` stepped one update at a time."""
    kw, R8, E, inits = world(case)
    H, W = kw["shape"]
    a = DenseStandIn(kw, R8, E)
    exp = MapArrival(E, H, W)
    a.reset(inits)
    for e in range(E):
        exp.see(e, a.fire_map(e), 0)
    out, updates = [], 0
    for n in CALLS:
        for _ in range(n):
            a.step(1)
            updates += 1
            st = a.status()[0]
            for e in range(E):
                exp.see(e, a.fire_map(e), st[e, 1])
        out.append((updates, exp.exp.copy()))
    return out


# ------------------------------------------------------------------ the two scripted episodes (on the 24 x 40 world)
SCRIPT_CASE = "24x40"
RECIPE_CALLS = (2, 3, 5)                  # the calls behind the fork, control lines of its own for every member in each update


def recipe_points(E, inits):
    """[int32 [n, E, 6, 3]] per call of ``RECIPE_CALLS``: (column, row, type) - six fire-line cells per member and update, drawn
    within 8 cells of environment 0's ignition, different for every member."""
    H, W = make_world(SCRIPT_CASE)[0]["shape"]
    rng = np.random.default_rng(7201)
    x0, y0 = int(inits[0][0]), int(inits[0][1])
    out = []
    for n in RECIPE_CALLS:
        x = np.clip(x0 + rng.integers(-8, 9, size=(n, E, 6)), 0, W - 1)
        y = np.clip(y0 + rng.integers(-8, 9, size=(n, E, 6)), 0, H - 1)
        out.append(np.stack([x, y, np.full_like(x, 3)], axis=-1).astype(np.int32))
    return out


def ring(x, y):
    """The eight neighbours of (x, y) as fire-line points: a fire ignited inside never leaves."""
    return [(x + dx, y + dy, 3) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy) != (0, 0)]


OUT_OF_STEP = dict(first=18, reset=(1, 3), xy=((30, 5), (20, 12)), ringed=3, then=(2, 8, 3))


def recipe_expected():
    """What the counterfactual recipe leaves on ``oracle/fire_dense``: int32 [E, H, W] arrival after 4 updates, a fork of
    environment 0 into all others and the calls of ``recipe_points``."""
    kw, R8, E, inits = world(SCRIPT_CASE)
    H, W = kw["shape"]
    a, exp = DenseStandIn(kw, R8, E), MapArrival(E, H, W)
    a.reset(inits)

    def see():
        st = a.status()[0]
        for e in range(E):
            exp.see(e, a.fire_map(e), st[e, 1])
    see()
    for _ in range(4):
        a.step(1)
        see()
    a.copy_envs([0] * (E - 1), list(range(1, E)))
    exp.exp[1:] = exp.exp[0]
    for pts in recipe_points(E, inits):
        for s in range(pts.shape[0]):
            a.apply_mitigation([(e, int(x), int(y), int(t)) for e in range(E) for (x, y, t) in pts[s, e]])
            a.step(1)
            see()
    return exp.exp


def out_of_step_expected():
    """[(running flags, update counts, arrival)] behind each call of ``OUT_OF_STEP["then"]`` on ``oracle/fire_dense``."""
    kw, R8, E, inits = world(SCRIPT_CASE)
    H, W = kw["shape"]
    o = OUT_OF_STEP
    a, exp = DenseStandIn(kw, R8, E), MapArrival(E, H, W)
    a.reset(inits)

    def see(envs=range(E)):
        st = a.status()[0]
        for e in envs:
            exp.see(e, a.fire_map(e), st[e, 1])
    see()
    for _ in range(o["first"]):
        a.step(1)
        see()
    for e, (x, y) in zip(o["reset"], o["xy"]):
        a.reset_env(e, x, y)
        exp.restart(e)
    see(o["reset"])
    a.apply_mitigation([(o["ringed"], x, y, t) for (x, y, t) in ring(*o["xy"][o["reset"].index(o["ringed"])])])
    out = []
    for n in o["then"]:
        for _ in range(n):
            a.step(1)
            see()
        st = a.status()[0]
        out.append((st[:, 0].copy(), st[:, 1].copy(), exp.exp.copy()))
    return out
