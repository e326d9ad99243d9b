"""Agents (``sf_agents_*``) without a GPU: the NumPy restatement of a tick (``tests/_agents_oracle.py``, the
yardstick of the GPU tests) against a scenario worked by hand, and the ctypes binding against the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from _agents_oracle import AgentsOracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class FakeWorld:
    """Maps and result rows for the restatement: ``step`` plays a script {update number: [(env, x, y, status), ...]}."""

    def __init__(self, E, H, W, script):
        self.E, self.H, self.W, self.script = E, H, W, script
        self.maps = np.zeros((E, H, W), dtype=np.uint8)
        self.running = np.ones(E, dtype=np.int32)
        self.steps = np.zeros(E, dtype=np.int32)
        self.t = 0
        self.log = []

    def status(self):
        st = np.zeros((self.E, 8), dtype=np.int32)
        st[:, 0], st[:, 1] = self.running, self.steps
        for e in range(self.E):
            st[e, 2:8] = np.bincount(self.maps[e].ravel(), minlength=6)[:6]
        return st, np.zeros(self.E)

    def fire_map(self, e):
        return self.maps[e].copy()

    def apply_mitigation(self, rows):
        self.log.append(("mit", sorted(rows)))
        for ty in (3, 4, 5):                              # update_mitigation's order: a later type overwrites
            for (e, x, y, t) in rows:
                if t == ty:
                    self.maps[e, y, x] = t

    def step(self, n):
        for _ in range(n):
            self.t += 1
            for (e, x, y, s) in self.script.get(self.t, []):
                if self.running[e] == 1:
                    self.maps[e, y, x] = s
            self.steps += self.running == 1

    def reset_env(self, e, x, y):
        self.log.append(("reset", e, x, y))
        self.maps[e] = 0
        self.maps[e, y, x] = 1
        self.running[e], self.steps[e] = 1, 0


def test_hand_worked_scenario():
    """6 x 7 cells, two environments of four agents, weights (-1, 0.25, -10, -0.5), only_unburned, done_on_burn, auto_reset.
    Tick 1, environment 0: agent 0 walks off the left edge and draws a FIRELINE where it stands, agent 1 walks off the right edge,
    agent 2 steps onto agent 3's cell and draws a SCRATCHLINE, agent 3 draws a WETLINE there (the cell ends as WETLINE); the fire
    takes two cells.  Environment 1 is not running: reported done, untouched by its actions, then re-ignited.  Tick 2, environment
    0: the top and the bottom edge, an invalid action word, and agent 3 steps into the fire where its FIRELINE is refused."""
    H, W, E, K = 6, 7, 2, 4
    script = {1: [(0, 5, 2, 1), (0, 4, 3, 1)], 2: [(0, 5, 1, 2), (0, 4, 4, 1)]}
    w = FakeWorld(E, H, W, script)
    w.maps[0, 1, 5] = 1
    w.maps[1, 2, 2] = 2
    w.running[1] = 0
    ign = [(5, 1), (1, 4)]
    o = AgentsOracle(w, E, H, W, K, ign, n_updates=1, weights=(-1.0, 0.25, -10.0, -0.5), only_unburned=True, done_on_burn=True,
                     max_ticks=0, auto_reset=True)
    start = np.array([[(0, 0), (6, 5), (3, 2), (3, 3)], [(1, 1), (2, 2), (3, 3), (4, 4)]], dtype=np.int32)
    o.place([0, 1], start)

    r = o.step([[3 + 5 * 1, 4, 2 + 5 * 2, 0 + 5 * 3], [1 + 5, 2 + 10, 3 + 15, 4]])
    assert o.pos[0].tolist() == [[0, 0], [6, 5], [3, 3], [3, 3]]
    assert r["points"][0].tolist() == [[0, 0, 3], [6, 5, 0], [3, 3, 4], [3, 3, 5]]
    assert r["points"][1].tolist() == [[1, 1, 0], [2, 2, 0], [3, 3, 0], [4, 4, 0]]          # padding: not running
    assert w.log[0] == ("mit", [(0, 0, 0, 3), (0, 3, 3, 4), (0, 3, 3, 5)])
    assert r["terms"].tolist() == [[2, 3, 0, 2], [0, 0, 0, 0]]
    assert r["reward"].tolist() == [-2.25, 0.0] and r["reward"].dtype == np.float32
    assert r["done"].tolist() == [0, 1]
    assert r["final_len"].tolist() == [0, 0] and r["final_ret"].tolist() == [0.0, 0.0]
    assert w.log[1:] == [("reset", 1, 1, 4)]                                                 # auto_reset of the one that was not running
    assert o.pos[1].tolist() == start[1].tolist()
    assert w.maps[0, 3, 3] == 5 and w.maps[0, 0, 0] == 3 and w.maps[1, 4, 1] == 1 and w.maps[1, 2, 2] == 0

    r = o.step([[1, 2, 99, 4 + 5 * 1], [-3, 0, 20, 0]])
    assert r["points"][0].tolist() == [[0, 0, 0], [6, 5, 0], [3, 3, 0], [4, 3, 0]]            # (4, 3) is BURNING: refused
    assert [x for x in w.log if x[0] == "mit"] == w.log[:1]                                   # no points: no second scatter
    assert r["terms"].tolist() == [[1, 0, 1, 2], [0, 0, 0, 0]]
    assert r["reward"].tolist() == [-12.0, 0.0]
    assert r["done"].tolist() == [1, 0]
    assert r["final_len"].tolist() == [2, 0] and r["final_ret"].tolist() == [-14.25, 0.0]
    assert w.log[2:] == [("reset", 0, 5, 1)]
    assert o.pos[0].tolist() == start[0].tolist() and o.pos[1].tolist() == start[1].tolist()
    assert o.ep_len.tolist() == [0, 1] and o.ep_ret.tolist() == [0.0, 0.0]


def test_without_only_unburned_and_auto_reset():
    """A line on a BURNING cell is emitted (the reference's quirk), max_ticks ends the episode, and nothing is reset."""
    w = FakeWorld(1, 6, 7, {})
    w.maps[0, 2, 2] = 1
    o = AgentsOracle(w, 1, 6, 7, 1, None, n_updates=3, weights=(0.0, 1.0, 0.0, 0.0), only_unburned=False, max_ticks=2, auto_reset=False)
    o.place([0], [[(2, 3)]])
    r = o.step([[1 + 5 * 2]])
    assert r["points"][0].tolist() == [[2, 2, 4]] and w.maps[0, 2, 2] == 4 and w.steps[0] == 3
    assert r["terms"].tolist() == [[-1, 1, 0, 0]] and r["done"].tolist() == [0]              # (the BURNING cell became a line)
    r = o.step([[0]])
    assert r["done"].tolist() == [1] and r["final_len"].tolist() == [2] and r["final_ret"].tolist() == [1.0]
    assert w.log == [("mit", [(0, 2, 2, 4)])] and o.pos[0].tolist() == [[2, 2]] and o.ep_len.tolist() == [2]


def _header():
    return open(os.path.join(ROOT, "include", "simfire_hip.h")).read()


def test_prototypes_are_bound_with_matching_arity():
    from simfire_amd import _lib
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    protos = dict(re.findall(r"\bint\s+(sf_agents_[a-z_]+)\s*\(([^)]*)\)\s*;", code))
    assert set(protos) == {"sf_agents_create", "sf_agents_place", "sf_agents_step", "sf_agents_device"}
    for name, args in protos.items():
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name]) == len([a for a in args.split(",") if a.strip()]), name
    lib = _lib.load()
    for name in protos:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name]


@pytest.mark.parametrize("struct,cls", [("sf_agent_params", "SfAgentParams"), ("sf_agent_out", "SfAgentOut")])
def test_struct_layouts_match_the_header(struct, cls):
    from simfire_amd import _lib
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), code, re.S).group(1)
    size_of = {"int32_t": 4, "float": 4, "double": 8, "uint8_t": 1}
    fields, size = [], 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ty, names = decl.split(None, 1)
        for nm in names.split(","):
            nm = nm.strip()
            ptr = nm.startswith("*")
            m = re.fullmatch(r"\*?\s*(\w+)(?:\[(\d+)\])?", nm)
            fields.append(m.group(1))
            size += 8 if ptr else size_of[ty] * int(m.group(2) or 1)
    ct = getattr(_lib, cls)
    assert [f[0] for f in ct._fields_] == fields
    assert C.sizeof(ct) == size == 40


class _PerEnvDense:
    """``oracle/fire_dense`` with a table per environment: one single-environment oracle each, behind the pre-agent API."""

    def __init__(self, kw, tabs, inits):
        from oracle import fire_dense
        self.n_envs = len(tabs)
        self.o = [fire_dense.DenseOracle(n_envs=1, **kw) for _ in tabs]
        for o, t, xy in zip(self.o, tabs, inits):
            o.set_rtable(t)
            o.reset([xy])

    def status(self):
        st, el = zip(*(o.status() for o in self.o))
        return np.concatenate(st), np.concatenate(el)

    def fire_map(self, e):
        return self.o[e].fire_map(0)

    def apply_mitigation(self, rows):
        for (e, x, y, t) in rows:
            self.o[e].apply_mitigation([(0, x, y, t)])      # (one row at a time keeps the order; update_mitigation's precedence is per type)

    def step(self, n):
        for o in self.o:
            o.step(n)

    def reset_env(self, e, x, y):
        self.o[e].reset_env(0, x, y)


def _dense_handle(case):
    from oracle import fire_dense
    import _agents_worlds as aw
    kw, R8, E, inits, starts = aw.make_world(case)
    if aw.CASES[case].get("per_env"):
        assert all((R8[e] != R8[0]).any() for e in range(1, E))
        return _PerEnvDense(kw, R8, inits), E
    a = fire_dense.DenseOracle(n_envs=E, **kw)
    a.set_rtable(R8)
    a.reset(inits)
    return a, E


# (E, ignitions, the first start, max_time, pixel_scale, sum of the R table) of the four first cases, as drawn before the optional keys existed
_OLD_WORLDS = {
    "24x40_k5_u1_att": (4, [[3, 15], [0, 20], [18, 0], [18, 0]], [15, 0], 11.0, 20.0, 1666698.0),
    "33x17_k64_u3": (5, [[13, 1], [15, 29], [0, 32], [14, 14], [2, 32]], [16, 16], 10.0, 5.0, 1019887.0),
    "24x40_k1_u1_att_t6": (6, [[14, 0], [39, 20], [0, 0], [0, 0], [20, 2], [0, 12]], [15, 0], 10.0, 5.0, 1666447.5),
    "33x17_k5_u3_noreset": (8, [[10, 0], [16, 31], [16, 3], [15, 0], [0, 0], [15, 3], [16, 1], [16, 1]], [16, 0], 6.0, 50.0, 997925.5),
}


def test_the_old_cases_draw_the_worlds_they_always_drew():
    """The optional keys of the new cases leave the rng order of the four first cases alone: E, the ignitions and the first starts
    as they were recorded before the keys existed."""
    import _agents_worlds as aw
    assert tuple(_OLD_WORLDS) == aw.OLD_CASES
    for case in aw.OLD_CASES:
        assert "modes" not in aw.CASES[case] and aw.case_modes(case) == aw.BASE_MODES
        kw, R8, E, inits, starts = aw.make_world(case)
        got = (E, inits.tolist(), starts[0, 0].tolist(), kw["max_time"], kw["pixel_scale"], float(R8.sum()))
        assert got == _OLD_WORLDS[case], (case, got)


def test_gpu_cases_cover_what_they_claim():
    """Every case of ``tests/test_agents_gpu.py`` on handle A alone - ``oracle/fire_dense`` standing in for it: the case sees an
    auto-reset (without auto_reset: a done report and an environment found not running), an agent in the fire, a blocked move, an
    emitted point and, with only_unburned, a refused one; where the case names a ``split`` (the rows either side of the team cut,
    the columns either side of 1024), agents on both sides of it."""
    import _agents_worlds as aw
    for case, c in aw.CASES.items():
        a, E = _dense_handle(case)
        assert (4 <= E <= 8) if "E" not in c else E == (aw.E_STAND_IN if c["E"] == "cu+8" else c["E"])
        seen = aw.drive(case, a)
        assert seen["in_fire"] and seen["blocked"] and seen["emitted"] and seen["done"], (case, seen)
        assert seen["reset"] if c["auto_reset"] else seen["off"], (case, seen)
        if c["only_unburned"]:
            assert seen["refused"], (case, seen)
        if "split" in c:
            assert seen["lo"] and seen["hi"], (case, seen["lo"], seen["hi"])
    old = [aw.CASES[k] for k in aw.OLD_CASES]
    on = {k: {c[k] for c in old} for k in ("att", "only_unburned", "done_on_burn", "auto_reset")}
    assert all(v == {True, False} for v in on.values()), on
    assert {c["n_updates"] for c in old} == {1, 3} and {c["max_ticks"] for c in old} == {0, 6}
    assert {c["K"] for c in old} == {1, 5, 64}
    # the new cases: every base mode name is the mode of some case that proves its launch structure ran
    proved = {m for c in aw.CASES.values() if c.get("engage") for m in c["modes"]}
    assert {"run_team", "run_win", "run_kwin", "auto"} <= proved
    assert {c.get("diag", True) for c in aw.CASES.values()} == {True, False}
    assert {c.get("md", 4) for c in aw.CASES.values()} == {4, 8}


def _rewards(terms, w, how):
    """The reward of every term row under one evaluation rule.  "spec": double, left to right, every operation rounded once, then
    one rounding to float.  "f32": every operation in float.  "fma": double, the three additions contracted
    with their multiplications (one rounding for a * b + c; exact rational arithmetic stands in for the fused operation)."""
    from fractions import Fraction
    out = []
    for t in terms:
        if how == "spec":
            r = w[0] * float(t[0])
            for i in (1, 2, 3):
                r = r + w[i] * float(t[i])
        elif how == "f32":
            f = np.float32
            r = f(w[0]) * f(t[0])
            for i in (1, 2, 3):
                r = f(r + f(f(w[i]) * f(t[i])))
        else:
            r = w[0] * float(t[0])
            for i in (1, 2, 3):
                r = float(Fraction(w[i]) * t[i] + Fraction(r))
        out.append(np.float32(r))
    return np.array(out, dtype=np.float32)


def test_reward_arithmetic_is_told_apart():
    """The term rows of the case with weights that are not exact in binary (-0.1, 1/3, -1e-3, 0.7 on 72 x 80, terms up to the
    hundreds): a reward evaluated in float differs from the specified one (double, left to right, one rounding to float) in at
    least one tick, so the bitwise comparison of the GPU test tells the two apart.

    A contracted evaluation (fused multiply-add) is NOT a different function of these inputs, whatever the seed and the weights:
    a weight is a float widened (24 significant bits), a term is a cell or agent count below 2^20, so every product w * t has at
    most 44 significant bits and is exact in double - a fused a * b + c and a rounded a * b followed by + c then round the same
    exact sum once.  The test asserts that equality on the case's rows and on adversarial ones, instead of a separation that
    cannot exist; -ffp-contract=off in the build is belt and braces, not something a reward can show."""
    import _agents_worlds as aw
    case = "72x80_k5_u2_win"
    c = aw.CASES[case]
    a, E = _dense_handle(case)
    terms = aw.drive(case, a)["terms"]
    w = [float(np.float32(v)) for v in c["weights"]]
    assert max(t[0] for t in terms) >= 100 and len(set(terms)) >= 20, (max(t[0] for t in terms), len(set(terms)))
    spec, f32, fma = (_rewards(terms, w, how) for how in ("spec", "f32", "fma"))
    assert (spec.view(np.uint32) != f32.view(np.uint32)).any()
    assert spec.tobytes() == fma.tobytes()
    rng = np.random.default_rng(96000)
    hard = [tuple(int(v) for v in rng.integers(-(1 << 20), 1 << 20, size=4)) for _ in range(2000)]
    wh = [float(np.float32(v)) for v in (-0.1, 1e8 / 3.0, -1e-7, 0.7)]
    assert _rewards(hard, wh, "spec").tobytes() == _rewards(hard, wh, "fma").tobytes()
    for t in hard[:200]:
        for wi, ti in zip(wh, t):
            from fractions import Fraction
            assert Fraction(wi * float(ti)) == Fraction(wi) * ti          # the product is exact
