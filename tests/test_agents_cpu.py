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


def test_gpu_cases_cover_what_they_claim():
    """Every case of ``tests/test_agents_gpu.py`` on handle A alone - ``oracle/fire_dense`` standing in for it: the case sees an
    auto-reset (without auto_reset: a done report and an environment found not running), an agent in the fire, a blocked move, an
    emitted point and, with only_unburned, a refused one."""
    from oracle import fire_dense
    import _agents_worlds as aw
    for case, c in aw.CASES.items():
        kw, R8, E, inits, starts = aw.make_world(case)
        assert 4 <= E <= 8
        a = fire_dense.DenseOracle(n_envs=E, **kw)
        a.set_rtable(R8)
        a.reset(inits)
        seen = aw.drive(case, a)
        assert seen["in_fire"] and seen["blocked"] and seen["emitted"] and seen["done"], (case, seen)
        assert seen["reset"] if c["auto_reset"] else seen["off"], (case, seen)
        if c["only_unburned"]:
            assert seen["refused"], (case, seen)
    on = {k: {c[k] for c in aw.CASES.values()} for k in ("att", "only_unburned", "done_on_burn", "auto_reset")}
    assert all(v == {True, False} for v in on.values()), on
    assert {c["n_updates"] for c in aw.CASES.values()} == {1, 3} and {c["max_ticks"] for c in aw.CASES.values()} == {0, 6}
    assert {c["K"] for c in aw.CASES.values()} == {1, 5, 64}
