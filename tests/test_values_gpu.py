"""Values at risk on the GPU (``sf_values_set``).  The yardstick is the API that existed before: handle A runs
the per-step kernels without recording, one update per call, and its maps after every update give the expected arrival
(``tests/_arrival_oracle.py``) over which ``tests/_values_oracle.py`` sums the plane.  Handle B carries the plane, in the mode under
test, and makes the same updates in calls of 1, 2, 3, 5, 7, 11, 23.  Run with ``pytest -m gpu``."""
import ctypes as C

import numpy as np
import pytest

import _values_worlds as vw
from _values_oracle import VALUE_MAX, damage

pytestmark = pytest.mark.gpu


def _engine(kw, E, R8, mode=None):
    from simfire_amd.engine import FireEngine
    eng = FireEngine(n_envs=E, **kw)
    if mode is None:
        eng.set_fused(0)
    else:
        m = vw.mode_settings(mode)
        eng.set_fused(m["fused"])
        if m.get("tuning"):
            eng.set_tuning(**m["tuning"])
    eng.set_rtable(R8)
    return eng


# ------------------------------------------------------------------ 1. the invariant at every API boundary
@pytest.mark.parametrize("case,mode", vw.PAIRS, ids=["%s-%s" % p for p in vw.PAIRS])
def test_damage_matches_the_maps(case, mode):
    """``_values_worlds.drive``: behind the reset, every call and every op of the case (the four resets, fork, snapshot / restore,
    late enabling and a plane set in the middle of an episode) ``damage()`` and ``values_torch()[0]`` equal the plane summed over the
    arrival rebuilt from A's maps, for every environment."""
    import torch
    c = vw.CASES[case]
    kw, R8, E, _ = vw.make_world(case)
    a, b = _engine(kw, E, R8), _engine(kw, E, R8, mode)
    if case == "70x1030_wide":
        assert b.geometry()["pitch"] // 16 > 64              # two bitmap words per row
    seen = vw.drive(case, mode, a, b, torch=torch)
    sparse, dense = b.value_passes()
    kinds = [g for _, g in seen["launches"]]
    print("launches (n, (kind, layout)):", case, mode, seen["launches"], "value passes sparse / dense:", sparse, dense, "damage", seen["total"])
    assert seen["rises"] >= 3
    if mode in ("run", "run_win", "run_team", "run_kwin") and c.get("md", 4) <= 5:
        assert sparse > 0, (sparse, dense)                    # one-word rows behind a resident launch: the bitmap walk
    if mode == "run_noteam":
        assert dense >= len(kinds), (sparse, dense)           # two-word rows in the plain kernel: the dense form behind a resident launch
    if mode in ("fused0", "fused1") or c.get("md", 4) > 5:
        assert sparse <= 1 and dense > 0, (sparse, dense)     # (the pass of a full reset may find the fresh bitmap)
    if "values_at" not in vw.VALUE_CASES[case]:               # the plane from the start: a value pass behind every arrival pass (+ the recounts)
        assert b.arrival_passes()[0] + b.arrival_passes()[1] <= sparse + dense


# ------------------------------------------------------------------ 2. sparse equals dense
@pytest.mark.parametrize("case,mode", [("24x40", "run"), ("72x80_win", "run_win"), ("136x64_team", "run_team"), ("24x40_lines", "run")])
def test_sparse_pass_equals_dense_pass(case, mode):
    """The same world once with the bitmap walk and once with the dense form forced (``set_values_dense``) on a twin handle: the
    damages are equal after each of 10 calls, and they are not trivially zero."""
    kw, R8, E, inits = vw.make_world(case)
    values = vw.make_values(case, E, inits)
    s, d = _engine(kw, E, R8, mode), _engine(kw, E, R8, mode)
    d.set_values_dense(True)
    K = vw.CASES[case].get("lines", 0)
    rng = np.random.default_rng(1)
    for h in (s, d):
        h.reset(inits)
        h.enable_arrival(True)
        h.values_set(values)
    seen = set()
    for i in range(10):
        n = vw.STEPS[i % len(vw.STEPS)]
        if K:
            pts = np.stack([rng.integers(kw["shape"][1], size=(n, E, K)), rng.integers(kw["shape"][0], size=(n, E, K)),
                            rng.choice([0, 3, 4, 5], size=(n, E, K))], axis=-1).astype(np.int32)
        for h in (s, d):
            h.step_mitigated(pts) if K else h.step(n)
            assert (h.last_launch_kind(), h.cell_layout()) == (2, 1)
        ds, dd = s.damage(), d.damage()
        assert (ds == dd).all(), (case, i, ds.tolist(), dd.tolist())
        seen.add(tuple(ds.tolist()))
    assert len(seen) >= 4 and any(any(v != 0 for v in t) for t in seen)
    assert s.value_passes()[0] >= 10 and d.value_passes()[0] == 0, (s.value_passes(), d.value_passes())


# ------------------------------------------------------------------ 3. another plane in the middle of an episode
@pytest.mark.parametrize("case,mode", [("24x40", "run"), ("33x17", "fused0")])
def test_plane_swap(case, mode):
    """``values_set`` with a different plane behind the fifth call: from there on the damage is the oracle's sum under the new
    plane (the shared and the per-environment form)."""
    import torch
    kw, R8, E, _ = vw.make_world(case)
    a, b = _engine(kw, E, R8), _engine(kw, E, R8, mode)
    seen = vw.drive(case, mode, a, b, torch=torch, swap_at=4)
    assert seen["rises"] >= 3


def test_fork_with_planes_per_environment():
    """A fork under per-environment planes: the destination's damage is ITS plane summed over the source's arrival."""
    case = "33x17"
    kw, R8, E, inits = vw.make_world(case)
    values = vw.make_values(case, E, inits)
    a, b = _engine(kw, E, R8), _engine(kw, E, R8, "run")
    for h in (a, b):
        h.reset(inits)
    b.enable_arrival(True)
    b.values_set(values)
    from _arrival_oracle import MapArrival
    exp = MapArrival(E, *kw["shape"])
    for e in range(E):
        exp.see(e, a.fire_map(e), 0)
    for u in range(1, 10):
        a.step(1)
        for e in range(E):
            exp.see(e, a.fire_map(e), a.status()[0][e, 1])
    b.step(9)
    assert (b.damage() == damage(values, exp.exp)).all()
    b.copy_envs([0, 0], [1, 2])
    exp.exp[1] = exp.exp[0]
    exp.exp[2] = exp.exp[0]
    want = damage(values, exp.exp)
    assert (b.damage() == want).all() and len({int(want[0]), int(want[1]), int(want[2])}) == 3, (b.damage().tolist(), want.tolist())


# ------------------------------------------------------------------ 4. off and on
def test_switch_off_and_on():
    """``values_set(None)`` frees the memory: ``memory_bytes()`` is back at its earlier figure and ``damage()`` raises;
    ``enable_arrival(False)`` while a plane is set raises and changes nothing; ``state_bytes()`` and a saved blob's bytes are the
    same with values on and off."""
    from simfire_amd import _lib
    case = "24x40"
    kw, R8, E, inits = vw.make_world(case)
    values = vw.make_values(case, E, inits)
    b = _engine(kw, E, R8, "run")
    b.reset(inits)
    b.enable_arrival(True)
    b.step(5)
    blob0 = b.save_state([0, 1]).tobytes()                      # (first: the staging buffer it grows is counted by memory_bytes)
    mem0, bytes0 = b.memory_bytes(), b.state_bytes()
    b.values_set(values)
    H, W = kw["shape"]
    assert b.memory_bytes() - mem0 >= H * W * 4 + E * 8
    assert b.state_bytes() == bytes0 and b.save_state([0, 1]).tobytes() == blob0
    d = b.damage()
    assert (d == damage(values, np.stack([b.arrival(e) for e in range(E)]))).all() and (d != 0).any()      # (B's own plane: a sanity check only)
    with pytest.raises(_lib.SimfireHipError, match="sf_values_set"):
        b.enable_arrival(False)
    assert b.arrival_on and (b.damage() == d).all() and (b.arrival(0) >= 0).sum() >= 1
    per_env = np.broadcast_to(values, (E, H, W)).copy()
    b.values_set(per_env)                                       # the plane per environment: E planes ...
    assert b.memory_bytes() - mem0 >= E * H * W * 4 and (b.damage() == d).all()
    b.values_set(values)                                        # ... and back to one
    mem1 = b.memory_bytes()
    b.values_set(torch_plane(values))                           # from device memory
    assert b.memory_bytes() == mem1 and (b.damage() == d).all()
    b.values_set(None)
    assert b.memory_bytes() == mem0 and not b.values_on
    with pytest.raises(_lib.SimfireHipError, match="sf_values_set"):
        b.damage()
    with pytest.raises(_lib.SimfireHipError, match="sf_values_set"):
        b.values_torch()
    assert b.state_bytes() == bytes0 and b.save_state([0, 1]).tobytes() == blob0
    b.values_set(None)                                          # off twice: nothing
    b.enable_arrival(False)                                     # and now recording may go
    assert not b.arrival_on
    b.step(3)


def torch_plane(values):
    import torch
    return torch.from_numpy(np.ascontiguousarray(values, dtype=np.int32)).cuda()


# ------------------------------------------------------------------ 5. refusals
def test_refusals():
    import torch
    from simfire_amd import _lib
    case = "24x40"
    kw, R8, E, inits = vw.make_world(case)
    H, W = kw["shape"]
    values = vw.make_values(case, E, inits)
    b = _engine(kw, E, R8, "fused0")
    b.reset(inits)
    L, h = b._L, b._h
    p = np.ascontiguousarray(values)
    assert L.sf_values_set(h, p.ctypes.data_as(C.c_void_p), 0, 0) == _lib.SF_ESTATE           # no arrival recording
    with pytest.raises(_lib.SimfireHipError, match="sf_enable_arrival"):
        b.values_set(values)
    buf = np.zeros(E, dtype=np.int64)
    assert L.sf_values_get(h, buf.ctypes.data_as(C.c_void_p)) == _lib.SF_ESTATE
    b.enable_arrival(True)
    b.step(4)
    for bad in (VALUE_MAX + 1, -VALUE_MAX - 1):
        q = p.copy()
        q[H - 1, W - 1] = bad
        assert L.sf_values_set(h, q.ctypes.data_as(C.c_void_p), 0, 0) == _lib.SF_EINVAL         # host input: before any device work
        with pytest.raises(ValueError):
            b.values_set(q)
        assert not b.values_on and L.sf_values_get(h, buf.ctypes.data_as(C.c_void_p)) == _lib.SF_ESTATE
        t = torch_plane(q)
        assert L.sf_values_set(h, C.c_void_p(t.data_ptr()), 0, 1) == _lib.SF_EINVAL             # device input: the kernel's verdict
    for wrong in (np.zeros((H, W + 1), np.int32), np.zeros((E + 1, H, W), np.int32), np.zeros((H * W,), np.int32)):
        with pytest.raises(ValueError):
            b.values_set(wrong)
        with pytest.raises(ValueError):
            b.values_set(torch_plane(wrong))
    with pytest.raises(ValueError):
        b.values_set(torch_plane(values).to(torch.int64))
    edge = p.copy()
    edge[0, 0], edge[H - 1, W - 1] = VALUE_MAX, -VALUE_MAX                                       # the bounds themselves are values
    b.values_set(edge)
    d = b.damage()
    q = p.copy()
    q[0, 0] = VALUE_MAX + 1
    with pytest.raises(ValueError, match="device plane"):
        b.values_set(torch_plane(q))                            # a refused plane leaves the one that is set, and its damage
    assert (b.damage() == d).all()
    b.step(3)
    assert (b.damage() == damage(edge, np.stack([b.arrival(e) for e in range(E)]))).all()
    # the fifth weight: not without agents, not without a plane
    assert L.sf_values_set_weight(h, 1.0, 1) == _lib.SF_ESTATE
    with pytest.raises(_lib.SimfireHipError, match="sf_agents_create"):
        b.agents_set_value_weight(-0.5)
    b.values_set(None)
    b.agents_create(2, inits)
    assert L.sf_values_set_weight(h, 1.0, 1) == _lib.SF_ESTATE
    with pytest.raises(_lib.SimfireHipError, match="sf_values_set"):
        b.agents_set_value_weight(-0.5)
    b.values_set(values)
    b.agents_set_value_weight(-0.5)
    b.agents_set_value_weight(None)
    with pytest.raises(NotImplementedError, match="arrival"):                                    # SF_ENOTSUP, as under recording
        b.loop_start(2)


def test_simulation_classes_carry_values():
    """``FireSimulation.set_values`` / ``damage`` through ``reset()`` and ``copy.deepcopy``; ``BatchedFireSimulation.set_values``
    (which enables arrival itself) / ``damage`` against the plane summed over ``arrival()``."""
    import copy
    import os
    import yaml
    from simfire_amd.config import Config
    from simfire_amd.simulation import BatchedFireSimulation, FireSimulation
    from test_env_state_gpu import CFG
    y = yaml.safe_load(open(os.path.join(CFG, "functional_config.yml")))
    y["area"]["screen_size"] = [96, 96]
    y["terrain"]["topography"]["functional"]["function"] = "flat"
    y["simulation"]["headless"] = True
    cfg = Config(config_dict=y)
    rng = np.random.default_rng(5)
    values = rng.integers(-50, 1000, size=(96, 96)).astype(np.int32)
    x0, y0 = cfg.fire.fire_initial_position
    sim = FireSimulation(cfg)
    sim.set_values(values)
    assert sim.record_arrival and sim.damage == int(values[y0, x0])
    sim.run(6)
    assert sim.damage == int(values[sim.arrival_steps >= 0].sum()) != int(values[y0, x0])
    twin = copy.deepcopy(sim)
    assert twin.damage == sim.damage
    sim.run(2)
    twin.run(2)
    assert twin.damage == sim.damage == int(values[sim.arrival_steps >= 0].sum())
    sim.reset()
    assert sim.damage == int(values[y0, x0])
    with pytest.raises(ValueError):
        sim.set_values(values[:, :-1])
    bat = BatchedFireSimulation(cfg, 4)
    per_env = rng.integers(0, 100, size=(4, 96, 96)).astype(np.int32)
    bat.set_values(per_env)
    bat.run(5, return_maps=False)
    arr = bat.arrival()
    assert (bat.damage() == damage(per_env, arr)).all() and (bat.damage([2, 0]) == damage(per_env, arr)[[2, 0]]).all()
    with pytest.raises(ValueError):
        BatchedFireSimulation(cfg, 4).set_values(per_env[:3])
