"""Arrival times on the GPU (``sf_enable_arrival``).  The yardstick is the API that existed before: handle A
runs the per-step kernels (``set_fused(0)``; the per-cell kernel where the sprite planes are wider) without recording, one update
per call, and its maps after every update give the expected arrival (``tests/_arrival_oracle.py``).  Handle B records, in the mode
under test, and makes the same updates in calls of 1, 2, 3, 5, 7, 11, 23.  Run with ``pytest -m gpu``."""
import numpy as np
import pytest

import _arrival_worlds as aw
from _arrival_oracle import MapArrival

pytestmark = pytest.mark.gpu


def _engine(kw, E, R8, mode=None):
    from simfire_amd.engine import FireEngine
    eng = FireEngine(n_envs=E, **kw)
    if mode is None:
        eng.set_fused(0)
    else:
        m = aw.mode_settings(mode)
        eng.set_fused(m["fused"])
        if m.get("tuning"):
            eng.set_tuning(**m["tuning"])
    eng.set_rtable(R8)
    return eng


def _n_envs(case):
    if aw.CASES[case].get("E") == "cu+8":
        import torch
        return torch.cuda.get_device_properties(0).multi_processor_count + 8
    return None


@pytest.mark.parametrize("case,mode", aw.PAIRS, ids=["%s-%s" % p for p in aw.PAIRS])
def test_arrival_matches_the_maps(case, mode):
    """``_arrival_worlds.drive``: behind every call the launch structure the mode names ran on B with recording on
    (``last_launch_kind()`` / ``cell_layout()``), ``B.arrival(e)`` equals the arrival rebuilt from A's maps for every environment,
    and B's maps, status rows, elapsed times and burn amounts equal A's bit for bit; the case's resets, fork, snapshot / restore
    or late enabling in between."""
    import torch
    c = aw.CASES[case]
    kw, R8, E, _ = aw.make_world(case, _n_envs(case))
    a, b = _engine(kw, E, R8), _engine(kw, E, R8, mode)
    if case == "70x1030_wide":
        assert b.geometry()["pitch"] // 16 > 64              # two bitmap words per row
    seen = aw.drive(case, mode, a, b, _n_envs(case), torch=torch)
    sparse, dense = b.arrival_passes()
    kinds = [g for _, g in seen["launches"]]
    print("launches (n, (kind, layout)):", case, mode, seen["launches"], "passes sparse / dense:", sparse, dense)
    if mode in ("run_kwin", "auto_many"):
        assert kinds.count((4, 1)) >= 3, kinds
    if case == "70x1030_wide" and mode == "auto":
        assert kinds.count((2, 1)) >= 4, kinds
    if mode in ("run", "run_win", "run_team", "run_kwin", "auto_many") and c.get("md", 4) <= 5:
        assert sparse > 0, (sparse, dense)                    # one-word rows behind a resident launch: the bitmap walk
    if mode == "run_noteam":
        assert dense >= len(kinds), (sparse, dense)           # two-word rows in the plain kernel: the dense form behind a resident launch
    if mode in ("fused0", "fused1") or c.get("md", 4) > 5:
        assert sparse <= 1 and dense > 0, (sparse, dense)     # (the pass of a full reset may find the fresh bitmap)
    if mode == "run_team":
        assert int(b.team_sizes().max()) >= 2


@pytest.mark.parametrize("case,mode", [("24x40", "run"), ("72x80_win", "run_win"), ("136x64_team", "run_team"), ("24x40_lines", "run")])
def test_sparse_pass_equals_dense_pass(case, mode):
    """The same world once with the bitmap walk and once with the dense pass forced (``set_arrival_dense``): the planes are equal
    after every call."""
    import torch
    kw, R8, E, inits = aw.make_world(case)
    s, d = _engine(kw, E, R8, mode), _engine(kw, E, R8, mode)
    d.set_arrival_dense(True)
    K = aw.CASES[case].get("lines", 0)
    rng = np.random.default_rng(1)
    for h in (s, d):
        h.reset(inits)
        h.enable_arrival(True)
    for i in range(10):
        n = aw.STEPS[i % len(aw.STEPS)]
        if K:
            pts = np.stack([rng.integers(kw["shape"][1], size=(n, E, K)), rng.integers(kw["shape"][0], size=(n, E, K)),
                            rng.choice([0, 3, 4, 5], size=(n, E, K))], axis=-1).astype(np.int32)
        for h in (s, d):
            h.step_mitigated(pts) if K else h.step(n)
            assert (h.last_launch_kind(), h.cell_layout()) == (2, 1)
        assert torch.equal(s.arrival_torch(), d.arrival_torch()), (case, i)
    assert s.arrival_passes()[0] >= 10 and d.arrival_passes()[0] <= 1, (s.arrival_passes(), d.arrival_passes())
    assert int((s.arrival_torch() > 0).sum()) >= 50


def test_state_blobs_and_recording():
    """Blobs of a handle without recording are refused by one with it and the other way round (ValueError: SF_EINVAL), host and
    device pointers alike; with recording off ``state_bytes()`` is the formula of DESIGN.md section 11 (256 + the sections, each
    rounded up to 16 bytes), with it on one u32 plane more."""
    import torch
    kw, R8, E, inits = aw.make_world("33x17")
    H, W = kw["shape"]
    off, on = _engine(kw, E, R8, "run"), _engine(kw, E, R8, "run")
    for h in (off, on):
        h.reset(inits)
    on.enable_arrival(True)
    r16 = lambda v: (v + 15) // 16 * 16
    n = H * W
    parent = 256 + r16(n) + r16(n) + r16(n * 8) + (r16(n * 4) if kw["attenuate_line_ros"] else 0)
    assert off.state_bytes() == parent
    assert on.state_bytes() == parent + r16(n * 4)
    for h in (off, on):
        h.step(7)
    b_off, b_on = off.save_state([0, 1]), on.save_state([0, 1])
    # one blob in a buffer of the loading handle's size: the header is what is looked at
    pad_off = np.zeros((1, on.state_bytes()), dtype=np.uint8)
    pad_off[0, :off.state_bytes()] = b_off[0]
    with pytest.raises(ValueError, match="arrival recording"):
        on.load_state([0], pad_off)
    with pytest.raises(ValueError, match="arrival recording"):
        off.load_state([0], b_on[:1])
    with pytest.raises(ValueError, match="arrival recording"):
        on.load_state([0], torch.from_numpy(pad_off).cuda())
    with pytest.raises(ValueError, match="arrival recording"):
        off.load_state([0], torch.from_numpy(b_on[:1].copy()).cuda())
    assert off.save_state([0, 1]).tobytes() == b_off.tobytes() and on.save_state([0, 1]).tobytes() == b_on.tobytes()      # nothing changed
    # a matching blob restores the plane
    before = np.stack([on.arrival(e) for e in range(E)])
    on.step(5)
    on.load_state([2, 3], b_on)                               # environments 0, 1 as they were after 7 updates, into 2 and 3
    assert (on.arrival(2) == before[0]).all() and (on.arrival(3) == before[1]).all()
    # switching recording off gives the parent's bytes back: byte for byte the blob of the handle that never recorded
    again = _engine(kw, E, R8, "run")
    again.reset(inits)
    again.enable_arrival(True)
    again.step(7)
    again.enable_arrival(False)
    assert again.state_bytes() == parent
    assert again.save_state([0, 1]).tobytes() == b_off.tobytes()
    with pytest.raises(Exception, match="sf_enable_arrival"):
        again.arrival(0)


def test_refusals():
    from simfire_amd import _lib
    kw, R8, E, inits = aw.make_world("72x80_win")
    b = _engine(kw, E, R8, "run")
    b.reset(inits)
    with pytest.raises(_lib.SimfireHipError, match="sf_enable_arrival"):        # SF_ESTATE
        b.arrival(0)
    with pytest.raises(_lib.SimfireHipError, match="sf_enable_arrival"):
        b.arrival_torch()
    b.loop_start(2)                                         # recording off: the closed loop starts ...
    b.loop_step(None)
    b.enable_arrival(True)                                  # ... and enabling ends it
    with pytest.raises(NotImplementedError, match="arrival"):                  # SF_ENOTSUP
        b.loop_start(2)
    b.step(3)
    assert (b.arrival(0) >= 0).sum() >= 1
    mem = b.memory_bytes()
    b.enable_arrival(False)
    assert mem - b.memory_bytes() >= E * kw["shape"][0] * kw["shape"][1] * 4
    b.loop_start(2)
    b.loop_stop()


def test_agents_step_with_auto_reset():
    """``agents_step`` ticks with ``auto_reset`` on the 24 x 40 case of ``tests/_agents_worlds.py`` (one update per tick), B recording,
    against the same ticks assembled on A from the older calls; the expected arrival follows A's map after every tick and starts
    over where the tick reports done."""
    import torch
    import _agents_worlds as agw
    from test_agents_gpu import _Outs, _create, _engine as agent_engine
    case = "24x40_k5_u1_att"
    c = agw.CASES[case]
    assert c["n_updates"] == 1 and c["auto_reset"]
    kw, R8, E, inits, starts = agw.make_world(case)
    for mode in ("run", "fused0"):
        a, b = agent_engine(kw, E, "fused0", R8, inits), agent_engine(kw, E, mode, R8, inits)
        b.enable_arrival(True)
        _create(b, c, inits)
        b.agents_place(list(range(E)), starts)
        outs = _Outs(E)
        exp = MapArrival(E, c["H"], c["W"])
        for e in range(E):
            exp.see(e, a.fire_map(e), 0)
        log = dict(resets=0, cells=0)

        def on_tick(t, actions, want, o):
            b.agents_step(torch.from_numpy(actions).cuda(), **outs.kwargs())
            st = a.status()[0]
            for e in range(E):
                if want["done"][e]:
                    log["resets"] += int((exp.exp[e] >= 0).sum() >= 2)
                    exp.restart(e)
                exp.see(e, a.fire_map(e), st[e, 1])
            log["cells"] = max(log["cells"], int((exp.exp >= 0).sum()))
            assert (outs.host()["done"] == want["done"]).all() and (outs.host()["terms"] == want["terms"]).all(), (mode, t)
            for e in range(E):
                assert (b.arrival(e) == exp.exp[e]).all(), (mode, t, e)
            assert (a.fire_maps() == b.fire_maps()).all(), (mode, t)

        agw.drive(case, a, on_tick)
        assert log["resets"] >= 1 and log["cells"] >= 50, log


def test_simulation_classes_carry_arrival():
    """``FireSimulation.record_arrival`` / ``arrival_steps`` through ``copy.deepcopy``; ``BatchedFireSimulation.enable_arrival`` /
    ``arrival`` through ``clone_envs`` and ``get_state`` / ``set_state``."""
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
    sim = FireSimulation(cfg)
    with pytest.raises(Exception, match="sf_enable_arrival"):
        sim.arrival_steps
    sim.record_arrival = True
    sim.run(6)
    arr = sim.arrival_steps
    x, y = cfg.fire.fire_initial_position
    assert arr.dtype == np.int32 and arr[y, x] == 0 and arr.max() >= 1 and (arr >= 0).sum() == int((np.asarray(sim.fire_map) == 1).sum() + (np.asarray(sim.fire_map) == 2).sum())
    twin = copy.deepcopy(sim)
    assert twin.record_arrival and (twin.arrival_steps == arr).all()
    sim.run(3)
    twin.run(3)
    assert (twin.arrival_steps == sim.arrival_steps).all() and sim.arrival_steps.max() > arr.max()
    sim.reset()
    assert sim.record_arrival and (sim.arrival_steps >= 0).sum() == 1 and sim.arrival_steps[y, x] == 0
    bat = BatchedFireSimulation(cfg, 4)
    bat.enable_arrival()
    bat.run(5, return_maps=False)
    a0 = bat.arrival()
    assert a0.shape[0] == 4 and (a0.max(axis=(1, 2)) >= 1).all()
    state = bat.get_state([0])
    bat.clone_envs([1], [2])
    assert (bat.arrival([2])[0] == a0[1]).all()
    bat.run(4, return_maps=False)
    assert bat.arrival([0])[0].max() > a0[0].max()
    bat.set_state(state, [3])
    assert (bat.arrival([3])[0] == a0[0]).all()
    plain = BatchedFireSimulation(cfg, 4)
    with pytest.raises(ValueError, match="arrival"):
        plain.set_state(state, [0])
