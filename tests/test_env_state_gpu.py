"""Environment state on the GPU: fork inside a handle (``sf_copy_envs``), snapshot / restore (``sf_save_state`` / ``sf_load_state``),
``BatchedFireSimulation.clone_envs`` / ``get_state`` / ``set_state`` and ``copy.deepcopy(FireSimulation)``.

Every environment keeps a log of what was done to it (its ignition, control lines, updates); a forked environment's log is its
source's up to the fork, then its own.  After every update the device is compared bit for bit with ``oracle/fire_dense.c`` replaying
each log from the start (with ``prune_after_quit``, which the oracle does not model, with a fresh one-environment handle of the
per-step kernels replaying it).  Run with ``pytest -m gpu``."""
import copy
import os

import numpy as np
import pytest

import _golden
from oracle import fire_dense

pytestmark = pytest.mark.gpu

CFG = os.path.join(os.path.dirname(__file__), "golden", "configs")


def _world(rng, H, W, md, att, diag=True):
    kw = dict(shape=(H, W), max_fire_duration=md, pixel_scale=float(rng.choice([5.0, 20.0, 50.0])),
              update_rate=float(rng.choice([1.0, 0.5, 1.5])),
              max_time=(None if rng.random() < 0.6 else float(rng.integers(8, 40))),
              attenuate_line_ros=att, diagonal_spread=diag)
    R8 = rng.choice([0.0, 3.0, 7.5, 12.0, 30.0, 400.0, 1200.0], size=(8, H, W))
    R8[:, rng.random((H, W)) < 0.1] = 0.0
    return kw, R8


class _Replay:
    """The reference for one environment: a fresh oracle that its log is replayed on; ``apply`` then carries it along."""

    def __init__(self, kw, prune, graph):
        self.kw, self.prune, self.graph = kw, prune, graph

    def apply(self, o, op, rtables):
        if op[0] == "table":
            o.set_rtable(rtables[op[1]])
        elif op[0] == "reset":
            o.reset([op[1]])
        elif op[0] == "mit":
            o.apply_mitigation([(0, x, y, t) for (x, y, t) in op[1]])
        else:
            o.step(1)

    def run(self, log, rtables):
        from simfire_amd.engine import FireEngine
        kw = dict(self.kw)
        kw.pop("n_envs", None)
        if self.prune:
            o = FireEngine(**kw)
            o.set_fused(0)
            o.set_prune_after_quit(True)
            if self.graph:
                o.enable_spread_graph(True)
        else:
            o = fire_dense.DenseOracle(**kw)
        for op in log:
            self.apply(o, op, rtables)
        return o


def _check(eng, e, ref, tag, graph=False, burn=True):
    # (fire_map / status read the blocked plane where it is current; burn converts the handle to the row-major planes)
    assert (eng.fire_map(e) == ref.fire_map(0)).all(), tag
    if burn:
        assert (eng.burn(e) == ref.burn(0)).all(), tag
    st, el = eng.status()
    so, eo = ref.status()
    assert (st[e] == so[0]).all() and el[e] == eo[0], (tag, st[e], so[0], el[e], eo[0])
    if graph:
        want = ref.spread_parents(0) if hasattr(ref, "spread_parents") else ref.parents(0)
        assert (eng.spread_parents(e) == want).all(), tag


MODES = {
    "fused0": dict(fused=0),
    "fused1": dict(fused=1),
    "run": dict(fused=2),
    "run_win": dict(fused=2, tuning=dict(run_window=3)),
    "run_team": dict(fused=2, tuning=dict(run_team=2)),                          # every environment split into two workgroups
    "run_kwin": dict(fused=-1, tuning=dict(run_compact=2, run_window=1)),        # k_win in front of k_run (the automatic choice only)
}
RESIDENT = ("run", "run_win", "run_team", "run_kwin")


def _fork_world(seed, mode, att, md, prune, graph, one_to_many, steps=36):
    """A handle of 4-8 environments running different episodes; at a random update some src is forked into dst(s) that have
    burnt for a while; every environment then gets actions of its own.  Compared with its replayed log after every update."""
    from simfire_amd.engine import FireEngine
    rng = np.random.default_rng(seed)
    window = mode in ("run_win", "run_kwin")
    if mode == "run_team":
        H, W = int(rng.integers(130, 320)), int(rng.integers(64, 300))      # (>= 5 tile rows: bands for two members)
    elif window:
        H, W = int(rng.integers(64, 200)), int(rng.integers(64, 200))
    else:
        H, W = int(rng.integers(5, 70)), int(rng.integers(5, 70))
    E = int(rng.integers(4, 9))
    kw, R8 = _world(rng, H, W, md, att, diag=bool(rng.integers(2)) or window)
    eng = FireEngine(n_envs=E, **kw)
    m = MODES[mode]
    eng.set_fused(m["fused"])
    if m.get("tuning"):
        eng.set_tuning(**m["tuning"])
    if prune:
        eng.set_prune_after_quit(True)
    if graph:
        eng.enable_spread_graph(True)
    eng.set_rtable(R8)
    inits = [(int(rng.integers(W)), int(rng.integers(H))) for _ in range(E)]
    eng.reset(inits)
    logs = [[("table", 0), ("reset", inits[e])] for e in range(E)]
    rep = _Replay(kw, prune, graph)
    fork_at = int(rng.integers(3, steps // 2))
    chunk = 1 if mode in ("fused0", "fused1") else int(rng.integers(2 if mode == "run_kwin" else 1, 4))
    resident = mode in RESIDENT and md <= 5 and not graph      # (wider sprite planes, the spread graph: always the per-step kernels)
    refs = {e: rep.run(logs[e], [R8]) for e in range(E)}
    saw = False                                      # the launch the mode names has run before the fork
    t = 0
    while t < steps:
        if t == fork_at:
            if mode == "run_team" or mode == "run_kwin":
                assert saw, (seed, mode, "the launch this mode names never ran")
            if resident:      # the last step was a resident launch and no getter has converted the layout since: the blocked plane is current
                assert eng.last_launch_kind() in (2, 4), eng.last_launch_kind()
            src = int(rng.integers(E))
            others = [e for e in range(E) if e != src]
            dst = [int(d) for d in rng.choice(others, size=(min(3, len(others)) if one_to_many else 1), replace=False)]
            eng.copy_envs([src] * len(dst), dst)
            for d in dst:
                logs[d] = list(logs[src])
                refs[d] = rep.run(logs[d], [R8])          # dst's whole history: src's up to here
            for e in range(E):
                _check(eng, e, refs[e], (seed, mode, "after fork", e), graph)
        pts = []
        for e in range(E):
            if rng.random() < 0.35:
                p = [(int(rng.integers(W)), int(rng.integers(H)), int(rng.integers(3, 6))) for _ in range(int(rng.integers(1, 5)))]
                fm = refs[e].fire_map(0)
                burning = np.argwhere(fm == 1)
                if len(burning) and rng.random() < 0.6:
                    y, x = burning[rng.integers(len(burning))]
                    p.append((int(x), int(y), int(rng.integers(3, 6))))
                pts += [(e, x, y, ty) for (x, y, ty) in p]
                logs[e].append(("mit", p))
                rep.apply(refs[e], ("mit", p), [R8])
        if pts:
            eng.apply_mitigation(pts)
        n = min(chunk, steps - t, fork_at - t if t < fork_at else steps)      # (a call never steps past the fork)
        if mode == "run_kwin" and t < fork_at and fork_at - t - n == 1:
            n += 1            # (the call in front of the fork steps 2+ updates: one update alone is the per-step kernels' in the automatic choice)
        eng.step(n)
        if mode == "run_team":
            saw |= int(eng.team_sizes().max()) >= 2
        elif mode == "run_kwin":
            saw |= eng.last_launch_kind() == 4
        for e in range(E):
            logs[e] += [("step",)] * n
            for _ in range(n):
                rep.apply(refs[e], ("step",), [R8])
        t += n
        for e in range(E):
            _check(eng, e, refs[e], (seed, mode, t, e), graph, burn=not (resident and t == fork_at))
    return eng


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("att", [False, True])
@pytest.mark.parametrize("seed", range(3))
def test_fork_random_worlds(seed, att, mode):
    _fork_world(71000 + seed + 10 * att, mode, att, md=int(np.random.default_rng(seed).integers(1, 6)), prune=False,
                graph=False, one_to_many=seed == 1)


@pytest.mark.parametrize("md", [9, 20])          # sprite planes of 2 and 4 bytes per cell
@pytest.mark.parametrize("mode", ["fused0", "run"])
def test_fork_wide_sprite_planes(md, mode):
    _fork_world(72000 + md, mode, True, md=md, prune=False, graph=False, one_to_many=True)


@pytest.mark.parametrize("mode", ["fused0", "fused1", "run"])
def test_fork_prune_after_quit_and_graph(mode):
    """Environments that QUIT (runtime cut-offs) and keep pruning; the spread-graph parents travel with the fork."""
    for seed in range(3):
        _fork_world(73000 + seed, mode, bool(seed & 1), md=3, prune=True, graph=False, one_to_many=True, steps=40)
    _fork_world(73100, mode, True, md=3, prune=False, graph=True, one_to_many=True)


def _big_engine(E, size=1024):
    from simfire_amd import workloads
    from simfire_amd.engine import FireEngine
    w = workloads.c3(size, E)
    eng = FireEngine(**w.engine_kwargs())
    eng.set_layers(*w.layers())
    eng.reset(w.init_xy)
    return w, eng


def test_one_to_many_1024():
    """64 x 1024^2: environment 0 forked into the other 63 while its fire is young (the window phase of k_run), again after it
    has outgrown the window; 100 updates after the first fork.  All 64 equal each other and the oracle for environment 0."""
    w, eng = _big_engine(64)
    o = fire_dense.DenseOracle(**dict(w.engine_kwargs(), n_envs=1))
    o.set_rtable(eng.get_rtable(0))
    o.reset(w.init_xy[:1])
    rest = list(range(1, 64))
    eng.step(30)
    o.step(30)
    eng.copy_envs([0] * 63, rest)
    for n in (10, 30):
        eng.step(n)
        o.step(n)
    eng.copy_envs([0] * 63, rest)
    for n in (20, 40):
        eng.step(n)
        o.step(n)
    maps = eng.fire_maps()
    st, el = eng.status()
    so, eo = o.status()
    ref_map, ref_burn = o.fire_map(0), o.burn(0)
    for e in range(64):
        assert (maps[e] == ref_map).all(), e
        assert (st[e] == so[0]).all() and el[e] == eo[0], e
    for e in (0, 1, 31, 63):
        assert (eng.burn(e) == ref_burn).all(), e


@pytest.mark.parametrize("terrain", [True, False])
def test_fork_per_env_terrain(terrain):
    from simfire_amd.engine import FireEngine
    rng = np.random.default_rng(74000 + terrain)
    H, W, E = 48, 57, 4
    kw, _ = _world(rng, H, W, 3, True)
    tabs = [_world(rng, H, W, 3, True)[1] for _ in range(E)]
    eng = FireEngine(n_envs=E, per_env_terrain=True, **kw)
    for e in range(E):
        eng.set_rtable(tabs[e], env=e)
    inits = [(int(rng.integers(W)), int(rng.integers(H))) for _ in range(E)]
    eng.reset(inits)
    eng.step(6)
    eng.copy_envs([1], [3], terrain=terrain)
    assert (eng.get_rtable(3) == tabs[1 if terrain else 3]).all()
    assert (eng.get_rtable(1) == tabs[1]).all()
    log = [("table", 1), ("reset", inits[1])] + [("step",)] * 6 + [("table", 1 if terrain else 3)]
    for t in range(12):
        eng.step(1)
        log.append(("step",))
        ref = _Replay(kw, False, False).run(log, tabs)
        _check(eng, 3, ref, (terrain, t))
    ref1 = _Replay(kw, False, False).run([("table", 1), ("reset", inits[1])] + [("step",)] * 18, tabs)
    _check(eng, 1, ref1, "src")


def test_save_load_across_handles():
    """Saved from a handle whose blocked plane is current (k_run), loaded into a handle with another E whose row-major planes are
    current (per-step kernels); both go on equal to each other and to the oracle.  Mismatching handles refuse the blob and keep
    their maps."""
    from simfire_amd.engine import FireEngine
    rng = np.random.default_rng(75000)
    H, W = 90, 120
    kw, R8 = _world(rng, H, W, 4, True)
    kw["max_time"] = None
    a = FireEngine(n_envs=3, **kw)
    a.set_fused(2)
    b = FireEngine(n_envs=5, **kw)
    b.set_fused(0)
    for x in (a, b):
        x.set_rtable(R8)
    inits = [(int(rng.integers(W)), int(rng.integers(H))) for _ in range(5)]
    a.reset(inits[:3])
    b.reset(inits)
    a.step(12)
    b.step(3)
    blob = a.save_state([1])
    assert blob.shape == (1, a.state_bytes())
    # every byte of a blob is written: saves of one state are equal whatever the buffers held before
    import torch
    a.save_state([0, 2])                                  # (other data through the staging buffer)
    again = a.save_state([1])
    dev = torch.full((a.state_bytes() + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    a.save_state([1], out=dev[:a.state_bytes()])
    assert (again == blob).all() and (dev[:a.state_bytes()].cpu().numpy() == blob[0]).all()
    with pytest.raises(ValueError):                       # a device blob must be 16-byte aligned
        a.save_state([1], out=dev[8:8 + a.state_bytes()])
    b.load_state([3], blob)
    log = [("table", 0), ("reset", inits[1])] + [("step",)] * 12
    for t in range(10):
        p = [(int(rng.integers(W)), int(rng.integers(H)), 3)]
        a.apply_mitigation([(1, x, y, ty) for (x, y, ty) in p])
        b.apply_mitigation([(3, x, y, ty) for (x, y, ty) in p])
        log += [("mit", p), ("step",)]
        a.step(1)
        b.step(1)
        ref = _Replay(kw, False, False).run(log, [R8])
        _check(a, 1, ref, ("a", t))
        _check(b, 3, ref, ("b", t))
    # refused: another grid, another max_fire_duration, attenuation off - the target's maps stay as they were
    for change in (dict(shape=(H, W + 1)), dict(max_fire_duration=5), dict(attenuate_line_ros=False)):
        c = FireEngine(n_envs=2, **dict(kw, **change))
        c.set_rtable(rng.choice([3.0, 30.0], size=(8, c.H, c.W)))
        c.reset([(1, 1), (2, 2)])
        c.step(3)
        before = c.fire_maps().copy()
        with pytest.raises(ValueError):
            nb = c.state_bytes()
            c.load_state([0], blob if nb == blob.shape[1] else np.resize(blob, (1, nb)))
        assert (c.fire_maps() == before).all(), change


def _batched(n_envs):
    import yaml
    from simfire_amd.config import Config
    from simfire_amd.simulation import BatchedFireSimulation
    y = yaml.safe_load(open(os.path.join(CFG, "functional_config.yml")))
    y["area"]["screen_size"] = [96, 96]
    y["terrain"]["topography"]["functional"]["function"] = "flat"
    y["simulation"]["headless"] = True
    return BatchedFireSimulation(Config(config_dict=y), n_envs)


@pytest.mark.parametrize("device", [False, True])
def test_rollback(device):
    sim = _batched(4)
    rng = np.random.default_rng(76000)
    A = [[(e, int(rng.integers(96)), int(rng.integers(96)), 3) for e in range(4)] for _ in range(20)]
    sim.run(10, return_maps=False)
    state = sim.get_state(device=device)
    assert state.on_device == device

    def branch():
        for pts in A:
            sim.update_mitigation(pts)
            sim.run(1, return_maps=False)
        return np.stack([sim.fire_map(e) for e in range(4)]), sim.results()

    m1, (r1, e1) = branch()
    sim.set_state(state)
    m2, (r2, e2) = branch()
    assert (m1 == m2).all() and (r1 == r2).all() and (e1 == e2).all()


def test_rollback_async_device_blobs():
    """Async mode with device blobs: get_state waits for the pack before it reads the headers; a blob handed to set_state and dropped
    at once stays alive until the handle's stream has read it, even while torch hands out and overwrites memory meanwhile."""
    import torch
    sim = _batched(4)
    eng = sim._engine
    rng = np.random.default_rng(76500)
    A = [[(e, int(rng.integers(96)), int(rng.integers(96)), 4) for e in range(4)] for _ in range(12)]
    sim.run(8, return_maps=False)
    eng.set_async(True)
    state = sim.get_state(device=True)
    ref_blob = state.blob.cpu().numpy()

    def branch():
        for pts in A:
            sim.update_mitigation(pts)
            eng.step(1)
        eng.sync()
        return np.stack([sim.fire_map(e) for e in range(4)]), sim.results()

    m1, (r1, e1) = branch()
    sim.set_state(sim.get_state(device=True))             # round trip through a temporary blob: changes nothing
    sim.set_state(state)
    del state
    junk = [torch.full((ref_blob.size,), 0x5A, dtype=torch.uint8, device="cuda") for _ in range(4)]      # (memory reuse under the restore)
    eng.sync()
    del junk
    assert (sim.get_state().blob[:, 128:] == ref_blob[:, 128:]).all()       # (the header carries the handle's fire_rows bound, which has grown)
    m2, (r2, e2) = branch()
    assert (m1 == m2).all() and (r1 == r2).all() and (e1 == e2).all()
    eng.set_async(False)


def test_clone_envs_batched_and_async_delta():
    """clone_envs in async mode, then run_delta / fire_map_delta on dst: the host mirror built from the deltas equals the map;
    ignitions follow, so reset([dst]) re-ignites where src started."""
    sim = _batched(4)
    eng = sim._engine
    sim.run(5, return_maps=False)
    mirror = {}
    for e in range(4):
        assert eng.fire_map_delta(e) is None
        mirror[e] = eng.fire_map(e).reshape(-1).copy()
    eng.set_async(True)
    sim.clone_envs([2], [0])
    assert (sim.ignitions[0] == sim.ignitions[2]).all()
    for t in range(6):
        row, el, d = eng.run_delta(2, env=0)
        if d is None:
            mirror[0][:] = eng.fire_map(0).reshape(-1)
        else:
            mirror[0][d[0]] = d[1]
        assert (mirror[0] == eng.fire_map(0).reshape(-1)).all(), t
        assert (eng.fire_map(0) == eng.fire_map(2)).all(), t
    eng.set_async(False)
    sim.reset([0])
    m = eng.fire_map(0)
    x, y = sim.ignitions[2]
    assert m[y, x] == 1 and m.sum() == 1


def test_deepcopy_fire_simulation_c1():
    import yaml
    from simfire_amd.config import Config
    from simfire_amd.simulation import FireSimulation
    d = _golden.load("sim_c1_128.npz")
    y = yaml.safe_load(open(os.path.join(CFG, "functional_config.yml")))
    y["area"]["screen_size"] = [128, 128]
    y["terrain"]["topography"]["functional"]["function"] = "flat"
    y["simulation"]["headless"] = True
    sim = FireSimulation(Config(config_dict=y))
    for _ in range(7):
        sim.run(1)
    twin = copy.deepcopy(sim)
    assert twin.fire_map is not sim.fire_map and twin.config is not sim.config and twin._engine is not sim._engine
    assert (twin.fire_map == sim.fire_map).all() and twin.elapsed_steps == sim.elapsed_steps
    assert twin.elapsed_time == sim.elapsed_time and twin.start_time == sim.start_time
    for s in (sim, twin):
        steps = 7
        while s.active:
            s.run(1)
            steps += 1
            if f"map_{steps}" in d:
                assert (s.fire_map == d[f"map_{steps}"]).all(), steps
            assert (s.fire_map == s._engine.fire_map(0)).all(), steps      # the delta mirror
        assert steps == int(d["steps"]) and s.elapsed_steps == steps
        assert (s.fire_map == d["final"]).all() and s.elapsed_time == float(d["elapsed_time"])
    # mitigations on a copy do not reach the original
    sim2 = FireSimulation(Config(config_dict=y))
    sim2.run(3)
    twin2 = copy.deepcopy(sim2)
    twin2.update_mitigation([(100, 100, 3), (101, 100, 4)])
    twin2.run(2)
    sim2.run(2)
    assert sim2.fire_map[100, 100] == 0 and twin2.fire_map[100, 100] == 3 and twin2.fire_map[100, 101] == 4
    assert (sim2.fire_map == sim2._engine.fire_map(0)).all() and (twin2.fire_map == twin2._engine.fire_map(0)).all()


def test_errors():
    from simfire_amd.engine import FireEngine
    rng = np.random.default_rng(77000)
    kw, R8 = _world(rng, 20, 30, 3, True)
    eng = FireEngine(n_envs=4, **kw)
    eng.set_rtable(R8)
    with pytest.raises(RuntimeError):          # before sf_reset
        eng.copy_envs([0], [1])
    with pytest.raises(RuntimeError):
        eng.save_state([0])
    eng.reset([(1, 1), (2, 2), (3, 3), (4, 4)])
    for src, dst in (([0], [4]), ([-1], [1]), ([0, 1], [2, 2]), ([0, 1], [1, 2]), ([0], [0])):
        with pytest.raises(ValueError):
            eng.copy_envs(src, dst)
    eng.copy_envs([], [])
    with pytest.raises(ValueError):
        eng.load_state([0, 0], eng.save_state([1, 2]))
    # a fork ends the closed loop; the next loop_start works
    eng.set_fused(2)
    eng.loop_start(1)
    eng.loop_step()
    eng.copy_envs([0], [3])
    assert (eng.fire_map(0) == eng.fire_map(3)).all()
    eng.loop_start(1)
    eng.loop_step()
    eng.loop_stop()
    st, _ = eng.status()
    assert (st[0] == st[3]).all()
