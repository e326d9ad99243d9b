"""``observe`` on the GPU (``sf_observe`` / ``k_observe``): every case is compared bit for bit with tests/_obs_oracle.py, which is fed
from ``fire_maps()``, ``attribute_data(e)`` and the agent entries.  ``observe`` is called before the oracle's inputs are read, so the
observation is taken from the cell plane the last step left current; each case asserts that the launch structure - and the plane - it
is about really was there.  Run with ``pytest -m gpu``."""
import numpy as np
import pytest

import _obs_oracle as O

pytestmark = pytest.mark.gpu

ALL = ["fire_map"] + [f"burn_status:{s}" for s in O.STATUS_NAMES] + list(O.ATTRIBUTES) + ["agent_positions"]


def _layers(rng, H, W):
    y = np.arange(H, dtype=np.float64)[:, None]
    elev = 800.0 + 3.0 * y + rng.random((H, W)) * 40.0
    elev[0, 0], elev[-1, -1] = -300.0, 11500.0                    # outside get_attribute_bounds: normalised, not clamped
    return (rng.uniform(0.05, 1.0, (H, W)), rng.uniform(0.5, 6.0, (H, W)), rng.uniform(0.12, 0.6, (H, W)),
            rng.integers(500, 3500, (H, W)) + rng.random((H, W)), elev, rng.uniform(0.0, 900.0, (H, W)), rng.uniform(0.0, 360.0, (H, W)))


def _engine(H, W, E, seed, per_env=False, fbfm=False, md=4):
    from simfire_amd.engine import FireEngine
    rng = np.random.default_rng(seed)
    eng = FireEngine((H, W), n_envs=E, max_fire_duration=md, pixel_scale=10.0, update_rate=1.0, attenuate_line_ros=True,
                     per_env_terrain=per_env)
    if fbfm:
        for e in range(E):
            lay = _layers(rng, H, W)
            codes = rng.choice([1, 2, 4, 5, 8, 9, 10], size=(H, W))
            eng.set_layers_fbfm(codes, lay[4], lay[5], lay[6], env=e)
    elif per_env:
        for e in range(E):
            eng.set_layers(*_layers(rng, H, W), env=e)
    else:
        eng.set_layers(*_layers(rng, H, W))
    eng.reset(np.stack([rng.integers(0, W, E), rng.integers(0, H, E)], axis=1))
    return eng, rng


def _agents(rng, n, H, W, k=7):
    a = np.stack([rng.integers(-2, W + 2, (n, k)), rng.integers(-2, H + 2, (n, k)), rng.integers(-1, 5, (n, k))], axis=2)
    a[:, 1, :2] = a[:, 0, :2]                                      # two entries on one cell
    return a.astype(np.int32)


def _check(eng, channels=ALL, dtype=None, **kw):
    import torch
    out = eng.observe(channels, dtype=dtype, **kw)
    if eng.async_mode:
        eng.sync()
    got = out.cpu()
    maps = eng.fire_maps()
    cache = {}

    def attrs(e):
        key = e if eng.params.per_env_terrain else 0
        if key not in cache:
            cache[key] = eng.attribute_data(e)
        return cache[key]
    okw = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in kw.items() if k != "out"}
    want = O.observe(channels, maps, attrs, **okw)
    assert tuple(got.shape) == want.shape
    if dtype is torch.bfloat16:
        g, w = got.view(torch.int16).numpy().view(np.uint16), O.bf16_bits(want)
    else:
        g, w = got.numpy().view(np.uint32), want.view(np.uint32)
    bad = np.argwhere(g != w)
    assert bad.size == 0, (len(bad), bad[:5].tolist(), [float(got.float()[tuple(b)]) for b in bad[:5]], [float(want[tuple(b)]) for b in bad[:5]])
    return out


def _divisor(rng, *ns):
    d = [f for f in (1, 2, 3, 4, 5, 8) if all(n % f == 0 for n in ns)]
    return int(rng.choice(d))


def _suite(eng, rng):
    """Three requests: the whole grid with agents; a crop around centers at the corners / off the grid, pooled with mixed modes and a
    pad; bfloat16 with a subset of the environments (repeats)."""
    import torch
    H, W, E = eng.H, eng.W, eng.n_envs
    f = _divisor(rng, H, W)
    _check(eng, pool=f, agents=_agents(rng, E, H, W), normalize=bool(rng.integers(2)))
    f = int(rng.choice([1, 2, 4]))
    ch, cw = f * int(rng.integers(1, 20)), f * int(rng.integers(1, 20))
    cen = np.stack([rng.choice([0, W - 1, -5, W + 40, int(rng.integers(W))], E), rng.choice([0, H - 1, -9, int(rng.integers(H))], E)], 1)
    modes = {c: ("max" if rng.integers(2) else "mean") for c in ALL}
    _check(eng, pool=f, pool_mode=modes, crop=(ch, cw), centers=cen, pad=float(rng.choice([0.0, -1.5, 0.3])), agents=_agents(rng, E, H, W))
    envs = rng.integers(0, E, max(2, E // 2) + 1)
    _check(eng, ["fire_map", "elevation", "burn_status:BURNING", "wind_speed", "fire_map"], envs=envs, dtype=torch.bfloat16,
           pool=_divisor(rng, H, W))


# ------------------------------------------------------------------ launch structures
@pytest.mark.parametrize("mode", ["fused0", "fused1", "generic"])
def test_per_step_kernels(mode):
    eng, rng = _engine(90, 140, 3, 1000 + len(mode), md=(8 if mode == "generic" else 4))
    want = {"fused0": 0, "fused1": 1, "generic": 3}[mode]
    if mode == "generic":
        eng.set_generic(True)
    else:
        eng.set_fused(want)
    for n in (1, 4, 9):
        eng.step(n)
        assert eng.last_launch_kind() == want and eng.cell_layout() == 0
        _suite(eng, rng)


@pytest.mark.parametrize("win", [1, 0])
def test_resident_launch_in_and_past_the_window_phase(win):
    eng, rng = _engine(120, 160, 4, 2000 + win)
    eng.set_fused(2)
    eng.set_tuning(run_window=win)
    eng.enable_counters(True)
    for n in (2, 5, 30):
        eng.step(n)
        assert eng.last_launch_kind() == 2 and eng.cell_layout() == 1
        _suite(eng, rng)
    cnt = eng.counters()["window_updates"]
    assert (cnt > 0) if win else (cnt == 0)


def test_window_kernel_in_front_of_the_resident_launch():
    eng, rng = _engine(100, 120, 6, 3000)
    eng.set_tuning(run_compact=2, run_window=1)
    eng.step(2)
    assert eng.last_launch_kind() == 4 and eng.cell_layout() == 1
    _suite(eng, rng)
    eng.step(3)
    _suite(eng, rng)


def test_team_launches():
    eng, rng = _engine(200, 150, 3, 4000)
    eng.set_fused(2)
    eng.set_tuning(run_team=2)
    seen = False
    for n in (6, 20):
        eng.step(n)
        assert eng.last_launch_kind() == 2 and eng.cell_layout() == 1
        seen |= bool((eng.team_sizes() == 2).all())
        _suite(eng, rng)
    assert seen


@pytest.mark.parametrize("W", [77, 1030, 1102])
def test_widths_and_two_word_rows(W):
    eng, rng = _engine(70, W, 2, 5000 + W)
    layouts = set()
    eng.step(6)
    layouts.add(eng.cell_layout())
    _suite(eng, rng)
    eng.set_fused(0)
    eng.step(3)
    assert eng.cell_layout() == 0
    layouts.add(0)
    _suite(eng, rng)
    if W == 77:
        assert layouts == {0, 1}


def test_after_a_rollout_with_control_lines():
    eng, rng = _engine(96, 130, 4, 6000)
    eng.set_fused(2)
    blk = np.zeros((6, 4, 5, 3), dtype=np.int32)
    blk[..., 0] = rng.integers(0, 130, (6, 4, 5))
    blk[..., 1] = rng.integers(0, 96, (6, 4, 5))
    blk[..., 2] = rng.integers(3, 6, (6, 4, 5))
    eng.step_mitigated(blk)
    assert eng.last_launch_kind() == 2 and eng.cell_layout() == 1
    _suite(eng, rng)
    assert (eng.fire_maps() >= 3).any()


def test_after_clone_and_restore():
    eng, rng = _engine(80, 100, 4, 7000)
    eng.set_fused(2)
    eng.step(5)
    eng.copy_envs([0], [2])
    assert eng.cell_layout() == 1
    _suite(eng, rng)
    blob = eng.save_state([1])
    eng.step(4)
    eng.load_state([1], blob)
    _suite(eng, rng)


def test_async_mode():
    import torch
    eng, rng = _engine(80, 112, 3, 8000)
    eng.set_async(True)
    eng.step(3)
    out = torch.full((3, len(ALL), 40, 56), 7.0, device="cuda:0")
    _check(eng, pool=2, out=out, agents=_agents(rng, 3, 80, 112))
    eng.step(2)
    _check(eng, crop=(16, 16), centers=torch.tensor([[5, 5], [100, 70], [50, 40]], dtype=torch.int32, device="cuda:0"))
    eng.set_async(False)


@pytest.mark.parametrize("fbfm", [False, True])
def test_per_environment_terrain(fbfm):
    eng, rng = _engine(70, 90, 4, 9000 + fbfm, per_env=True, fbfm=fbfm)
    eng.step(4)
    a0, a1 = eng.attribute_data(0), eng.attribute_data(1)
    assert not (a0["w_0"] == a1["w_0"]).all() or not (a0["elevation"] == a1["elevation"]).all()
    _suite(eng, rng)
    eng.set_fused(2)
    eng.step(3)
    _suite(eng, rng)


def test_env_subsets_with_repeats():
    eng, rng = _engine(64, 80, 5, 10000)
    eng.step(4)
    _check(eng, envs=[3, 0, 3, 3, 1], pool=4, agents=_agents(rng, 5, 64, 80))
    _check(eng, ["agent_positions", "fire_map"], envs=[4], agents=np.array([[[1, 1, 3], [2, 2, 3], [1, 1, 9]]], np.int32))


def test_device_tensor_centers_and_agents():
    import torch
    eng, rng = _engine(72, 96, 4, 11000)
    eng.set_fused(2)
    eng.step(6)
    cen = torch.tensor(np.stack([rng.integers(-10, 106, 4), rng.integers(-10, 82, 4)], 1), dtype=torch.int32, device="cuda:0")
    ag = torch.from_numpy(_agents(rng, 4, 72, 96)).to("cuda:0")
    _check(eng, crop=(24, 32), centers=cen, agents=ag, pool=2, pool_mode="max")


def test_c3_sized_batch():
    """256 environments of 1024 x 1024 (BASELINE C3), 9 channels, pool 8, on the blocked plane of the resident launch."""
    from simfire_amd.engine import FireEngine
    from simfire_amd.workloads import c3
    w = c3()
    eng = FireEngine(**w.engine_kwargs())
    eng.set_layers(*w.layers())
    eng.reset(w.init_xy)
    eng.step(20)
    assert eng.last_launch_kind() == 2 and eng.cell_layout() == 1
    ch = ["fire_map"] + [f"burn_status:{s}" for s in O.STATUS_NAMES] + ["elevation", "wind_speed"]
    _check(eng, ch, pool=8)


def test_fire_simulation_after_host_edits():
    import os
    import yaml
    from simfire_amd.config import Config
    from simfire_amd.observe import agents_from_map
    from simfire_amd.simulation import FireSimulation
    y = yaml.safe_load(open(os.path.join(os.path.dirname(__file__), "golden", "configs", "functional_config.yml")))
    y["area"]["screen_size"] = [128, 128]
    y["terrain"]["topography"]["functional"]["function"] = "flat"
    y["simulation"]["headless"] = True
    sim = FireSimulation(Config(config_dict=y))
    for _ in range(5):
        sim.run(1)
    sim.fire_map[40, 10:30] = 4                                   # a host edit the device has not seen yet
    sim.update_agent_positions([(3, 4, 1), (10, 11, 2), (5, 5, 1)])
    out = sim.observe(ALL, pool=2).cpu().numpy()
    eng = sim._engine
    maps = eng.fire_maps()
    assert (maps[0, 40, 10:30] == 4).all() and (maps[0] == sim.fire_map).all()
    want = O.observe(ALL, maps, lambda e: eng.attribute_data(e), pool=2, agents=agents_from_map(sim.agent_positions))
    assert (out.view(np.uint32) == want.view(np.uint32)).all()
    ag = out[0, ALL.index("agent_positions")]
    assert ag[2, 2] == 0.25 and ag[2, 1] == 0.0 and ag[5, 5] == 0.5      # agent 1 moved from (3, 4) to (5, 5); agent 2 at (10, 11)


# ------------------------------------------------------------------ no side effects
@pytest.mark.parametrize("fused", [-1, 0])
def test_observe_does_not_change_the_rollout(fused):
    """The same seeded rollout with and without observe after every step: maps, result rows, elapsed_time, burn amounts and the
    sf_run_delta lists are identical."""
    import torch
    a, _ = _engine(96, 112, 4, 12000)
    b, _ = _engine(96, 112, 4, 12000)
    for e in (a, b):
        e.set_fused(fused)
    rng = np.random.default_rng(5)
    for t in range(30):
        n = int(rng.choice([1, 1, 1, 2, 5]))
        if rng.random() < 0.3:
            pts = [(int(rng.integers(4)), int(rng.integers(112)), int(rng.integers(96)), int(rng.integers(3, 6))) for _ in range(6)]
            a.apply_mitigation(pts)
            b.apply_mitigation(pts)
        if t % 7 == 3:
            blk = np.stack([rng.integers(0, 112, (2, 4, 3)), rng.integers(0, 96, (2, 4, 3)), rng.integers(3, 6, (2, 4, 3))], 3).astype(np.int32)
            a.step_mitigated(blk)
            b.step_mitigated(blk)
            ra, rb = a.status(), b.status()
            assert (ra[0] == rb[0]).all() and (ra[1] == rb[1]).all()
        else:
            env = t % 4
            row_a, el_a, d_a = a.run_delta(n, env)
            row_b, el_b, d_b = b.run_delta(n, env)
            assert (row_a == row_b).all() and el_a == el_b, t
            assert (d_a is None) == (d_b is None), t
            if d_a is not None:
                ia, ib = np.argsort(d_a[0]), np.argsort(d_b[0])
                assert (d_a[0][ia] == d_b[0][ib]).all() and (d_a[1][ia] == d_b[1][ib]).all(), t
        b.observe(ALL, pool=int(rng.choice([1, 2, 4])), agents=_agents(rng, 4, 96, 112),
                  dtype=(torch.bfloat16 if t % 2 else None))
    sa, sb = a.status(), b.status()
    assert (sa[0] == sb[0]).all() and (sa[1] == sb[1]).all()
    assert (a.fire_maps() == b.fire_maps()).all()
    for e in range(4):
        assert (a.burn(e) == b.burn(e)).all()
        da, db = a.fire_map_delta(e), b.fire_map_delta(e)
        assert (da is None) == (db is None)
