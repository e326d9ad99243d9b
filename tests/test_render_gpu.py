"""``render`` on the GPU (``sf_render`` / ``k_render_bg`` / ``k_render``): every frame is compared bit for bit with
tests/_render_oracle.py, fed from ``fire_maps()`` (or ``history``), the layers the test set and ``attribute_data(e)["elevation"]``.
Each case asserts that the cell plane it is about was the one current.  Run with ``pytest -m gpu``."""
import numpy as np
import pytest

import _render_oracle as R

pytestmark = pytest.mark.gpu

RGB = (57, 122, 31)


def _layers(rng, H, W, kind):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    elev = 900.0 + 40.0 * np.sin(x / 9.0) * np.cos(y / 13.0) + 3.0 * y
    if kind == 1:
        elev = rng.uniform(-282.0, 11000.0, (H, W))
    w0 = rng.uniform(0.0, 1.3, (H, W))                             # alpha outside [0, 1] as well
    return (w0, rng.uniform(0.5, 8.0, (H, W)), rng.uniform(0.05, 1.2, (H, W)), rng.integers(500, 3500, (H, W)) + 0.5, elev,
            rng.uniform(0.0, 900.0, (H, W)), rng.uniform(0.0, 360.0, (H, W)))


class _World:
    """An engine and what the oracle needs of every table: fuel colours for a terrain_rgb."""

    def __init__(self, H, W, E, seed, per_env=False, fbfm=False, md=4):
        from simfire_amd.engine import FireEngine
        self.rng = rng = np.random.default_rng(seed)
        self.eng = FireEngine((H, W), n_envs=E, max_fire_duration=md, pixel_scale=10.0, update_rate=1.0, attenuate_line_ros=True,
                              per_env_terrain=per_env)
        self.fuel = {}
        for t in range(E if per_env else 1):
            lay = _layers(rng, H, W, t % 2)
            if fbfm:
                codes = rng.choice([1, 2, 4, 5, 8, 9, 10, 91, 98, 99], size=(H, W))
                self.eng.set_layers_fbfm(codes, lay[4], lay[5], lay[6], env=t if per_env else None)
                self.fuel[t] = lambda rgb, c=codes: R.fbfm_rgb(c)
            else:
                self.eng.set_layers(*lay, env=t if per_env else None)
                self.fuel[t] = lambda rgb, l=lay: R.fuel_rgb(l[0], l[1], l[2], rgb)
        self.eng.reset(np.stack([rng.integers(0, W, E), rng.integers(0, H, E)], axis=1))

    def table(self, e):
        return e if self.eng.params.per_env_terrain else 0

    def want(self, maps, envs, scale=1, mode=None, agents=None, background="fuel", contours=True, rgb=RGB):
        out = []
        for i, e in enumerate(envs):
            z = self.eng.attribute_data(int(e))["elevation"]
            fuel = self.fuel[self.table(int(e))](rgb) if background == "fuel" else None
            out.append(R.render(maps[i], fuel, R.contour_mask(z), scale=scale, mode=mode, agents=None if agents is None else agents[i],
                                background=background, contours=contours))
        return np.stack(out)


def _agents(rng, n, H, W, k=6):
    a = np.stack([rng.integers(-2, W + 2, (n, k)), rng.integers(-2, H + 2, (n, k)), rng.integers(-1, 5, (n, k))], axis=2)
    a[:, 1, :2] = a[:, 0, :2]
    return a.astype(np.int32)


def _check(w, envs=None, scale=1, mode=None, agents=None, background="fuel", contours=True, channels_last=True):
    eng = w.eng
    envs = np.arange(eng.n_envs) if envs is None else np.asarray(envs)
    got = eng.render(envs=envs, scale=scale, mode=mode, background=background, contours=contours, terrain_rgb=RGB, agents=agents,
                     channels_last=channels_last).cpu().numpy()
    if not channels_last:
        got = got.transpose(0, 2, 3, 1)
    maps = eng.fire_maps()[envs]
    want = w.want(maps, envs, scale=scale, mode=mode, agents=agents, background=background, contours=contours)
    bad = np.argwhere((got != want).any(-1))
    assert bad.size == 0, (scale, mode, background, len(bad), bad[:5].tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())


def _suite(w):
    H, W, E = w.eng.H, w.eng.W, w.eng.n_envs
    rng = w.rng
    for scale in (1, 2, 4):
        for mode in (("nearest",) if scale == 1 else ("nearest", "mean", "sprites")):
            _check(w, scale=scale, mode=mode, agents=_agents(rng, E, H, W))
    envs = rng.integers(0, E, E + 2)
    _check(w, envs=envs, scale=2, background="white", agents=_agents(rng, len(envs), H, W), channels_last=False)
    _check(w, scale=4, mode="mean", contours=False, channels_last=False)


# ------------------------------------------------------------------ launch structures and planes
def test_per_step_launches_row_major_plane():
    w = _World(37, 101, 3, 11)
    w.eng.set_fused(0)
    for n in (1, 6):
        w.eng.step(n)
        assert w.eng.cell_layout() == 0
        _suite(w)


def test_resident_launch_blocked_plane():
    w = _World(90, 140, 4, 12)
    w.eng.set_fused(2)
    for n in (2, 9):
        w.eng.step(n)
        assert w.eng.last_launch_kind() == 2 and w.eng.cell_layout() == 1
        _suite(w)


def test_control_lines_burned_and_agents():
    w = _World(64, 80, 2, 13)
    w.eng.step(8)
    pts = np.array([[0, 10, 5, 3], [0, 11, 5, 4], [1, 12, 6, 5], [1, 3, 3, 5]], dtype=np.int32)
    w.eng.apply_mitigation(pts)
    w.eng.step(3)
    _suite(w)


@pytest.mark.parametrize("fbfm", [False, True])
def test_per_environment_terrain(fbfm):
    w = _World(70, 90, 4, 14 + fbfm, per_env=True, fbfm=fbfm)
    w.eng.step(5)
    _suite(w)


def test_shared_fbfm_terrain():
    w = _World(48, 64, 3, 16, fbfm=True)
    w.eng.step(4)
    _suite(w)


def test_regenerated_world_and_clone():
    """Layers drawn on the device (what set_seeds + reset call) and tables copied by clone_envs(terrain=True): the backgrounds are
    rebuilt from the new layers."""
    w = _World(64, 96, 4, 17, per_env=True)
    w.eng.step(3)
    _check(w, scale=2)
    fuel = (0.4, 3.0, 0.15, 1700.0)
    w.eng.generate_layers([1, 3], elevation={"seed": 5, "octaves": 3, "persistence": 0.5, "lacunarity": 2.0, "lo": 0.0, "hi": 900.0},
                          fuel=fuel)
    for e in (1, 3):
        w.fuel[e] = lambda rgb: R.fuel_rgb(np.full((64, 96), fuel[0]), np.full((64, 96), fuel[1]), np.full((64, 96), fuel[2]), rgb)
    w.eng.reset(np.array([[5, 5], [40, 30], [10, 50], [90, 60]]))
    w.eng.step(4)
    _suite(w)
    w.eng.copy_envs([1], [2], terrain=True)
    w.fuel[2] = w.fuel[1]
    _suite(w)


def test_1024_grid():
    w = _World(1024, 1024, 2, 18)
    w.eng.step(6)
    for scale, mode in ((1, None), (4, "sprites"), (4, "mean")):
        _check(w, scale=scale, mode=mode, agents=_agents(w.rng, 2, 1024, 1024))


def test_terrain_rgb_change_rebuilds():
    w = _World(40, 56, 2, 19)
    w.eng.step(2)
    _check(w)
    got = w.eng.render(terrain_rgb=(200, 10, 10)).cpu().numpy()
    want = w.want(w.eng.fire_maps(), [0, 1], rgb=(200, 10, 10))
    assert (got == want).all()


# ------------------------------------------------------------------ no side effects, errors
def test_render_changes_no_state():
    a, b = _World(60, 70, 3, 20), _World(60, 70, 3, 20)
    for eng in (a.eng, b.eng):
        eng.set_fused(2)
        eng.step(4)
        eng.fire_map_delta(0)
        eng.step(3)
    for scale in (1, 4):
        a.eng.render(scale=scale, agents=_agents(a.rng, 3, 60, 70))
    da, db = a.eng.fire_map_delta(0), b.eng.fire_map_delta(0)
    assert (da is None) == (db is None)
    if da is not None:                                                 # (the delta lists come in no particular order)
        ia, ib = np.argsort(da[0]), np.argsort(db[0])
        assert (da[0][ia] == db[0][ib]).all() and (da[1][ia] == db[1][ib]).all()
    assert (a.eng.fire_maps() == b.eng.fire_maps()).all()
    for x, y in zip(a.eng.status(), b.eng.status()):
        assert (np.asarray(x) == np.asarray(y)).all()
    a.eng.step(5)
    b.eng.step(5)
    assert (a.eng.fire_maps() == b.eng.fire_maps()).all()


def test_errors():
    from simfire_amd.engine import FireEngine
    eng = FireEngine((16, 16), n_envs=2)
    with pytest.raises(RuntimeError):
        eng.render()                                                   # no layers
    w = _World(16, 32, 2, 21)
    with pytest.raises(RuntimeError):
        w.eng.render(history=(0, 1))                                   # no history ring
    with pytest.raises(ValueError):
        w.eng.render(scale=0)


# ------------------------------------------------------------------ FireSimulation: recording, history frames, save_gif
def _fire_sim(size=64):
    import os
    import yaml
    from simfire_amd.config import Config
    from simfire_amd.simulation import FireSimulation
    y = yaml.safe_load(open(os.path.join(os.path.dirname(__file__), "golden", "configs", "functional_config.yml")))
    y["area"]["screen_size"] = [size, size]
    y["simulation"]["headless"] = True
    return FireSimulation(Config(config_dict=y, simplex_topography=True))


def test_recording_history_frames_and_gif(tmp_path):
    sim = _fire_sim()
    sim.update_agent_positions([(3, 4, 1), (10, 11, 2)])
    sim.recording_options = {"background": "white"}
    sim.recording = True
    sim.run(3)
    sim.run(70)                                                        # more than one history chunk
    frames = sim.frames
    eng = sim._engine
    k = frames.shape[0]
    assert k == sim.elapsed_steps and k > 3
    z = eng.attribute_data(0)["elevation"]
    agents = [[3, 4, 1], [10, 11, 2]]
    ring_first = max(0, k - sim._history_cap)
    maps = eng.history(0, ring_first, k - ring_first)
    for t in range(ring_first, k):
        want = R.render(maps[t - ring_first], None, R.contour_mask(z), agents=agents, background="white")
        assert (frames[t] == want).all(), t
    last = sim.render(background="white")
    assert (last == frames[-1]).all()
    path = sim.save_gif(tmp_path / "clip")
    assert path.suffix == ".gif" and path.parent == tmp_path / "clip"
    Image = pytest.importorskip("PIL.Image")
    im = Image.open(path)
    dec = []
    for i in range(im.n_frames):
        im.seek(i)
        dec += [np.array(im.convert("RGB"))] * (im.info["duration"] // 100)
    assert (np.stack(dec) == frames).all()


def test_recording_off_and_no_frames():
    sim = _fire_sim(32)
    with pytest.raises(ValueError):
        sim.save_gif()
    with pytest.raises(NotImplementedError):
        sim.rendering = True
    sim.recording = True
    sim.run(2)
    assert sim.frames.shape[0] == sim.elapsed_steps
    sim.recording = False
    n = sim.frames.shape[0]
    sim.run(2)
    assert sim.frames.shape[0] == n
    sim.recording = True
    assert sim.frames.shape[0] == 0
