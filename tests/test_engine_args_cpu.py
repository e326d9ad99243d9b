"""The binding's argument checks without a GPU: for every entry point that takes a list of environment numbers, which exception a
bad list raises and how its message begins - and the mask, points, value-plane, episode and wind checks - all of it raised before
the library is touched.  A characterization: the table states what the binding did before the checks were gathered in
``simfire_amd/_args.py``, and holds for it unchanged."""
import os
import subprocess
import sys

import numpy as np
import pytest

E, H, W = 4, 24, 40


class _NoLibrary:
    """Stands in for the loaded library: any entry looked up on it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was touched ({name}) before the arguments were checked")


def _engine(params=False):
    from simfire_amd import _lib
    from simfire_amd.engine import FireEngine
    eng = FireEngine.__new__(FireEngine)
    eng._L, eng._h = _NoLibrary(), None
    eng.H, eng.W, eng.n_envs = H, W, E
    eng.async_mode, eng._blobs_in_flight = False, []
    eng.values_on, eng.arrival_on, eng.episodes_on, eng.n_agents = False, True, False, 2
    if params:
        eng.params = _lib.SfParams(n_envs=E, height=H, width=W, device=0, per_env_terrain=1)
    return eng


def _obs(envs):
    from simfire_amd.observe import ObsSpec
    return ObsSpec(["fire_map"], E, H, W, envs=envs)


def _render(envs):
    from simfire_amd.render import RenderSpec
    return RenderSpec(E, H, W, envs=envs)


CALLS = {
    "reset_envs": lambda v: _engine().reset_envs(v, np.zeros((len(v), 2), dtype=np.int32)),
    "agents_place": lambda v: _engine().agents_place(v, np.zeros((len(v), 2, 2), dtype=np.int32)),
    "copy_envs": lambda v: _engine().copy_envs(v, v),
    "save_state": lambda v: _engine().save_state(v),
    "distance": lambda v: _engine(params=True).distance(2, envs=v),
    "reach": lambda v: _engine(params=True).reach(envs=v),
    "ObsSpec": _obs,
    "RenderSpec": _render,
    "ensemble_stats": lambda v: _engine().ensemble_stats([v]),          # (one group: a 2-D list is one dimension too many here, too)
}
LISTS = {"out of range": [E], "negative": [-1], "2-D": [[0, 1]], "float": [0.5], "empty": []}
ACCEPTED = "accepted"       # the list passes the binding's checks: the call goes on to the library or to the device
UNPINNED = None             # the legacy lenient form lets a float through to the library: known, left alone, not pinned here

# entry point -> for each of LISTS: (exception, how the message begins) | ACCEPTED | UNPINNED
TABLE = {
    "reset_envs": [(IndexError, "reset_envs: "), (IndexError, "reset_envs: "), (ValueError, "reset_envs: envs must be a list"),
                   (ValueError, "reset_envs: envs must be a list"), ACCEPTED],
    "agents_place": [(ValueError, "agents_place: "), (ValueError, "agents_place: "), (ValueError, "envs must be a list of environment numbers"),
                     UNPINNED, ACCEPTED],
    "copy_envs": [ACCEPTED, ACCEPTED, (ValueError, "src must be a list of environment numbers"), UNPINNED, ACCEPTED],
    "save_state": [ACCEPTED, ACCEPTED, (ValueError, "envs must be a list of environment numbers"), UNPINNED, ACCEPTED],
    "distance": [(ValueError, "distance: "), (ValueError, "distance: "), (ValueError, "distance: envs must be a list"),
                 (ValueError, "distance: envs must be a list"), ACCEPTED],
    "reach": [(ValueError, "reach: "), (ValueError, "reach: "), (ValueError, "reach: envs must be a list"),
              (ValueError, "reach: envs must be a list"), ACCEPTED],
    "ObsSpec": [(ValueError, "envs "), (ValueError, "envs "), (ValueError, "envs must be a non-empty list"),
                (ValueError, "envs must be a non-empty list"), (ValueError, "envs must be a non-empty list")],
    "RenderSpec": [(ValueError, "envs "), (ValueError, "envs "), (ValueError, "envs must be a list"), (ValueError, "envs must "), ACCEPTED],
    "ensemble_stats": [(ValueError, "ensemble_stats: members "), (ValueError, "ensemble_stats: members "),
                       (ValueError, "ensemble_stats: members must be a 2-D"), (ValueError, "ensemble_stats: members must be a 2-D"),
                       (ValueError, "ensemble_stats: ")],
}


def test_the_table_covers_every_entry_point_and_list():
    assert set(TABLE) == set(CALLS) and all(len(row) == len(LISTS) for row in TABLE.values())


@pytest.mark.parametrize("entry, case", [(e, c) for e in TABLE for c in LISTS])
def test_environment_lists(entry, case):
    want = TABLE[entry][list(LISTS).index(case)]
    if want is UNPINNED:
        return
    try:
        CALLS[entry](LISTS[case])
    except Exception as exc:                    # noqa: BLE001 (the table says which)
        got = exc
    else:
        got = None
    if want is ACCEPTED:
        # past the checks: nothing raised, the stand-in library reached, or - on a machine without a GPU - torch refusing to allocate
        assert not isinstance(got, (ValueError, IndexError, TypeError)), (entry, case, got)
    else:
        assert type(got) is want[0] and str(got).startswith(want[1]), (entry, case, got)


def test_device_masks_refuse_host_tensors():
    torch = pytest.importorskip("torch")
    xy = np.zeros((E, 2), dtype=np.int32)
    for mask in (torch.ones(E, dtype=torch.uint8), torch.ones(E, dtype=torch.bool), torch.ones(E + 1, dtype=torch.uint8),
                 torch.ones(E, dtype=torch.int32), np.ones(E, dtype=np.uint8), [1, 0, 0, 1]):
        with pytest.raises(ValueError, match="^reset_where: mask must be "):
            _engine().reset_where(mask, xy)
        with pytest.raises(ValueError, match="^episodes_begin: mask must be "):
            _engine().episodes_begin(mask)
    with pytest.raises(ValueError, match="^reset_where: "):
        _engine().reset_where(None, None)


def test_points_and_passable_refuse_host_arrays():
    torch = pytest.importorskip("torch")
    pts = np.zeros((E, 2, 3), dtype=np.int32)
    for bad in (pts, pts.tolist(), torch.from_numpy(pts)):
        with pytest.raises(ValueError, match="^distance: points must be a CUDA int32 tensor"):
            _engine(params=True).distance(2, points=bad)
        with pytest.raises(ValueError, match="^reach: points must be a CUDA int32 tensor"):
            _engine(params=True).reach(points=bad)
    for bad in (np.ones((H, W), dtype=np.uint8), torch.ones((H, W), dtype=torch.uint8), torch.ones((E, H, W), dtype=torch.uint8)):
        with pytest.raises(ValueError, match="^reach: passable must be a CUDA uint8 tensor"):
            _engine(params=True).reach(passable=bad)
    from simfire_amd.observe import ObsSpec
    from simfire_amd.render import RenderSpec
    for bad, word in ((np.zeros((E, 3), np.int32), "shape"), (np.zeros((E, 1, 3)) + 0.5, "integers"), (np.full((E, 1, 3), 2 ** 31), "int32"),
                      (np.zeros((E, 257, 3), np.int32), "at most 256"), (torch.from_numpy(pts), "CUDA int32 tensor")):
        with pytest.raises(ValueError, match=word):
            ObsSpec(["fire_map"], E, H, W, agents=bad)
        with pytest.raises(ValueError, match=word):
            RenderSpec(E, H, W, agents=bad)


@pytest.mark.parametrize("bad, kw", [
    (np.zeros((H, W + 1), dtype=np.int32), {}),
    (np.zeros((E - 1, H, W), dtype=np.int32), {}),
    (np.zeros((H, W), dtype=np.int32), dict(per_env=True)),
    (np.zeros((E, H, W), dtype=np.int32), dict(per_env=False)),
    (np.zeros((H, W), dtype=np.float32), {}),
    (np.full((H, W), (1 << 24) + 1, dtype=np.int64), {}),
    (np.full((E, H, W), -(1 << 24) - 1, dtype=np.int64), {}),
])
def test_values_set(bad, kw):
    eng = _engine(params=True)
    with pytest.raises(ValueError, match="^values_set: "):
        eng.values_set(bad, **kw)
    assert not eng.values_on


@pytest.mark.parametrize("kw", [
    dict(ignition_box=(0, 0, 1)), dict(ignition_box=(-1, 0, 5, 5)), dict(ignition_box=(0, 0, W, 5)), dict(ignition_box=(0, 0, 5, H)),
    dict(ignition_box=(6, 0, 5, 5)), dict(agent_box=(0, 6, 5, 5)), dict(agent_box=(0, 0, 1, 1, 1)), dict(live_cells=True),
    dict(wind_speed=(1.0, 2.0)), dict(wind_direction=(0.0, 90.0)), dict(wind_speed=(2.0, 1.0), wind_direction=(0.0, 90.0)),
    dict(wind_speed=(-1.0, 1.0), wind_direction=(0.0, 90.0)), dict(wind_speed=(1.0, 2.0), wind_direction=(90.0, 0.0)),
    dict(wind_speed=(1.0, float("inf")), wind_direction=(0.0, 90.0)), dict(wind_speed=(1.0, 2.0, 3.0), wind_direction=(0.0, 90.0)),
])
def test_episodes_set(kw):
    eng = _engine()
    with pytest.raises(ValueError, match="^episodes_set: "):
        eng.episodes_set(7, **kw)
    assert not eng.episodes_on


@pytest.mark.parametrize("speed, direction, envs", [
    (np.zeros(E + 1), np.zeros(E + 1), None),                     # one value per table, one too many
    (np.zeros((H, W)), np.zeros(E), None),                        # a field and a list
    (np.zeros((H, W + 1)), np.zeros((H, W + 1)), None),           # not the grid
    (np.zeros((E, H, W)), np.zeros((E, H, W)), [0, 1]),           # a field per environment, two listed
    (np.zeros(3), np.zeros(3), [0, 1]),
    (np.zeros((2, 2, H, W)), np.zeros((2, 2, H, W)), [0, 1]),
])
def test_set_wind_shapes(speed, direction, envs):
    with pytest.raises(ValueError, match="^set_wind: speed "):
        _engine(params=True).set_wind(speed, direction, envs)


def test_set_wind_takes_arrays_or_tensors_not_both():
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match="^set_wind: "):
        _engine(params=True).set_wind(torch.zeros(E, dtype=torch.float64), np.zeros(E))
    for t in (torch.zeros(E, dtype=torch.float64), torch.zeros(E, dtype=torch.float32)):          # host tensors
        with pytest.raises(ValueError, match="^set_wind: speed must be a contiguous "):
            _engine(params=True).set_wind(t, t)


MODULES = ("_args", "observe", "render", "distance", "reach", "ensemble")


def test_the_request_modules_import_without_torch_or_the_library():
    code = ("import sys\nimport simfire_amd._lib as L\n" + "".join(f"import simfire_amd.{m}\n" for m in MODULES)
            + "assert 'torch' not in sys.modules, 'torch was imported'\nassert not L._libs, 'the library was loaded'\nprint('clean')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0 and r.stdout.strip() == "clean", r.stderr
