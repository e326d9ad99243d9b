"""``observe`` without a GPU: the NumPy oracle (tests/_obs_oracle.py) against small hand-worked cases, and every argument check of the
spec builder (simfire_amd/observe.py), which raises before any device call."""
import numpy as np
import pytest

import _obs_oracle as O
from simfire_amd.observe import CHANNELS, ObsSpec, agents_from_map

MAP = np.array([[[0, 1, 2, 3],
                 [4, 5, 0, 1],
                 [2, 2, 3, 0],
                 [5, 4, 1, 0]]], dtype=np.uint8)


def _attrs(e):
    g = np.arange(16, dtype=np.float64).reshape(4, 4)
    return {"w_0": (g / 10).astype(np.float32), "sigma": (g * 100 + 1).astype(np.uint32), "delta": (g / 2 + 0.2).astype(np.float32),
            "M_x": (g / 20 + 0.12).astype(np.float32), "elevation": g * 1000 - 282, "wind_speed": g * 30, "wind_direction": g * 22.5}


def test_fire_map_and_every_indicator():
    out = O.observe(["fire_map"] + [f"burn_status:{s}" for s in O.STATUS_NAMES], MAP, None)
    assert out.shape == (1, 7, 4, 4) and out.dtype == np.float32
    assert (out[0, 0] == MAP[0]).all()
    for s in range(6):
        assert (out[0, 1 + s] == (MAP[0] == s)).all()


def test_attributes_raw_and_normalised_at_the_bounds():
    a = _attrs(0)
    raw = O.observe(list(O.ATTRIBUTES), MAP, _attrs, normalize=False)
    for c, name in enumerate(O.ATTRIBUTES):
        assert (raw[0, c] == np.asarray(a[name]).astype(np.float64).astype(np.float32)).all(), name
    norm = O.observe(["elevation", "wind_speed", "w_0"], MAP, _attrs)
    assert norm[0, 0, 0, 0] == 0.0                       # -282 = min
    assert norm[0, 0, 3, 3] == np.float32((15 * 1000 - 282 + 282) / 11282)
    assert norm[0, 1, 3, 3] == np.float32(450 / 250)     # not clamped
    assert norm[0, 2, 0, 0] == 0.0 and norm[0, 2, 1, 2] == np.float32(np.float64(np.float32(0.6)))


def test_crop_at_the_corners_and_fully_off_the_grid():
    out = O.observe(["fire_map"], MAP, None, crop=(3, 3), centers=[[0, 0]], pad=-1.0)
    assert out[0, 0].tolist() == [[-1, -1, -1], [-1, 0, 1], [-1, 4, 5]]
    out = O.observe(["fire_map"], MAP, None, crop=(2, 2), centers=[[3, 3]], pad=9.0)
    assert out[0, 0].tolist() == [[3, 0], [1, 0]]          # top-left (3 - 1, 3 - 1)
    out = O.observe(["fire_map", "elevation"], MAP, _attrs, crop=(2, 3), centers=[[10, -7]], pad=0.25)
    assert (out == np.float32(0.25)).all()                # pad is final, not normalised


def test_mean_and_max_pooling_with_padding():
    out = O.observe(["fire_map"], MAP, None, pool=2)
    assert out[0, 0].tolist() == [[2.5, 1.5], [3.25, 1.0]]
    out = O.observe(["fire_map"], MAP, None, pool=2, pool_mode="max")
    assert out[0, 0].tolist() == [[5, 3], [5, 3]]
    out = O.observe(["fire_map", "burn_status:BURNED"], MAP, None, pool=2, pool_mode={"fire_map": "max"},
                    crop=(2, 4), centers=[[2, 0]], pad=7.0)
    # window rows -1, 0; columns 0..3: the top row is padding
    assert out[0, 0].tolist() == [[7.0, 7.0]]
    assert out[0, 1].tolist() == [[(7 + 7 + 0 + 0) / 4, (7 + 7 + 1 + 0) / 4]]


def test_sequential_mean_is_not_pairwise():
    v = np.array([1e16, 1.0, -1e16, 1.0] + [0.0] * 12).reshape(1, 4, 4)
    attrs = lambda e: {"elevation": v[0]}
    out = O.observe(["elevation"], np.zeros((1, 4, 4), np.uint8), attrs, normalize=False, pool=4)
    s = 1e16
    for x in v.reshape(-1)[1:]:
        s = s + x
    assert out[0, 0, 0, 0] == np.float32(s / 16)


def test_agents_later_entries_win_and_moved_ids_leave():
    H = W = 4
    entries = [(0, 0, 1), (0, 0, 2), (1, 1, 3), (2, 2, 3), (3, 3, 0), (9, 0, 4), (1, 0, 5), (1, 0, 6), (2, 0, 6)]
    m = O.agent_map(entries, H, W)
    assert m[0, 0] == 2 and m[1, 1] == 0 and m[2, 2] == 3 and m[3, 3] == 0
    assert m[0, 1] == 0 and m[0, 2] == 6                 # 5 was overwritten by 6, then 6 moved on
    out = O.observe(["agent_positions"], MAP, None, agents=np.array([entries]))
    assert (out[0, 0] == m).all()
    ref = np.zeros((H, W), np.int64)                      # the reference's loop, literally (simulation.py:493-494)
    for col, row, aid in entries:
        if aid > 0 and col < W:
            ref[ref == aid] = 0
            ref[row][col] = aid
    assert (ref == m).all()


def test_bf16_rounding_matches_torch():
    torch = pytest.importorskip("torch")
    x = np.array([1.0, 1.00390625, 1.005859375, 1.0078125 + 2 ** -9, 3.14159, -2.71828, 1e-30, 65504.0, 0.0], dtype=np.float32)
    x = np.concatenate([x, np.random.default_rng(0).standard_normal(10000).astype(np.float32) * 1000])
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert (O.bf16_bits(x) == want).all()


def test_agents_from_map():
    m = np.zeros((4, 5), np.int64)
    m[1, 3] = 7
    m[2, 0] = 2
    a = agents_from_map(m)
    assert a.shape == (1, 2, 3) and sorted(map(tuple, a[0].tolist())) == [(0, 2, 2), (3, 1, 7)]
    assert (O.agent_map(a[0], 4, 5) == m).all()
    m[0, 0] = 7
    with pytest.raises(ValueError):
        agents_from_map(m)


# ------------------------------------------------------------------ the spec builder's checks
@pytest.mark.parametrize("kw,match", [
    (dict(channels="fire_map"), "list of channel names"),
    (dict(channels=[]), "1 to 32"),
    (dict(channels=["fire_map"] * 33), "1 to 32"),
    (dict(channels=["fuel"]), "unknown channel"),
    (dict(pool=3), "not divisible"),
    (dict(pool=0), "pool must be"),
    (dict(pool=2.0), "integer"),
    (dict(pool_mode="median"), "pool_mode"),
    (dict(pool_mode={"elevation": "max"}), "not one of the channels"),
    (dict(pool_mode={"fire_map": "min"}), "pool_mode of"),
    (dict(envs=[0, 4]), "outside"),
    (dict(envs=[]), "non-empty"),
    (dict(envs=[[0]]), "non-empty"),
    (dict(crop=(4, 4)), "needs centers"),
    (dict(centers=[[0, 0]] * 4), "only used with a crop"),
    (dict(crop=(0, 4), centers=[[0, 0]] * 4), "positive"),
    (dict(crop=(6, 4), centers=[[0, 0]] * 4, pool=4), "not divisible"),
    (dict(crop=(4, 4), centers=[[0, 0]] * 3), "shape"),
    (dict(crop=(4, 4), centers=np.zeros((4, 2)) + 0.5), "integers"),
    (dict(agents=np.zeros((4, 3), np.int32)), "shape"),
    (dict(agents=np.zeros((4, 257, 3), np.int32)), "at most 256"),
    (dict(agents=np.full((4, 1, 3), 2 ** 31)), "int32"),
    (dict(dtype="float16"), "dtype"),
])
def test_spec_errors(kw, match):
    args = dict(channels=["fire_map"], n_envs=4, H=8, W=12)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        ObsSpec(**args)


def test_spec_out_checks():
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match="CUDA tensor"):
        ObsSpec(["fire_map"], 2, 8, 8, out=torch.empty((2, 1, 8, 8)))
    with pytest.raises(ValueError, match="CUDA int32 tensor"):
        ObsSpec(["fire_map"], 2, 8, 8, crop=(2, 2), centers=torch.zeros((2, 2), dtype=torch.int32))


def test_spec_shape_codes_and_params():
    torch = pytest.importorskip("torch")
    s = ObsSpec(["fire_map", "elevation", "agent_positions", "fire_map"], 5, 64, 96, envs=[3, 3, 0], pool=8,
                pool_mode={"elevation": "max"}, crop=(32, 48), centers=np.array([[1, 2], [3, 4], [5, 6]]),
                agents=np.zeros((3, 2, 3), np.int64), dtype=torch.bfloat16, pad=-2.0)
    assert s.shape == (3, 4, 4, 6)
    assert s.codes == [CHANNELS["fire_map"], 11, 14, 0] and s.modes == [0, 1, 0, 0]
    p = s.params()
    assert p.n_channels == 4 and p.pool == 8 and (p.crop_h, p.crop_w) == (32, 48) and p.dtype == 1 and p.pad == -2.0
    assert p.agents_k == 2 and p.centers and p.agents and not p.centers_device


def test_observe_api_exists_on_every_layer():
    from simfire_amd.engine import FireEngine
    from simfire_amd.simulation import BatchedFireSimulation, FireSimulation
    for cls in (FireEngine, BatchedFireSimulation, FireSimulation):
        assert callable(getattr(cls, "observe", None)), cls
