"""The binding's one call frame and its zero-copy views on the GPU.  Every call that hands the library a torch tensor is made with
tensors the test keeps no reference to: in async mode each must stay alive until ``sync()`` - the handle's stream may still touch
its memory - and be gone after it; with async off each is gone when the call returns.  Each zero-copy view has the shape, dtype,
strides and address the library reports.  Run with ``pytest -m gpu``."""
import ctypes as C
import gc
import weakref

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E, H, W, K = 4, 24, 40, 2


@pytest.fixture(scope="module")
def eng():
    from simfire_amd.engine import FireEngine
    from simfire_amd.parameters import fuel_planes
    rng = np.random.default_rng(11)
    eng = FireEngine((H, W), n_envs=E, per_env_terrain=True, pixel_scale=30.0, max_fire_duration=4)
    for e in range(E):
        w0, de, mx, sg = fuel_planes(rng.choice([1, 2, 4, 5], size=(H, W)))
        eng.set_layers(w0, de, mx, sg, np.zeros((H, W)), np.full((H, W), 600.0 + 50.0 * e), np.full((H, W), 45.0 * e), env=e)
    xy = np.array([[20, 12], [10, 6], [30, 18], [5, 20]], dtype=np.int32)
    eng.reset(xy)
    eng.enable_arrival(True)
    eng.values_set(rng.integers(0, 9, size=(H, W)).astype(np.int32))
    eng.agents_create(K, xy, n_updates=1)
    eng.agents_place(np.arange(E), np.array([[[2, 2], [W - 3, H - 3]]] * E, dtype=np.int32))
    eng.episodes_set(5, ignition_box=(4, 4, W - 5, H - 5))
    eng.step(3)
    yield eng
    eng.close()


def _calls(eng):
    """name -> a function that makes the call with fresh tensors and returns weak references to every one of them."""
    import torch
    dev = torch.device("cuda:0")

    def new(shape, dtype, fill=0):
        return torch.full(shape, fill, dtype=dtype, device=dev)

    def refs(*tensors):
        return [weakref.ref(t) for t in tensors]

    def observe():
        out, agents = new((E, 2, H, W), torch.float32), eng.agents_device().clone()
        eng.observe(["fire_map", "agent_positions"], agents=agents, out=out)
        return refs(out, agents)

    def render():
        out = new((E, H, W, 3), torch.uint8)
        eng.render(out=out)
        return refs(out)

    def distance():
        points, out = eng.agents_device().clone(), new((E, K), torch.float32)
        eng.distance(("BURNING", "BURNED"), points=points, out=out)
        return refs(points, out)

    def reach():
        passable, points = new((H, W), torch.uint8, 1), eng.agents_device().clone()
        res = eng.reach(passable=passable, points=points)
        assert set(res) == {"count", "point_in"}
        return refs(passable, points, *res.values())

    def ensemble_stats():
        res = eng.ensemble_stats([[0, 1], [2, 3]], horizons=(2, -1), count=True, first=True)
        assert set(res) == {"count", "prob", "first"}
        return refs(*res.values())

    def agents_step():
        t = [new((E, K), torch.int32), new((E,), torch.float32), new((E,), torch.bool), new((E, 4), torch.int32), new((E,), torch.int32),
             new((E,), torch.float64)]
        eng.agents_step(t[0], reward=t[1], done=t[2], terms=t[3], final_len=t[4], final_ret=t[5])
        return refs(*t)

    def reset_where():
        mask, xy = new((E,), torch.uint8, 1), new((E, 2), torch.int32, 7)
        eng.reset_where(mask, xy)
        return refs(mask, xy)

    def episodes_begin():
        mask = new((E,), torch.bool, True)
        eng.episodes_begin(mask)
        return refs(mask)

    def set_wind():
        speed, direction = new((E,), torch.float64, 500.0), new((E,), torch.float64, 90.0)
        eng.set_wind(speed, direction)
        return refs(speed, direction)

    def save_state():
        out = new((2 * eng.state_bytes(),), torch.uint8)
        assert eng.save_state([1, 2], out=out) is out
        return refs(out)

    def load_state():
        blob = torch.from_numpy(eng.save_state([0, 3])).to(dev)
        eng.load_state([3, 0], blob)
        return refs(blob)

    return dict(observe=observe, render=render, distance=distance, reach=reach, ensemble_stats=ensemble_stats, agents_step=agents_step,
                reset_where=reset_where, episodes_begin=episodes_begin, set_wind=set_wind, save_state=save_state, load_state=load_state)


NAMES = ("observe", "render", "distance", "reach", "ensemble_stats", "agents_step", "reset_where", "episodes_begin", "set_wind",
         "save_state", "load_state")


def test_every_device_tensor_call_is_covered(eng):
    assert tuple(_calls(eng)) == NAMES


@pytest.mark.parametrize("name", NAMES)
def test_async_calls_keep_their_tensors_until_sync(eng, name):
    eng.sync()
    eng.set_async(True)
    try:
        kept = _calls(eng)[name]()
        gc.collect()
        assert kept and all(r() is not None for r in kept), name           # the handle's stream may still touch them
        eng.sync()
        gc.collect()
        assert all(r() is None for r in kept), name
        assert not eng._blobs_in_flight
    finally:
        eng.set_async(False)


@pytest.mark.parametrize("name", NAMES)
def test_synchronous_calls_keep_nothing(eng, name):
    assert not eng.async_mode
    kept = _calls(eng)[name]()
    gc.collect()
    assert kept and all(r() is None for r in kept), name
    assert not eng._blobs_in_flight


def test_zero_copy_views(eng):
    import torch
    L, h = eng._L, eng._h
    eng.sync()

    def same(t, ptr, shape, dtype, byte_strides):
        assert t.is_cuda and t.device.index == 0 and tuple(t.shape) == shape and t.dtype == dtype
        assert t.data_ptr() == ptr and tuple(s * t.element_size() for s in t.stride()) == byte_strides

    p = C.c_void_p()
    assert L.sf_agents_device(h, C.byref(p)) == 0
    same(eng.agents_device(), p.value, (E, K, 3), torch.int32, (K * 12, 12, 4))

    ptrs = [C.c_void_p(), C.c_void_p(), C.c_void_p()]
    assert L.sf_episodes_device(h, *[C.byref(q) for q in ptrs]) == 0
    ep = eng.episodes_torch()
    assert set(ep) == {"index", "ignition", "wind"}
    same(ep["index"], ptrs[0].value, (E,), torch.int32, (4,))
    same(ep["ignition"], ptrs[1].value, (E, 2), torch.int32, (8, 4))
    same(ep["wind"], ptrs[2].value, (E, 2), torch.float64, (16, 8))

    pitch, stride = C.c_int64(), C.c_int64()
    assert L.sf_arrival_device(h, C.byref(p), C.byref(pitch), C.byref(stride)) == 0
    same(eng.arrival_torch(), p.value, (E, H, W), torch.int32, (stride.value, pitch.value, 4))
    assert pitch.value >= 4 * W and stride.value >= H * pitch.value

    d, t = C.c_void_p(), C.c_void_p()
    assert L.sf_values_device(h, C.byref(d), C.byref(stride), C.byref(t)) == 0
    damage, loss = eng.values_torch()
    same(damage, d.value, (E,), torch.int64, (stride.value,))
    same(loss, t.value, (E,), torch.int64, (8,))
    assert damage.cpu().tolist() == eng.damage().tolist()

    ptr, pitch, stride = eng.fire_map_device()
    same(eng.fire_maps_torch(), ptr, (E, H, W), torch.uint8, (stride, pitch, 1))
    assert (eng.fire_maps_torch().cpu().numpy() == eng.fire_maps()).all()
