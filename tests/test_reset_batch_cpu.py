"""Batched resets without a GPU: the C ABI entries as the header, the binding and the built library have them, and every argument
error of ``FireEngine.reset_envs`` / ``reset_where`` / ``BatchedFireSimulation.reset_done`` raised before the library is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sf_reset_envs", "sf_reset_where")


def test_header_binding_and_library_agree():
    from simfire_amd import _lib
    header = open(os.path.join(ROOT, "include", "simfire_hip.h")).read()
    for name in NEW:
        assert name in _lib.SIGNATURES
        assert re.search(r"\bint %s\(" % name, header), name
    # int sf_reset_envs(sf_sim *, int32_t n, const int32_t *envs, const int32_t *xy)
    assert _lib.SIGNATURES["sf_reset_envs"] == [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    # int sf_reset_where(sf_sim *, const uint8_t *device_mask, const int32_t *xy, int32_t xy_device_pointer)
    assert _lib.SIGNATURES["sf_reset_where"] == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
    decl = {n: re.search(r"\bint %s\(([^;]*)\);" % n, header, re.S).group(1) for n in NEW}
    assert len(re.sub(r"/\*.*?\*/", "", decl["sf_reset_envs"], flags=re.S).split(",")) == 4
    assert len(re.sub(r"/\*.*?\*/", "", decl["sf_reset_where"], flags=re.S).split(",")) == 4
    assert re.search(r"const uint8_t \*device_mask", decl["sf_reset_where"])
    lib = _lib.load()                                     # (raises if the library has not been built)
    for name in NEW:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name]


class _NoLibrary:
    """Stands in for the loaded library: any entry looked up on it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was touched ({name}) before the arguments were checked")


def _engine(H=20, W=30, E=4):
    from simfire_amd.engine import FireEngine
    eng = FireEngine.__new__(FireEngine)
    eng._L = _NoLibrary()
    eng._h = None
    eng.H, eng.W, eng.n_envs = H, W, E
    eng.async_mode = False
    eng._blobs_in_flight = []
    return eng


@pytest.mark.parametrize("envs, xy, exc", [
    ([0, 1], [[1, 1]], ValueError),                      # lengths differ
    ([0, 1], [[1, 1, 1], [2, 2, 2]], ValueError),        # not [n, 2]
    ([0, 1], [1, 1, 2, 2], ValueError),                  # flat
    ([[0, 1]], [[1, 1], [2, 2]], ValueError),            # envs not a list
    ([0.5], [[1, 1]], ValueError),                       # envs not integers
    ([0], [[1.5, 1.0]], ValueError),                     # ignitions not integers
    ([4], [[1, 1]], IndexError),                         # environment out of range
    ([-1], [[1, 1]], IndexError),
    ([0, 1], [[1, 1], [30, 5]], ValueError),             # x == W
    ([0, 1], [[1, 20], [3, 5]], ValueError),             # y == H
    ([0], [[-1, 5]], ValueError),
])
def test_reset_envs_argument_errors(envs, xy, exc):
    with pytest.raises(exc):
        _engine().reset_envs(envs, xy)


def test_reset_envs_empty_list_is_a_no_op():
    _engine().reset_envs([], np.zeros((0, 2), dtype=np.int32))


@pytest.mark.parametrize("mask, xy", [
    (None, None),                                                    # no ignitions
    (None, np.zeros((3, 2), dtype=np.int32)),                        # not [n_envs, 2]
    (None, np.zeros((4, 2))),                                        # not integers
    (None, np.array([[0, 0], [1, 1], [30, 2], [3, 3]])),             # off the grid in a host array
    (None, np.array([[0, 0], [1, 1], [2, -1], [3, 3]])),
    (np.ones(4, dtype=np.uint8), np.zeros((4, 2), dtype=np.int32)),  # a host mask
    ([1, 0, 0, 1], np.zeros((4, 2), dtype=np.int32)),
])
def test_reset_where_argument_errors(mask, xy):
    with pytest.raises(ValueError):
        _engine().reset_where(mask, xy)


def test_reset_where_refuses_host_tensors():
    import torch
    xy = np.zeros((4, 2), dtype=np.int32)
    for mask in (torch.ones(4, dtype=torch.uint8), torch.ones(4, dtype=torch.bool)):      # CPU tensors
        with pytest.raises(ValueError):
            _engine().reset_where(mask, xy)


def _sim(pending):
    from simfire_amd.simulation import BatchedFireSimulation
    sim = BatchedFireSimulation.__new__(BatchedFireSimulation)
    sim.n_envs = 4
    sim.ignitions = np.array([[1, 1], [2, 2], [3, 3], [4, 4]], dtype=np.int32)
    sim._pending = pending
    sim._engine = _engine()
    return sim


def test_reset_done_with_a_pending_layer_seed_raises():
    with pytest.raises(ValueError, match=r"reset\(envs\)"):
        _sim({2: {"elevation"}}).reset_done()
    import torch
    with pytest.raises(ValueError, match=r"reset\(envs\)"):
        _sim({0: {"fuel"}}).reset_done(torch.ones(4, dtype=torch.uint8))


def test_reset_with_a_list_is_one_engine_call():
    sim = _sim({})
    calls = []
    sim._engine.reset_envs = lambda envs, xy: calls.append((list(envs), np.asarray(xy).tolist()))
    sim._engine.reset_env = lambda *a: pytest.fail("reset(envs) looped over reset_env")
    sim.reset([3, 1, 3])
    assert calls == [([3, 1, 3], [[4, 4], [2, 2], [4, 4]])]
    sim.reset([])
    assert len(calls) == 1
    sim.ignitions[2] = (30, 0)                           # off the 20 x 30 grid: refused before the library is touched
    sim._engine = _engine()
    with pytest.raises(ValueError):
        sim.reset([0, 2])
    with pytest.raises(ValueError):
        sim.reset_done()


def test_segment_capacity_covers_the_largest_selection():
    """The slice table (``env_segs``, simfire_hip.hip) against the capacity of the kernel arguments that carry a selection of it
    (``kEnvSegs``, sf_env_segs.h), from the source text: every ``add(kind, ...)`` of the table counted by kind - the loops by their
    trip counts, the cells of the current layout by the larger branch - and summed over the kinds a fork and a batched reset name."""
    csrc = os.path.join(ROOT, "simfire_amd", "csrc")
    header = open(os.path.join(csrc, "sf_env_segs.h")).read()
    # (the host code of the main unit: simfire_hip.hip and the fragments it includes)
    host = "".join(open(os.path.join(csrc, f)).read() for f in sorted(f for f in os.listdir(csrc) if f == "simfire_hip.hip" or f == "sf_handle.h" or f.startswith("sf_host_")))
    kinds = re.findall(r"^\s*(kSeg\w+) = 1u << \d+,", header, re.M)
    assert len(kinds) == len(set(kinds)) >= 14
    cap = int(re.search(r"constexpr int kEnvSegs = (\d+);", header).group(1))
    body = re.search(r"static int env_segs\(.*?\n\{\n(.*?)\n\}\n", host, re.S).group(1)
    count = dict.fromkeys(kinds, 0)
    branch = []                                          # slices of kSegCells on each side of the layout branch
    for line in body.splitlines():
        m = re.search(r"\badd\((kSeg\w+),", line)
        if not m or "auto add" in line:
            continue
        loop = re.search(r"for \(int k = 0; k < (\d+); \+\+k\)", line)
        if m.group(1) == "kSegCells":
            branch.append(line)
        else:
            count[m.group(1)] += int(loop.group(1)) if loop else 1
    assert len(branch) == 3 and "planes.blocked()" in branch[0]   # the blocked plane | status + the sprite-mask plane
    count["kSegCells"] = 2
    assert all(count.values()), count                    # every kind has a slice
    assert len(re.findall(r"\badd\(", host)) == len(re.findall(r"\badd\(kSeg", body))          # (no second table beside it)

    def selection(name):
        expr = re.search(r"constexpr unsigned %s = ([^;]*);" % name, header).group(1)
        names = [k.strip() for k in expr.split("|")]
        assert set(names) <= set(kinds) and len(names) == len(set(names)), names
        return sum(count[k] for k in names)

    fork, reset = selection("kForkKinds"), selection("kResetKinds")
    assert (fork, reset) == (22, 14)
    assert sum(count.values()) == 23                     # (the fork leaves out snap)
    assert max(fork, reset) <= cap
    for arg in (r"struct CopyList \{\s*EnvSeg seg\[kEnvSegs\];", r"EnvSeg seg\[kEnvSegs\];\s*// the slices to zero"):
        assert re.search(arg, open(os.path.join(csrc, "sf_state_kernels.h")).read() + open(os.path.join(csrc, "sf_reset_kernels.h")).read())
