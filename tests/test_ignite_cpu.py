"""Ignitions during an episode without a GPU: the wrapper over the sprite-list oracle
(``tests/_ignite_oracle.py``) against the fixtures recorded from the real reference (``tests/golden/ignite_*.npz``), its invariances,
the C ABI entries as the header, the binding and the built library have them, the argument errors of ``FireEngine.ignite`` raised
before the library is touched, and the source scans of the new kernel file."""
import ctypes as C
import glob
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _ignite_oracle  # noqa: E402
from oracle import fire_sprites  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = sorted(os.path.basename(p)[7:-4] for p in glob.glob(os.path.join(GOLDEN, "ignite_*.npz")))
NEW = ("sf_ignite", "sf_ignite_device")


def load(name):
    d = dict(np.load(os.path.join(GOLDEN, f"ignite_{name}.npz")))
    d["max_time"] = None if np.isnan(d["max_time"]) else float(d["max_time"])
    return d


def wrapper(d, rtable=None):
    return _ignite_oracle.IgniteFire(tuple(int(v) for v in d["shape"]), tuple(int(v) for v in d["init_pos"]),
                                     d["rtable"] if rtable is None else rtable, int(d["max_fire_duration"]), float(d["pixel_scale"]),
                                     float(d["update_rate"]), max_time=d["max_time"], attenuate_line_ros=bool(d["attenuate"]),
                                     diagonal_spread=bool(d["diagonal"]))


def rows_of(d, s, change=None):
    """The fixture's control-line points and ignition rows of update ``s``; ``change`` rewrites the ignition rows."""
    pts = [(int(x), int(y), int(t)) for (u, x, y, t) in d["schedule"] if u == s]
    ign = [(int(x), int(y)) for (u, x, y) in d["ignite"] if u == s]
    return pts, (change(ign) if change else ign)


def replay(d, change=None, check=True):
    """Every update of the fixture through the wrapper; returns it.  ``check``: against the reference's records, bit for bit."""
    w = wrapper(d)
    for s in range(len(d["status"])):
        pts, ign = rows_of(d, s, change)
        w.apply_mitigation(pts)
        w.ignite(ign)
        w.update()
        if check:
            assert (w.fire_map == d["fire_maps"][s]).all(), f"map differs at update {s}"
            assert int(w.running) == int(d["status"][s]) and w.fire.elapsed_time == d["elapsed"][s], f"status differs at update {s}"
    if check:
        assert (w.fire.burn == d["burn"]).all()
    return w


def test_there_are_fixtures():
    assert len(FIXTURES) >= 3 and not glob.glob(os.path.join(GOLDEN, "traj_*ignite*"))
    for name in FIXTURES:
        d = load(name)
        assert os.path.getsize(os.path.join(GOLDEN, f"ignite_{name}.npz")) < 100 * 1024
        assert max(d["shape"]) <= 48 and len(d["status"]) <= 30 and int(d["n_lit"]) >= 3
        assert len(d["ignite"]) > int(d["n_lit"])          # some rows are repeats or lie on cells that are not UNBURNED
    assert any(not load(n)["diagonal"] for n in FIXTURES) and any(load(n)["attenuate"] and len(load(n)["schedule"]) for n in FIXTURES)


@pytest.mark.parametrize("name", FIXTURES)
def test_wrapper_replays_the_reference(name):
    replay(load(name))


@pytest.mark.parametrize("name", FIXTURES)
def test_order_repeats_and_dead_rows_do_not_matter(name):
    d = load(name)
    rng = np.random.default_rng(7)
    base = replay(d, check=False)

    def same(w):
        return (w.fire_map == base.fire_map).all() and (w.fire.burn == base.fire.burn).all() and (w.arrival == base.arrival).all() \
            and w.fire.sprites == base.fire.sprites and w.fire.durations == base.fire.durations and w.steps == base.steps
    assert same(replay(d, change=lambda p: p[::-1]))
    assert same(replay(d, change=lambda p: [p[i] for i in rng.permutation(len(p))]))
    assert same(replay(d, change=lambda p: p + p[:3] + p))
    # rows on cells that are not UNBURNED: the maps of the update before name them
    seen = {"s": 0}

    def with_dead(p):
        s = seen["s"]
        seen["s"] += 1
        if s == 0:
            return p + [tuple(int(v) for v in d["init_pos"])]
        ys, xs = np.nonzero(d["fire_maps"][s - 1] != fire_sprites.UNBURNED)
        lines = [(int(x), int(y)) for (u, x, y, t) in d["schedule"] if u == s]
        return [(int(xs[i]), int(ys[i])) for i in rng.choice(len(ys), size=min(5, len(ys)), replace=False)] + p + lines
    assert same(replay(d, change=with_dead))


def test_no_rows_is_the_plain_oracle():
    d = load(FIXTURES[0])
    w = wrapper(d)
    plain = fire_sprites.SpriteFire(tuple(int(v) for v in d["shape"]), tuple(int(v) for v in d["init_pos"]), int(d["max_fire_duration"]),
                                    float(d["pixel_scale"]), float(d["update_rate"]), rtable=d["rtable"], max_time=d["max_time"],
                                    attenuate_line_ros=bool(d["attenuate"]), diagonal_spread=bool(d["diagonal"]))
    m = np.zeros(tuple(int(v) for v in d["shape"]), dtype=np.int64)
    m[d["init_pos"][1], d["init_pos"][0]] = fire_sprites.BURNING
    for _ in range(12):
        assert w.ignite([]) == []
        w.update()
        m, _st = plain.update(m)
        assert (w.fire_map == m).all() and (w.fire.burn == plain.burn).all() and w.fire.sprites == plain.sprites
        assert w.fire.durations == plain.durations and w.fire.elapsed_time == plain.elapsed_time


def test_canonical_insert_keeps_the_order():
    sprites, durations = [(5, 5), (1, 2), (7, 2), (3, 4)], [2, 0, 0, 0]
    s, t = _ignite_oracle.canonical_insert(sprites, durations, [(9, 9), (0, 2), (4, 2), (3, 3)])
    assert s == [(5, 5), (0, 2), (1, 2), (4, 2), (7, 2), (3, 3), (3, 4), (9, 9)] and t == [2] + [0] * 7
    s, t = _ignite_oracle.canonical_insert([(5, 5), (6, 6)], [3, 1], [(2, 8), (1, 1)])      # no sprite of age 0 there yet
    assert s == [(5, 5), (6, 6), (1, 1), (2, 8)] and t == [3, 1, 0, 0]


def test_header_binding_and_library_agree():
    from simfire_amd import _lib
    header = open(os.path.join(ROOT, "include", "simfire_hip.h")).read()
    for name in NEW:
        assert name in _lib.SIGNATURES, f"simfire_amd/_lib.py does not bind {name}"
        assert _lib.SIGNATURES[name] == [C.c_void_p, C.c_void_p, C.c_int32]
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header, re.S)
        assert decl, f"include/simfire_hip.h does not declare {name}"
        assert len(re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")) == 3
    assert re.search(r"fire\.py:102-103.*?fire\.py:566-587.*?\bint sf_ignite\(", header, re.S)      # the comment cites what it follows
    lib = _lib.load()                                     # (raises if the library has not been built)
    for name in NEW:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name]
    # what needs no device: the refusals in front of the prologue
    assert lib.sf_ignite(None, None, 0) == _lib.SF_EINVAL and lib.sf_ignite_device(None, None, 0) == _lib.SF_EINVAL
    assert b"null handle" in lib.sf_last_error()


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


@pytest.mark.parametrize("points, exc", [
    ([[0, 1]], ValueError),                              # not [n, 3] or [n, 4]
    ([[0, 1, 1, 0, 0]], ValueError),
    ([0, 1, 1], ValueError),                             # flat
    ([[[0, 1, 1]]], ValueError),
    ([[0.0, 1.0, 1.0]], ValueError),                     # not integers
    ([[0, 1, 1, 3]], ValueError),                        # reserved != 0
    ([[0, 1, 1], [4, 1, 1]], IndexError),                # environment out of range
    ([[-1, 1, 1]], IndexError),
    ([[0, 30, 5]], ValueError),                          # x == W
    ([[0, 3, 20]], ValueError),                          # y == H
    ([[0, -1, 5]], ValueError),
    ([[0, 3, -1, 0]], ValueError),
    ([[0, 2 ** 31, 0]], ValueError),
])
def test_ignite_argument_errors(points, exc):
    with pytest.raises(exc):
        _engine().ignite(points)


def test_ignite_without_rows_is_a_no_op():
    _engine().ignite([])
    _engine().ignite(np.zeros((0, 3), dtype=np.int32))
    _engine().ignite(np.zeros((0, 4), dtype=np.int64))


def test_ignite_rows_are_padded_with_the_reserved_zero():
    from simfire_amd import _args
    q = _args.ignite_rows([[3, 29, 19], [0, 0, 0]], 4, 20, 30, "ignite")
    assert q.dtype == np.int32 and q.flags.c_contiguous and q.tolist() == [[3, 29, 19, 0], [0, 0, 0, 0]]
    assert _args.ignite_rows(np.array([[1, 2, 3, 0]], dtype=np.int64), 4, 20, 30, "ignite").tolist() == [[1, 2, 3, 0]]


def test_ignite_torch_refuses_host_tensors_and_other_shapes():
    import torch
    for t in (torch.zeros((2, 4), dtype=torch.int32), np.zeros((2, 4), dtype=np.int32), [[0, 1, 1, 0]]):
        with pytest.raises(ValueError):
            _engine().ignite_torch(t)


def test_simulations_forward():
    from simfire_amd.simulation import BatchedFireSimulation
    from simfire_amd.vecenv import BatchedFireEnv
    sim = BatchedFireSimulation.__new__(BatchedFireSimulation)
    sim._engine = _engine()
    calls = []
    sim._engine.ignite = lambda p: calls.append(np.asarray(p).tolist())
    sim.ignite([[1, 2, 3]])
    env = BatchedFireEnv.__new__(BatchedFireEnv)
    env.sim = sim
    env.ignite([[0, 4, 5]])
    assert calls == [[[1, 2, 3]], [[0, 4, 5]]]
    sim._engine = _engine()
    with pytest.raises(IndexError):
        sim.ignite([[9, 1, 1]])


def _code(path):
    """A source file without its comments."""
    text = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group(0).count("\n"), open(path).read(), flags=re.S)
    return "\n".join(line.split("//")[0] for line in text.split("\n"))


def test_kernel_file_scans():
    """The new kernel file addresses cells through ``sf_cells.h`` / ``sf_common.h`` alone, holds no byte-permute builtin and no inline
    assembly, and meets shared bitmap words with ``atomicOr``; the book has the one new event and the host file reads flags through it."""
    csrc = os.path.join(ROOT, "simfire_amd", "csrc")
    k = _code(os.path.join(csrc, "sf_ignite_kernels.h"))
    assert "__builtin_amdgcn_perm" not in k and "asm" not in k
    assert not re.search(r"\b(kBlStatus|cells_env)\b", k) and "* 128" not in k
    for helper in ("bl_status(", "bl_mask_beside(", "cell_status(", "age_store(", "age_load(", "slot_of("):
        assert helper in k, helper
    assert len(re.findall(r"\batomicOr\(", k)) == 3 and "int4" in k
    assert not re.search(r"\ba\.commit\[e\]\s*=", k) and "res_block" not in k      # neither EnvState nor the result row
    book = open(os.path.join(csrc, "sf_planes.h")).read()
    assert re.search(r"void cells_ignited\(\) \{ fire_rows_ = 0; row_fresh_ = false; \}", book)
    host = _code(os.path.join(csrc, "sf_host_ignite.h"))
    assert host.count("begin_call(s, \"sf_ignite") == 2 and host.count("kStateCall") == 2 and "planes.cells_ignited()" in host
    assert "arrival_scan(s)" in host and "value_recount(s)" in host and host.count("finish_call(s, nullptr, !s->async, nullptr)") == 2
    unit = open(os.path.join(csrc, "simfire_hip.hip")).read()
    assert '#include "sf_ignite_kernels.h"' in unit and '#include "sf_host_ignite.h"' in unit
