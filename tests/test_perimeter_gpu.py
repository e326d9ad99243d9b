"""Fire perimeters on the GPU (``sf_perimeter``).  The yardstick is ``tests/_perimeter_oracle.py`` - a tracer
that walks the crack edges, with its own self-checks - fed with the maps fetched AFTER the call (a getter may convert the current
plane).  Every comparison is equality: the answer is integers and its order is canonical, so no bit may depend on how the kernel
schedules its work.  Capacities are chosen from the oracle, tight, so that no environment overflows - except in the overflow test.
Run with ``pytest -m gpu``."""
import ctypes as C
import os

import numpy as np
import pytest

import _arrival_worlds as aw
import _perimeter_oracle as po
import _perimeter_worlds as pw

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tests", "golden", "configs")
LISTS = ("vertices", "loop_start", "loop_area", "loop_edges")
_cache = {}


def _want(mask, conn, simplify=True):
    """The oracle's answer, computed once per (set, connectivity, simplify) and left unchanged."""
    mask = np.ascontiguousarray(mask, dtype=bool)
    key = (mask.shape, mask.tobytes(), conn, bool(simplify))
    if key not in _cache:
        _cache[key] = po.answer(mask, conn, simplify)
    return _cache[key]


def _engine(H, W, E, mode, diag=True, R8=None):
    from simfire_amd.engine import FireEngine
    eng = FireEngine(n_envs=E, **pw.engine_kwargs(H, W, diag=diag))
    m = aw.mode_settings(mode)
    eng.set_fused(m["fused"])
    if m.get("tuning"):
        eng.set_tuning(**m["tuning"])
    eng.set_rtable(pw.slow_table(H, W) if R8 is None else R8)
    return eng


def _loaded(H, W, masks, mode, diag=True):
    """An engine with one environment per mask, each loaded through ``load_fire_map``; ``run``: one update behind it (under the slow
    table it ignites nothing, so BURNING | BURNED is still the mask), which leaves the cells in the blocked plane."""
    E = len(masks)
    b = _engine(H, W, E, mode, diag)
    b.reset(np.zeros((E, 2), dtype=np.int32))
    for e, m in enumerate(masks):
        b.load_fire_map(e, pw.fire_map(m))
    if mode == "run":
        b.step(1)
    return b


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _caps(wants):
    """Tight capacities: the largest answer of the call fits exactly."""
    return dict(max_edges=max([w["edges"] for w in wants] + [0]), max_vertices=max([w["n_vertices"] for w in wants] + [1]),
                max_loops=max([w["loops"] for w in wants] + [1]))


def _ask(eng, **kw):
    """Every output of a traced ``perimeter`` call as NumPy arrays; the call changes neither the layout nor the launch kind."""
    lay, kind = eng.cell_layout(), eng.last_launch_kind()
    r = eng.perimeter(front=True, trace=True, **kw)
    eng.sync()                                               # (a handle in async mode has only enqueued)
    assert (eng.cell_layout(), eng.last_launch_kind()) == (lay, kind)
    assert all(v.is_cuda for v in r.values())
    return {k: v.cpu().numpy() for k, v in r.items()}, lay


def _same(r, i, want, tag):
    """Row ``i`` of every output equals the oracle's answer."""
    for name in ("edges", "cells", "loops", "holes", "n_vertices"):
        assert r[name].dtype == np.int32 and int(r[name][i]) == want[name], (tag, i, name, int(r[name][i]), want[name])
    assert r["front"].dtype == np.uint8 and (r["front"][i] == want["front"]).all(), (tag, i, "front", np.argwhere(r["front"][i] != want["front"])[:5].tolist())
    nl, nv = want["loops"], want["n_vertices"]
    assert r["loop_start"][i][:nl + 1].tolist() == want["loop_start"].tolist(), (tag, i, "loop_start")
    assert r["loop_area"][i][:nl].tolist() == want["loop_area"].tolist(), (tag, i, "loop_area")
    assert r["loop_edges"][i][:nl].tolist() == want["loop_edges"].tolist(), (tag, i, "loop_edges")
    bad = np.argwhere(r["vertices"][i][:nv] != want["vertices"])
    assert not len(bad), (tag, i, "vertices", len(bad), bad[:5].tolist(), r["vertices"][i][:nv][bad[:5, 0]].tolist(), want["vertices"][bad[:5, 0]].tolist())


def _sets(maps, mask=6):
    return [po.mask_of_status(m, mask) for m in maps]


# ---------------------------------------------------------------------------------------------- 1. the scenes
@pytest.mark.parametrize("shape", pw.SCENE_SHAPES, ids=["%dx%d" % s for s in pw.SCENE_SHAPES])
@pytest.mark.parametrize("mode", ["fused0", "run"])
def test_scenes(shape, mode):
    """Every scene of ``_perimeter_worlds.scenes`` in an environment of its own, through ``load_fire_map``.  ``fused0``: read in the
    row-major layout as loaded.  ``run``: one update first, so that the cells lie in the blocked plane; the maps are fetched after the
    calls.  Both connectivities, ``simplify`` on and off; the summary form gives the same ``edges``, ``cells`` and ``front``."""
    H, W = shape
    sc = pw.scenes(H, W)
    b = _loaded(H, W, [s["mask"] for s in sc], mode)
    E = len(sc)
    got = []
    for conn, simplify in ((4, True), (8, True), (4, False), (8, False)):
        caps = _caps([_want(s["mask"], conn, simplify) for s in sc])
        got.append((conn, simplify, _ask(b, connectivity=conn, simplify=simplify, **caps)))
    deflt = _ask(b, **_caps([_want(s["mask"], 8) for s in sc]))[0]      # (None: the handle's diagonal_spread - on)
    cheap = b.perimeter(front=True)
    only_front = b.perimeter(counts=False, front=True)
    maps = b.fire_maps()
    sets = _sets(maps)
    for e, s in enumerate(sc):
        assert (sets[e] == s["mask"]).all(), (shape, mode, s["name"])       # (so the capacities were the oracle's)
    for conn, simplify, (r, lay) in got:
        assert lay == 0 if mode == "fused0" else (lay == 1 or H * W <= 81), (shape, mode, lay)
        for e, s in enumerate(sc):
            _same(r, e, _want(sets[e], conn, simplify), (shape, mode, s["name"], conn, simplify))
    for e in range(E):
        _same(deflt, e, _want(sets[e], 8), (shape, mode, "default connectivity"))
    r = got[0][2][0]
    assert set(cheap) == {"edges", "cells", "front"} and set(only_front) == {"front"}
    for name in ("edges", "cells", "front"):
        assert (cheap[name].cpu().numpy() == r[name]).all(), (shape, mode, name)
    assert (only_front["front"].cpu().numpy() == r["front"]).all()


@pytest.mark.parametrize("mode", ["fused0", "run"])
def test_serpentine_256(mode):
    """One loop of about 3 x 10^4 edges, found in 16 doubling rounds; beside it the serpentine of single rows and the spiral, twice as long."""
    H = W = 256
    masks = [pw.serpentine(H, W, 2), pw.serpentine(H, W), pw.spiral(H, W)]
    b = _loaded(H, W, masks, mode)
    for conn in (4, 8):
        wants = [_want(m, conn) for m in masks]
        assert [w["loops"] for w in wants] == [1, 1, 1] and 30000 < wants[0]["edges"] < 35000 and 2 ** 16 < wants[1]["edges"] <= 2 ** 17
        r, lay = _ask(b, connectivity=conn, **_caps(wants))
        sets = _sets(b.fire_maps())
        for e in range(3):
            assert (sets[e] == masks[e]).all()
            _same(r, e, wants[e], (mode, conn, e))
    assert lay == (1 if mode == "run" else 0)


def test_checkerboard_64():
    """2048 loops of four edges under 4-connectivity; one component full of holes under 8-connectivity."""
    H = W = 64
    m = pw.checkerboard(H, W)
    b = _loaded(H, W, [m], "fused0")
    w4, w8 = _want(m, 4), _want(m, 8)
    assert (w4["loops"], w4["holes"]) == (2048, 0) and w8["loops"] - w8["holes"] == 1 and w8["holes"] > 1900
    for conn, w in ((4, w4), (8, w8)):
        r, _ = _ask(b, connectivity=conn, **_caps([w]))
        _same(r, 0, w, ("checkerboard", conn))


# ---------------------------------------------------------------------------------------------- 2. the other two sources
@pytest.mark.parametrize("shape", [(16, 64), (17, 65)], ids=["16x64", "17x65"])
def test_member_planes(shape):
    """``member`` shared and per environment (values 0, 1, 255), aligned rows and rows that are not; the status bytes do not matter."""
    H, W = shape
    E = 4
    b = _loaded(H, W, [pw.random_mask(7, H, W, 0.5)] * E, "run")
    per = pw.per_env_member(E, H, W)
    envs = [2, 0, 3, 1, 2]
    for conn in (4, 8):
        wants = [_want(per[e] != 0, conn) for e in envs]
        r, _ = _ask(b, member=_dev(per), envs=envs, connectivity=conn, **_caps(wants))
        for i in range(len(envs)):
            _same(r, i, wants[i], (shape, "per env", conn, i))
        shared = per[1]
        w = _want(shared != 0, conn)
        r, _ = _ask(b, member=_dev(shared), connectivity=conn, **_caps([w]))
        for i in range(E):
            _same(r, i, w, (shape, "shared", conn, i))
    cheap = b.perimeter(member=_dev(per), front=True)
    for e in range(E):
        w = _want(per[e] != 0, 4)
        assert (int(cheap["edges"][e]), int(cheap["cells"][e])) == (w["edges"], w["cells"]) and (cheap["front"][e].cpu().numpy() == w["front"]).all()


@pytest.mark.parametrize("mode", ["fused0", "run"])
def test_at_update_on_a_real_rollout(mode):
    """40 x 72, arrival recording on, 12 updates: the sets of the horizons 0, 5 and 12 against the oracle on ``arrival()``; with no
    lines drawn, horizon 12 is the BURNING | BURNED answer."""
    H, W, E = 40, 72, 3
    rng = np.random.default_rng(2760)
    R8 = rng.choice([12.0, 20.0, 30.0], size=(8, H, W))
    R8[:, rng.random((H, W)) < 0.1] = 0.0
    b = _engine(H, W, E, mode, R8=R8)
    b.reset(np.array([[10, 10], [60, 30], [36, 20]], dtype=np.int32))
    b.enable_arrival(True)
    b.step(12)
    answers = {}
    arr = [b.arrival(e) for e in range(E)]
    for h in (0, 5, 12):
        wants = [_want(po.mask_of_arrival(a, h), 8) for a in arr]
        r, lay = _ask(b, at_update=h, **_caps(wants))
        for e in range(E):
            _same(r, e, wants[e], (mode, h, e))
        answers[h] = r
    assert [int(answers[0]["cells"][e]) for e in range(E)] == [1] * E
    assert all(int(answers[12]["cells"][e]) > int(answers[5]["cells"][e]) > 1 for e in range(E))
    sets = _sets(b.fire_maps())
    assert all((sets[e] == po.mask_of_arrival(arr[e], 12)).all() for e in range(E))
    wants = [_want(s, 8) for s in sets]
    r, _ = _ask(b, **_caps(wants))
    for e in range(E):
        _same(r, e, wants[e], (mode, "status", e))
        for name in ("edges", "cells", "loops", "holes", "n_vertices"):
            assert int(r[name][e]) == int(answers[12][name][e])
    assert lay == (1 if mode == "run" else 0)
    b.enable_arrival(False)
    with pytest.raises(ValueError, match="arrival"):
        b.perimeter(at_update=3)


# ---------------------------------------------------------------------------------------------- 3. lists, chunks, overflow
def test_lists_and_chunks():
    """A list with a repeat and a permutation; under a budget of one environment's scratch the list is worked through one by one,
    under two and a bit two by two - bit for bit the default call; the scratch grows and never shrinks; the summary form uses none."""
    import torch
    H, W = 33, 130
    sc = pw.scenes(H, W)
    b = _loaded(H, W, [s["mask"] for s in sc], "run")
    E = len(sc)
    envs = [E - 1, 3, 0, 3, 7, 5, 3, E - 2, 1]
    wants = [_want(sc[e]["mask"], 4) for e in envs]
    caps = _caps(wants)
    from simfire_amd import perimeter
    need = b.perimeter_scratch_bytes(caps["max_edges"])
    assert need == perimeter.scratch_need(H, W, caps["max_edges"]) == (8 * H * 3 + 12 * (H + 1) * 9 + 32 * caps["max_edges"] + 255) // 256 * 256
    mem0 = b.memory_bytes()
    b.perimeter(front=True)
    assert b.memory_bytes() == mem0                            # the summary form: no scratch
    one = b.perimeter(envs=envs, trace=True, connectivity=4, scratch_bytes=need, **caps)
    assert b.memory_bytes() - mem0 == need
    two = b.perimeter(envs=envs, trace=True, connectivity=4, scratch_bytes=2 * need + 7, **caps)
    assert b.memory_bytes() - mem0 == 2 * need
    full, _ = _ask(b, envs=envs, connectivity=4, **caps)
    assert b.memory_bytes() - mem0 == len(envs) * need
    b.perimeter(envs=[0], trace=True, scratch_bytes=need, **caps)
    assert b.memory_bytes() - mem0 == len(envs) * need
    for i in range(len(envs)):
        _same(full, i, wants[i], ("list", i))
    for got in (one, two):
        for name in got:
            x = got[name].cpu().numpy()
            if name in LISTS:                                  # (entries beyond an answer's are never written)
                for i, w in enumerate(wants):
                    k = {"vertices": w["n_vertices"], "loop_start": w["loops"] + 1}.get(name, w["loops"])
                    assert (x[i][:k] == full[name][i][:k]).all(), (name, i)
            else:
                assert (x == full[name]).all(), name
    with pytest.raises(ValueError, match="scratch_bytes"):
        b.perimeter(trace=True, scratch_bytes=need - 1, **caps)
    r = b.perimeter(envs=[], trace=True, front=True)
    assert r["edges"].shape == (0,) and r["front"].shape == (0, H, W) and torch.is_tensor(r["vertices"])


def _raw(eng, n, envs, outs, **fields):
    """The raw call with the caller's own output tensors -> the return code."""
    from simfire_amd import _lib
    p = _lib.SfPerimeterParams(**dict(dict(at_update=-1), **fields))
    o = _lib.SfPerimeterOut(**{k: (v if isinstance(v, int) else v.data_ptr()) for k, v in outs.items()})
    e = None if envs is None else np.ascontiguousarray(envs, dtype=np.int32)
    return eng._L.sf_perimeter(eng._h, C.byref(p), n, None if e is None else e.ctypes.data_as(C.c_void_p), C.byref(o))


@pytest.mark.parametrize("mode", ["fused0", "run"])
def test_overflow_is_per_environment(mode):
    """One call: environments over ``max_edges``, over ``max_vertices`` only, over ``max_loops`` only, and ones that fit.  The outputs
    are filled with a sentinel first: untouched means untouched, the counts are what the header states, ``edges``, ``cells`` and
    ``front`` are always right."""
    import torch
    from simfire_amd import _lib
    H, W = 17, 65
    sc = {s["name"]: s["mask"] for s in pw.scenes(H, W)}
    names = ["corner_cell", "checkerboard", "spiral", "random_0", "one_cell_hole", "nested_rings", "empty", "run_to_word_boundary", "four_borders"]
    b = _loaded(H, W, [sc[k] for k in names], mode)
    E = len(names)
    wants = [_want(sc[k], 4) for k in names]
    ME, MV, ML = 1188, 30, 5

    def kind_of(w):
        if w["edges"] > ME:
            return "edges"
        over = (["vertices"] if w["n_vertices"] > MV else []) + (["loops"] if w["loops"] > ML else [])
        return "+".join(over) if over else "fits"
    kinds = [kind_of(w) for w in wants]
    assert kinds == ["fits", "edges", "vertices", "vertices+loops", "fits", "vertices+loops", "fits", "loops", "fits"], \
        [(w["edges"], w["n_vertices"], w["loops"]) for w in wants]
    assert wants[2]["edges"] == ME                             # (exactly at the capacity: fits)
    S = -77
    out = dict(edges=torch.full((E,), S, dtype=torch.int32, device="cuda"), cells=torch.full((E,), S, dtype=torch.int32, device="cuda"),
               front=torch.full((E, H, W), 9, dtype=torch.uint8, device="cuda"), loops=torch.full((E,), S, dtype=torch.int32, device="cuda"),
               holes=torch.full((E,), S, dtype=torch.int32, device="cuda"), n_vertices=torch.full((E,), S, dtype=torch.int32, device="cuda"),
               vertices=torch.full((E, MV, 2), S, dtype=torch.int32, device="cuda"), loop_start=torch.full((E, ML + 1), S, dtype=torch.int32, device="cuda"),
               loop_area=torch.full((E, ML), S, dtype=torch.int32, device="cuda"), loop_edges=torch.full((E, ML), S, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    assert _raw(b, E, np.arange(E), out, status_mask=6, connectivity=4, simplify=1, max_edges=ME, max_vertices=MV, max_loops=ML) == _lib.SF_OK
    b.sync()
    r = {k: v.cpu().numpy() for k, v in out.items()}
    assert (_sets(b.fire_maps())[1] == sc["checkerboard"]).all()
    for e, (w, kind) in enumerate(zip(wants, kinds)):
        assert (int(r["edges"][e]), int(r["cells"][e])) == (w["edges"], w["cells"]) and (r["front"][e] == w["front"]).all(), (e, kind)
        if kind == "edges":
            assert (int(r["loops"][e]), int(r["holes"][e]), int(r["n_vertices"][e])) == (-1, -1, -1)
        else:
            assert (int(r["loops"][e]), int(r["holes"][e]), int(r["n_vertices"][e])) == (w["loops"], w["holes"], w["n_vertices"]), (e, kind)
        if kind == "fits":
            _same(r, e, w, ("overflow", mode, e))
            nl, nv = w["loops"], w["n_vertices"]
            assert (r["vertices"][e][nv:] == S).all() and (r["loop_start"][e][nl + 1:] == S).all() and (r["loop_area"][e][nl:] == S).all() \
                and (r["loop_edges"][e][nl:] == S).all()
        else:
            for name in LISTS:
                assert (r[name][e] == S).all(), (e, kind, name)


# ---------------------------------------------------------------------------------------------- 4. async
def test_async_mode():
    """In async mode the calls only enqueue: steps and perimeter calls queued behind each other, one wait, the results those of the
    same calls made one by one."""
    kw, R8, E, inits = aw.make_world("24x40")
    from simfire_amd.engine import FireEngine
    hs = []
    for _ in range(2):
        h = FireEngine(n_envs=E, **kw)
        m = aw.mode_settings("run")
        h.set_fused(m["fused"])
        if m.get("tuning"):
            h.set_tuning(**m["tuning"])
        h.set_rtable(R8)
        hs.append(h)
    a, b = hs
    b.set_async(True)
    got = {id(a): [], id(b): []}
    for h in (a, b):
        h.reset(inits)
        for n in (3, 4):
            h.step(n)
            got[id(h)].append(h.perimeter(front=True, trace=True))
            got[id(h)].append(h.perimeter(status=("BURNING",), connectivity=4))
    b.sync()
    for x, y in zip(got[id(a)], got[id(b)]):
        for name in ("edges", "cells", "front", "loops", "holes", "n_vertices"):
            if name in x:
                assert (x[name].cpu().numpy() == y[name].cpu().numpy()).all(), name
    r = {k: v.cpu().numpy() for k, v in got[id(b)][2].items()}
    conn = 8 if b.params.diagonal_spread else 4
    for e, s in enumerate(_sets(b.fire_maps())):
        _same(r, e, _want(s, conn), ("async", e))
    assert int(r["cells"].min()) > 1


# ---------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_in_the_frames_order():
    """Every refusal through the raw call: SF_EINVAL before the environment list's range, that before SF_ENOTSUP, that before
    SF_ESTATE; a refused call enqueues nothing and changes no layout; the call after the refusals answers like the oracle."""
    import torch
    from simfire_amd import _lib
    from simfire_amd.engine import FireEngine
    H, W, E = 17, 65, 3
    masks = [pw.random_mask(3, H, W, 0.4), pw.nested_rings(H, W), pw.spiral(H, W)]
    b = _engine(H, W, E, "run")
    S = -7
    i32 = torch.full((E,), S, dtype=torch.int32, device="cuda")
    verts = torch.full((E, 64, 2), S, dtype=torch.int32, device="cuda")
    starts = torch.full((E, 17), S, dtype=torch.int32, device="cuda")
    front = torch.full((E, H, W), 9, dtype=torch.uint8, device="cuda")
    mem = torch.ones((H, W), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    all_envs = np.arange(E)
    good = dict(status_mask=6, max_edges=4096, max_vertices=64, max_loops=16)

    def rc(n=E, envs=all_envs, outs=None, reserved=(0, 0), **fields):
        from simfire_amd import _lib as L
        p = L.SfPerimeterParams(**dict(dict(at_update=-1), **dict(good, **fields)))
        p.reserved[0], p.reserved[1] = reserved
        o = L.SfPerimeterOut(**(dict(edges=i32.data_ptr()) if outs is None else outs))
        e = None if envs is None else np.ascontiguousarray(envs, dtype=np.int32)
        return b._L.sf_perimeter(b._h, C.byref(p), n, None if e is None else e.ctypes.data_as(C.c_void_p), C.byref(o))

    assert b._L.sf_perimeter(None, None, 0, None, None) == _lib.SF_EINVAL
    assert rc() == _lib.SF_ESTATE and b"sf_reset" in b._L.sf_last_error()          # before the reset
    assert rc(at_update=3, status_mask=0) == _lib.SF_ESTATE                         # (the reset comes first)
    assert rc(connectivity=5, envs=[E], n=1) == _lib.SF_EINVAL and b"connectivity" in b._L.sf_last_error()      # argument before list
    b.reset(np.zeros((E, 2), dtype=np.int32))
    for e, m in enumerate(masks):
        b.load_fire_map(e, pw.fire_map(m))
    b.step(1)
    lay, kind = b.cell_layout(), b.last_launch_kind()
    traced = dict(loops=i32.data_ptr())
    need = b.perimeter_scratch_bytes(4096)
    bad = [dict(status_mask=0), dict(status_mask=-1), dict(status_mask=64), dict(status_mask=6, member=mem.data_ptr()), dict(status_mask=6, at_update=2),
           dict(status_mask=0, member=mem.data_ptr(), at_update=0), dict(at_update=-2), dict(connectivity=6), dict(connectivity=-1), dict(connectivity=1),
           dict(max_edges=-1), dict(max_vertices=-1), dict(max_loops=-1), dict(max_vertices=0, outs=dict(vertices=verts.data_ptr())),
           dict(max_loops=0, outs=dict(loop_start=starts.data_ptr())), dict(max_loops=0, outs=dict(loop_area=starts.data_ptr())),
           dict(max_loops=0, outs=dict(loop_edges=starts.data_ptr())), dict(outs=dict()), dict(outs=dict(edges=i32.data_ptr() + 2)),
           dict(outs=dict(cells=i32.data_ptr() + 1)), dict(outs=dict(vertices=verts.data_ptr() + 2)), dict(outs=dict(loop_start=starts.data_ptr() + 3)),
           dict(outs=traced, scratch_bytes=need - 1), dict(outs=traced, scratch_bytes=1), dict(scratch_bytes=-1), dict(reserved=(1, 0)), dict(reserved=(0, 1)),
           dict(envs=[0, E]), dict(envs=[-1, 0]), dict(n=-1), dict(envs=None)]
    for kwargs in bad:
        kwargs = dict(kwargs)
        if kwargs.get("envs") is not None and "n" not in kwargs:
            kwargs["n"] = len(kwargs["envs"])
        assert rc(**kwargs) == _lib.SF_EINVAL, kwargs
        assert b"sf_perimeter" in b._L.sf_last_error(), kwargs
    # which refusal wins: an argument before the list's range, the range before the state
    assert rc(reserved=(1, 0), envs=[E], n=1) == _lib.SF_EINVAL and b"reserved" in b._L.sf_last_error()
    assert rc(at_update=0, status_mask=0, envs=[E], n=1) == _lib.SF_EINVAL and b"out of range" in b._L.sf_last_error()
    assert rc(at_update=0, status_mask=0) == _lib.SF_ESTATE and b"sf_enable_arrival" in b._L.sf_last_error()
    b.sync()
    assert (i32 == S).all() and (verts == S).all() and (starts == S).all() and (front == 9).all()      # nothing was enqueued
    assert (b.cell_layout(), b.last_launch_kind()) == (lay, kind)
    wide = FireEngine(n_envs=1, **pw.engine_kwargs(2, 8200))
    wide.set_rtable(pw.slow_table(2, 8200))
    wide.reset(np.zeros((1, 2), dtype=np.int32))
    p = _lib.SfPerimeterParams(status_mask=6, at_update=-1)
    o = _lib.SfPerimeterOut(edges=i32.data_ptr())
    one = np.zeros(1, dtype=np.int32)
    assert wide._L.sf_perimeter(wide._h, C.byref(p), 1, one.ctypes.data_as(C.c_void_p), C.byref(o)) == _lib.SF_ENOTSUP
    one[0] = 1                                               # the list's range before the width
    assert wide._L.sf_perimeter(wide._h, C.byref(p), 1, one.ctypes.data_as(C.c_void_p), C.byref(o)) == _lib.SF_EINVAL
    wide.sync()
    assert (i32 == S).all()
    assert rc(n=0) == _lib.SF_OK                              # a list of none
    b.sync()
    assert (i32 == S).all()
    assert rc(outs=dict(edges=i32.data_ptr(), front=front.data_ptr())) == _lib.SF_OK     # the call after the errors works
    b.sync()
    sets = _sets(b.fire_maps())
    assert i32.cpu().tolist() == [_want(s, 4)["edges"] for s in sets] and all((front[e].cpu().numpy() == _want(s, 4)["front"]).all() for e, s in enumerate(sets))
    wants = [_want(s, 8) for s in sets]
    r, _ = _ask(b, **_caps(wants))
    for e in range(E):
        _same(r, e, wants[e], ("after the refusals", e))
    for kwargs in (dict(member=mem.cpu().numpy()), dict(member=torch.ones((H, W + 1), dtype=torch.uint8, device="cuda")),
                   dict(member=torch.ones((H, W), dtype=torch.float32, device="cuda")), dict(member=mem, status=6)):
        with pytest.raises(ValueError, match="perimeter"):
            b.perimeter(**kwargs)


# ---------------------------------------------------------------------------------------------- 6. BatchedFireEnv and the simulation classes
def _config_24x40():
    import yaml
    from simfire_amd.config import Config
    y = yaml.safe_load(open(os.path.join(CFG, "functional_config.yml")))
    y["area"]["screen_size"] = [24, 40]
    y["terrain"]["topography"]["functional"]["function"] = "flat"
    y["simulation"]["headless"] = True
    return Config(config_dict=y)


def test_batched_fire_env_perimeter():
    """``info["fire_perimeter"]`` and ``info["fire_cells"]`` of three ticks against the oracle on the maps behind each tick; without
    the option ``info`` has the old keys only."""
    import torch
    import simfire_amd
    from simfire_amd.simulation import BatchedFireSimulation
    cfg = _config_24x40()
    H, W = cfg.area.screen_size
    E, K = 3, 2
    ign = np.array([(10, 10), (W - 5, 7), (3, H - 4)], dtype=np.int32)
    starts = np.array([(W - 1, 16), (20, 12)], dtype=np.int32)
    sim = BatchedFireSimulation(cfg, E, ignitions=ign)
    env = simfire_amd.BatchedFireEnv(sim, K, starts, n_updates=2, perimeter=dict(status=("BURNING", "BURNED")))
    plain = simfire_amd.BatchedFireEnv(BatchedFireSimulation(cfg, E, ignitions=ign), K, starts, n_updates=2)
    env.reset()
    plain.reset()
    rng = np.random.default_rng(2770)
    seen = []
    for t in range(3):
        actions = torch.from_numpy(rng.integers(0, 20, size=(E, K)).astype(np.int32)).cuda()
        obs, reward, done, info = env.step(actions)
        obs_p, reward_p, done_p, info_p = plain.step(actions)
        assert set(info) == set(info_p) | {"fire_perimeter", "fire_cells"} and torch.equal(obs, obs_p) and torch.equal(reward, reward_p)
        assert info["fire_perimeter"].is_cuda and info["fire_perimeter"].dtype == torch.int32 and info["fire_cells"].shape == (E,)
        sets = _sets(sim._engine.fire_maps())
        assert info["fire_perimeter"].cpu().tolist() == [po.cheap(s)[0] for s in sets], t
        assert info["fire_cells"].cpu().tolist() == [po.cheap(s)[1] for s in sets], t
        seen.append(int(info["fire_cells"].sum()))
    assert seen[2] > seen[0] > E
    for bad in (dict(radius=3), dict(status=("EMBERS",)), dict(status=0), "on"):
        with pytest.raises(ValueError, match="perimeter"):
            simfire_amd.BatchedFireEnv(sim, K, starts, perimeter=bad)
    r = sim.perimeter(envs=[1], trace=True, device=False)
    w = _want(_sets(sim._engine.fire_maps())[1], 8 if sim._engine.params.diagonal_spread else 4)
    assert (int(r["edges"][0]), int(r["loops"][0]), int(r["n_vertices"][0])) == (w["edges"], w["loops"], w["n_vertices"])


def test_fire_simulation_perimeter_after_a_host_edit():
    from simfire_amd.config import Config
    from simfire_amd.enums import BurnStatus
    from simfire_amd.simulation import FireSimulation
    sim = FireSimulation(Config(os.path.join(CFG, "test_config_flat_simple.yml")))
    sim.run(3)
    eng = sim._engine
    conn = 8 if eng.params.diagonal_spread else 4
    ps = float(eng.params.pixel_scale)

    def check(r, m, scale):
        w = _want(po.mask_of_status(m, 6), conn)
        assert (r["loops"], r["holes"]) == (w["loops"], w["holes"]) and len(r["rings"]) == w["loops"]
        assert r["length"] == (w["edges"] * scale if scale != 1 else w["edges"]) and r["area"] == (w["cells"] * scale * scale if scale != 1 else w["cells"])
        for l, (v, hole) in enumerate(r["rings"]):
            want = w["vertices"][w["loop_start"][l]:w["loop_start"][l + 1]]
            assert (v == want * scale).all() and hole == bool(w["loop_area"][l] < 0)
    r = sim.perimeter()
    check(r, np.asarray(sim.fire_map), 1)
    assert r["area"] > 1 and isinstance(r["length"], int)
    ys, xs = np.nonzero(np.asarray(sim.fire_map) == 1)
    sim.fire_map[ys.min(), xs[ys.argmin()]] = int(BurnStatus.UNBURNED)          # a host edit: a notch in the fire's edge
    sim.fire_map[0, 0] = int(BurnStatus.BURNED)                                # ... and a second loop far away
    r2 = sim.perimeter(unit="ft")
    check(r2, np.asarray(sim.fire_map), ps)
    assert r2["loops"] >= 2 and r2["area"] == (r["area"]) * ps * ps and r2["rings"][0][0].dtype == np.float64
    with pytest.raises(ValueError, match="unit"):
        sim.perimeter(unit="m")
