"""Distance fields without a device (``sf_distance``): the NumPy oracle against scipy and against itself without
its cuts, the cap and float identities, the ABI as the header and the binding state it, the Python argument errors, and - with
``_arrival_worlds.DenseStandIn`` in place of an engine - that the worlds of ``tests/test_distance_gpu.py`` show what its cases claim."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _arrival_worlds as aw
import _dist_oracle as do
import _dist_worlds as dw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_maps():
    rng = np.random.default_rng(2201)
    maps = []
    for H, W, p in ((24, 40, 0.01), (33, 17, 0.05), (7, 130, 0.004), (20, 20, 0.0), (5, 9, 0.5), (40, 33, 0.9), (1, 50, 0.1), (50, 1, 0.1)):
        m = np.where(rng.random((H, W)) < p, rng.integers(1, 6, size=(H, W)), 0).astype(np.uint8)
        maps.append(m)
    blob = np.zeros((31, 37), dtype=np.uint8)                  # a filled disc with a burning rim: inner cells are cut from the candidates
    y, x = np.mgrid[0:31, 0:37]
    r2 = (y - 14) ** 2 + (x - 20) ** 2
    blob[r2 <= 64] = 2
    blob[(r2 <= 64) & (r2 > 36)] = 1
    maps.append(blob)
    return maps


# ---------------------------------------------------------------------------------------------- 1. the oracle
def test_oracle_equals_scipy_edt_squared():
    ndi = pytest.importorskip("scipy.ndimage")
    checked = 0
    for m in _random_maps():
        for mask in (2, 6, 1, 56, 63, 2 | 8):
            src = do.selected(m, mask)
            got = do.dist2(m, mask)
            if not src.any():
                assert (got == do.FAR).all()
                continue
            want = np.rint(ndi.distance_transform_edt(~src) ** 2).astype(np.int64)
            assert (got == want).all(), (m.shape, mask)
            checked += 1
    assert checked >= 30


def test_oracle_cuts_change_nothing():
    for m in _random_maps():
        for mask in (2, 6, 1, 56, 63):
            assert (do.dist2(m, mask) == do.dist2_all_candidates(m, mask)).all(), (m.shape, mask)


def test_oracle_by_hand():
    m = np.array([[0, 0, 0, 0],
                  [0, 1, 0, 0],
                  [0, 0, 0, 3]], dtype=np.uint8)
    assert do.dist2(m, 2).tolist() == [[2, 1, 2, 5], [1, 0, 1, 4], [2, 1, 2, 5]]
    assert do.dist2(m, 2 | 8).tolist() == [[2, 1, 2, 4], [1, 0, 1, 1], [2, 1, 1, 0]]
    assert do.dist2(m, 2, max_d2=2).tolist() == [[2, 1, 2, 2], [1, 0, 1, 2], [2, 1, 2, 2]]
    assert (do.dist2(m, 4) == do.FAR).all() and (do.dist2(m, 4, max_d2=9) == 9).all()
    assert (do.dist2(m | 0xF8, 2) == do.dist2(m, 2)).all()             # only status & 7 counts
    pts = np.array([[1, 1, 1], [3, 0, 2], [3, 0, 0], [4, 0, 1], [0, 3, 1], [-1, 0, 1], [3, 0, -5], [3, 0, 2]])
    assert do.at_points(do.dist2(m, 2), pts).tolist() == [0, 5, -1, -1, -1, -1, -1, 5]
    assert do.points_as_float(np.array([0, 5, -1]), 1.0).tolist() == [0.0, np.float32(np.sqrt(5.0)), -1.0]


def test_cap_identity_and_empty_set():
    for m in _random_maps():
        for mask in (2, 6, 1, 56):
            full = do.dist2(m, mask)
            for cap in (1, 2, 25, 1000):
                assert (do.dist2(m, mask, cap) == np.minimum(full, cap)).all()
    empty = np.zeros((20, 20), dtype=np.uint8)
    assert (do.dist2(empty, 2) == do.FAR).all() and do.dist2(empty, 2).dtype == np.int32
    assert (do.dist2(empty, 2, 9) == 9).all()
    assert (do.dist2(empty, 1) == 0).all() and (do.dist2(empty, 63) == 0).all()


def test_float_formula():
    v = np.array([0, 1, 2, 3, 5, 25, 1000, 123457, 2 ** 31 - 2, do.FAR], dtype=np.int32)
    for scale in (1.0, 7.0, 0.3):
        got = do.as_float(v, scale)
        assert got.dtype == np.float32
        for a, b in zip(v.tolist(), got):
            assert np.float32(np.sqrt(np.float64(a)) / np.float64(scale)) == b       # one double sqrt, one double divide, one rounding
    import math
    assert do.as_float(np.array([do.FAR]), 1.0)[0] == np.float32(math.sqrt(2147483647.0))
    assert do.as_float(np.array([49]), 7.0)[0] == np.float32(1.0) and do.as_float(np.array([2]), 1.0)[0] == np.float32(math.sqrt(2.0))


# ---------------------------------------------------------------------------------------------- 2. the ABI
def test_header_declares_and_lib_binds_distance():
    from simfire_amd import _lib
    text = open(os.path.join(ROOT, "include", "simfire_hip.h")).read()
    assert re.search(r"int\s+sf_distance\s*\(\s*sf_sim\s*\*\s*sim\s*,\s*const\s+sf_dist_params\s*\*\s*params\s*,\s*int32_t\s+n\s*,\s*"
                     r"const\s+int32_t\s*\*\s*envs[^,)]*,\s*void\s*\*\s*device_out\s*\)\s*;", text)
    for name, val in (("SF_DIST_FAR", "2147483647"), ("SF_DIST_I32", "0"), ("SF_DIST_F32", "1"), ("SF_DIST_MAX_POINTS", "256")):
        assert re.search(r"#define\s+%s\s+%s\b" % (name, val), text), name
    assert re.search(r"typedef\s+struct\s+sf_dist_params\s*\{[^}]*int32_t\s+status_mask\s*;[^}]*int32_t\s+max_d2\s*;[^}]*int32_t\s+dtype\s*;"
                     r"[^}]*int32_t\s+k\s*;[^}]*double\s+scale\s*;[^}]*const\s+int32_t\s*\*\s*points\s*;[^}]*int64_t\s+scratch_bytes\s*;"
                     r"[^}]*int32_t\s+reserved\s*\[\s*2\s*\]\s*;[^}]*\}\s*sf_dist_params\s*;", text)
    assert text.index("int sf_observe(") < text.index("sf_distance(") < text.index("Agents on the device")      # next to sf_observe
    assert "no counterpart" in text[text.index("Distance fields"):text.index("#define SF_DIST_FAR")]
    assert "hipMalloc" in text[text.index("typedef struct sf_dist_params"):text.index("int sf_distance(")]
    # the layout the header's declaration has under the C ABI of the host
    P = _lib.SfDistParams
    assert C.sizeof(P) == 48
    assert [(f[0], getattr(P, f[0]).offset) for f in P._fields_] == [("status_mask", 0), ("max_d2", 4), ("dtype", 8), ("k", 12), ("scale", 16),
                                                                    ("points", 24), ("scratch_bytes", 32), ("reserved", 40)]
    assert (_lib.SF_DIST_FAR, _lib.SF_DIST_I32, _lib.SF_DIST_F32, _lib.SF_DIST_MAX_POINTS) == (2 ** 31 - 1, 0, 1, 256)
    assert "sf_distance" in _lib.SIGNATURES and len(_lib.SIGNATURES["sf_distance"]) == 5
    csrc = os.path.join(ROOT, "simfire_amd", "csrc")
    assert open(os.path.join(csrc, "simfire_hip.hip")).read().count('#include "sf_dist_kernels.h"') == 1
    # the step kernels and the other features do not know the new kernels
    for unit in sorted(os.listdir(csrc)):
        if unit.endswith((".hip", ".h")) and unit not in ("simfire_hip.hip", "sf_host_query.h", "sf_dist_kernels.h"):
            assert "k_dist_" not in open(os.path.join(csrc, unit)).read(), unit


def test_built_library_exports_sf_distance():
    from simfire_amd import _lib
    L = _lib.load()                        # (raises if the library has not been built)
    assert L.sf_distance.argtypes == _lib.SIGNATURES["sf_distance"]
    p = _lib.SfDistParams(status_mask=2, scale=1.0)
    e = np.zeros(1, dtype=np.int32)
    assert L.sf_distance(None, C.byref(p), 1, e.ctypes.data_as(C.c_void_p), C.c_void_p(16)) == _lib.SF_EINVAL
    assert b"sf_distance" in L.sf_last_error()


# ------------------------------------------------------------------------- 3. errors before any library call
class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called: {name}")


def _bare_engine(E=4, H=24, W=40):
    from simfire_amd.engine import FireEngine
    eng = FireEngine.__new__(FireEngine)
    eng._L, eng._h = _NoDevice(), None
    eng.n_envs, eng.H, eng.W = E, H, W
    eng.async_mode, eng._blobs_in_flight = False, []
    return eng


@pytest.mark.parametrize("kw", [
    dict(status=0), dict(status=64), dict(status=-1), dict(status=()), dict(status=("SMOULDERING",)), dict(status=(6,)), dict(status=(-1,)),
    dict(status=(1.0,)), dict(status=None), dict(status=2.0), dict(status=True),
    dict(status=2, max_dist=0), dict(status=2, max_dist=-3), dict(status=2, max_dist=2.5), dict(status=2, max_dist=46341),
    dict(status=2, max_dist=3, max_d2=9), dict(status=2, max_d2=0), dict(status=2, max_d2=2 ** 31),
    dict(status=2, dtype="float64"), dict(status=2, dtype="bfloat16"), dict(status=2, dtype=None),
    dict(status=2, scale=0.0), dict(status=2, scale=-1.0), dict(status=2, scale=float("inf")), dict(status=2, scale=float("nan")),
    dict(status=2, scale="x"), dict(status=2, scratch_bytes=-1), dict(status=2, scratch_bytes=1.5),
    dict(status=2, envs=[4]), dict(status=2, envs=[-1]), dict(status=2, envs=[[0, 1]]), dict(status=2, envs=[0.0]),
])
def test_python_argument_errors(kw):
    eng = _bare_engine()
    with pytest.raises(ValueError, match="distance"):
        eng.distance(**kw)


def test_request_forms():
    from simfire_amd.engine import FireEngine
    from simfire_amd.enums import BurnStatus
    req = FireEngine._distance_request
    assert req(("BURNING",))[:3] == (2, 0, 1)
    assert req(BurnStatus.BURNED, dtype="int32")[:3] == (4, 0, 0)
    assert req([BurnStatus.FIRELINE, "SCRATCHLINE", 5], max_dist=16)[:2] == (56, 256)
    assert req(63, max_d2=1000, scale=7)[:4] == (63, 1000, 1, 7.0)
    assert req("UNBURNED", scratch_bytes=4096)[4] == 4096
    assert req(np.int64(6), dtype=np.dtype("int32"))[:3] == (6, 0, 0)
    for names in dw.MASKS:
        assert req(names)[0] == do.mask_of(names)
    assert req(dw.MASKS[-1])[0] == 63


# ------------------------------------------------------------------- 4. the worlds of the GPU test see what it claims
def _stand_in(case):
    kw, R8, E, inits = aw.make_world(case)
    return aw.DenseStandIn(kw, R8, E), E, inits, kw["shape"]


def test_episode_worlds_see_what_they_claim():
    """Over the episodes of test 1 of the GPU file: every mask and every cap at some query point of every (case, mode) pair; BURNING
    fires that grow; a value of exactly 2, a value above the cap, a column with no source, the empty set (no control lines in these
    worlds) and the mask of all six."""
    for case in dw.EPISODE_CASES:
        h, E, inits, (H, W) = _stand_in(case)
        for mode in aw.CASES[case]["modes"]:
            qs = dw.queries(case, mode)
            assert {q[1] for q in qs} == set(dw.MASKS) and {q[2] for q in qs} == set(dw.CAPS), (case, mode)
        mode = aw.CASES[case]["modes"][0]
        words, burning = set(), []

        def on_query(i, n, names, cap):
            for e in range(E):
                m = h.fire_map(e)
                words.update(dw.seen(m, names, cap))
                if e == 0:
                    burning.append(int((m == 1).sum() + (m == 2).sum()))
        dw.run_episode(case, mode, h, inits, on_query)
        assert {"value of exactly 2", "value above the cap", "column with no source", "empty set", "all selected"} <= words, (case, words)
        assert burning[-1] > burning[0] >= 1 and burning[-1] >= 20, (case, burning)


def test_edge_worlds_see_what_they_claim():
    """Test 2 of the GPU file: fire lines on the four borders and corners, the lone BURNING corner, the mask that selects nothing."""
    for case in dw.EDGE_CASES:
        h, E, inits, (H, W) = _stand_in(case)
        assert E >= 3
        dw.edge_scene(h, E, H, W, inits)
        words = set()
        for e in range(E):
            m = h.fire_map(e)
            assert (m == dw.FIRELINE).sum() >= 4
            words |= dw.seen(m, ("FIRELINE",), 9)
            assert "all selected" not in dw.seen(m, ("UNBURNED",), 0)
            d = do.dist2(m, do.mask_of(("UNBURNED",)))
            assert d.max() >= 1 and (d[m == 0] == 0).all()
        assert {"source on row 0", "source on row H-1", "source in column 0", "source in column W-1", "value above the cap",
                "column with no source", "value of exactly 2"} <= words, (case, words)
        assert dw.seen(h.fire_map(0), ("SCRATCHLINE", "WETLINE"), 9) == {"empty set"}
        lone = dw.lone_corner_map(H, W)
        d = do.dist2(lone, 2)
        assert d[H - 1, W - 1] == 0 and d[0, 0] == (H - 1) ** 2 + (W - 1) ** 2 and dw.seen(lone, ("BURNING",), 0) >= {
            "source on row H-1", "source in column W-1", "column with no source", "value of exactly 2"}
    assert dw.CLAIMS <= words | {"empty set"}
