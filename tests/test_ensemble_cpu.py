"""Ensemble statistics without a GPU: the oracle by hand, the inputs of every case of ``tests/test_ensemble_gpu.py`` (run on
``oracle/fire_dense``), the declared ABI, the argument errors the Python layer raises before any library call, and the NULL-handle
refusal of the built library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _ensemble_oracle as eo
import _ensemble_worlds as ew
from test_values_cpu import _NoDevice, _bare_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------ 1. the oracle, by hand
def test_oracle_by_hand():
    # three environments on a 2 x 3 grid; cell (1, 2) is reached by nobody
    arrival = np.array([[[0, 1, 4], [-1, 2, -1]],
                        [[3, 0, -1], [-1, 7, -1]],
                        [[-1, -1, -1], [5, 1, -1]]], dtype=np.int32)
    values = np.array([[10, -3, 100], [7, 1000, 5]], dtype=np.int32)
    members = [[0, 1, 1], [2, 0, 2]]                          # a duplicate inside each group, environment 0 in both
    s = eo.stats(arrival, members, (0, 3, -1), values)
    assert s["count"].dtype == np.int32 and s["count"].shape == (2, 3, 2, 3)
    assert s["count"][0].tolist() == [[[1, 2, 0], [0, 0, 0]], [[3, 3, 0], [0, 1, 0]], [[3, 3, 1], [0, 3, 0]]]
    assert s["count"][1].tolist() == [[[1, 0, 0], [0, 0, 0]], [[1, 1, 0], [0, 3, 0]], [[1, 1, 1], [2, 3, 0]]]
    assert s["prob"].dtype == np.float32
    assert s["prob"][0, 0, 0, 0] == np.float32(1) / np.float32(3) and s["prob"][0, 0, 0, 1] == np.float32(2) / np.float32(3)
    assert s["prob"][0, 0, 0, 0].tobytes() == np.float32(0.33333334).tobytes() and s["prob"][0, 2, 0, 0] == np.float32(1.0)
    assert s["first"].tolist() == [[[0, 0, 4], [-1, 2, -1]], [[0, 1, 4], [5, 1, -1]]]
    assert s["mean"].dtype == np.float32
    assert s["mean"][0].tolist() == [[2.0, np.float32(1 / 3), 4.0], [-1.0, np.float32(16 / 3), -1.0]]
    assert s["mean"][1].tolist() == [[0.0, 1.0, 4.0], [5.0, np.float32(4 / 3), -1.0]]
    # loss: per member the values of the cells IT reached, duplicates counted again
    assert s["loss"].dtype == np.int64
    assert s["loss"].tolist() == [[10 - 6, 30 - 9 + 1000, 30 - 9 + 100 + 3000], [10, 10 - 3 + 3000, 10 - 3 + 100 + 14 + 3000]]
    # the first / mean take the members that arrived by the LAST horizon only
    t = eo.stats(arrival, members, (0, 3))
    assert "loss" not in t and t["first"].tolist() == [[[0, 0, -1], [-1, 2, -1]], [[0, 1, -1], [-1, 1, -1]]]
    assert t["mean"][0].tolist() == [[2.0, np.float32(1 / 3), -1.0], [-1.0, 2.0, -1.0]]
    # K = 1: the member's own plane
    k1 = eo.stats(arrival, [[0], [1], [2]], (-1,), values)
    assert (k1["count"][:, 0] == (arrival >= 0)).all() and (k1["first"] == arrival).all()
    assert (k1["prob"] == (arrival >= 0).astype(np.float32)[:, None]).all()
    assert (k1["mean"] == arrival.astype(np.float32)).all()
    assert k1["loss"][:, 0].tolist() == [10 - 3 + 100 + 1000, 10 - 3 + 1000, 7 + 1000]
    # a plane per environment
    per_env = np.stack([values, 2 * values, -values])
    assert eo.stats(arrival, members, (-1,), per_env)["loss"].tolist() == [[1107 + 2 * 2 * 1007], [1107 - 2 * 1007]]
    # sums beyond int32 and float32's integers: update indices near 2^31, 3 of them
    far = np.full((3, 1, 1), 2 ** 31 - 2, dtype=np.int32)
    m = eo.stats(far, [[0, 1, 2]], (-1,))
    assert m["first"][0, 0, 0] == 2 ** 31 - 2 and m["mean"][0, 0, 0] == np.float32(2 ** 31 - 2)


# ------------------------------------------------------------------------------ 2. the inputs of the GPU cases
@pytest.mark.parametrize("case", list(ew.CASES))
def test_case_sees_what_it_claims(case):
    kw, R8, E, inits = ew.world(case)
    values = ew.make_values(case, E, inits)
    moments = ew.expected_arrivals(case)
    assert [u for u, _ in moments] == [1, 3, 6, 11, 18, 29]
    updates, arr = moments[-1]
    s = eo.stats(arr, ew.layouts(E)["all"], (0, ew.MID, updates, -1), values)
    distinct = [len(set(np.unique(s["count"][0, t]).tolist()) - {0}) for t in range(4)]
    assert max(distinct) >= 3, distinct                          # at one horizon: three distinct non-zero counts
    assert (s["first"][0] != arr[0]).any()                       # `first` is not member 0's plane
    assert (s["loss"] != 0).all() and len(set(s["loss"][0].tolist())) >= 2, s["loss"]
    p = s["prob"][0]
    assert ((p > 0) & (p < 1)).any()


def test_scripted_episodes_see_what_they_claim():
    arr = ew.recipe_expected()
    E = arr.shape[0]
    p = eo.stats(arr, ew.layouts(E)["all"], (6, -1))["prob"][0]
    assert ((p > 0) & (p < 1)).sum() >= 20 and len(np.unique(p)) >= 4           # the members' lines made their fires differ
    o = ew.OUT_OF_STEP
    (run0, upd0, _), (run1, upd1, arr1), (run2, upd2, arr2) = ew.out_of_step_expected()
    others = [e for e in range(E) if e not in o["reset"]]
    assert (upd0[list(o["reset"])] == 2).all() and (upd0[others] == 20).all() and (run0 == 1).all()
    assert run1[o["ringed"]] != 1 and upd2[o["ringed"]] == upd1[o["ringed"]] < upd1[o["reset"][0]] < upd2[o["reset"][0]]     # gone out: frozen
    assert (arr1[o["ringed"]] >= 0).sum() == 1 and (arr2[o["reset"][0]] >= 0).sum() > (arr1[o["reset"][0]] >= 0).sum()


def test_layouts_and_horizons():
    for E in (3, 4, 5, 7):
        lay = ew.layouts(E)
        assert lay["all"].shape == (1, E) and lay["g3k5"].shape == (3, 5) and lay["k1"].shape == (E, 1) and lay["k67"].shape == (1, 67)
        assert {lay[k].shape[1] for k in ("k3", "k6", "k7")} == {3, 6, 7}
        g = lay["g3k5"]
        assert len(set(g[0].tolist())) < 5 and set(g[0].tolist()) & set(g[1].tolist())        # a duplicate; an environment in two groups
        assert np.bincount(lay["k67"][0], minlength=E).max() > E // 2 and set(lay["k67"][0].tolist()) == set(range(E))
        for m in lay.values():
            assert m.dtype == np.int32 and m.min() >= 0 and m.max() < E
    seen = set()
    for moment in range(len(ew.CALLS)):
        for j in range(7):
            hz = ew.horizons_at(moment, j)
            seen.add((j, len(hz)))
            assert all(b > a for a, b in zip(hz, hz[1:]) if b != -1) and -1 not in hz[:-1]
    assert seen == {(j, T) for j in range(7) for T in (1, 3, 8)}
    flat = [h for v in ew.HORIZONS.values() for hz in v for h in hz]
    assert 0 in flat and ew.MID in flat and ew.BEYOND in flat and -1 in flat


# ---------------------------------------------------------------------------------------------- 3. the ABI
def test_header_declares_and_lib_binds_ensemble():
    from simfire_amd import _lib
    text = open(os.path.join(ROOT, "include", "simfire_hip.h")).read()
    assert re.search(r"int\s+sf_ensemble_stats\s*\(\s*sf_sim\s*\*\s*sim\s*,\s*const\s+sf_ensemble_params\s*\*\s*params\s*,\s*"
                     r"const\s+int32_t\s*\*\s*members[^,)]*,\s*const\s+sf_ensemble_out\s*\*\s*out\s*\)\s*;", text)
    assert re.search(r"#define\s+SF_ENS_MAX_HORIZONS\s+8\b", text)
    assert re.search(r"typedef\s+struct\s+sf_ensemble_params\s*\{[^}]*n_groups\s*,\s*group_size[^}]*n_horizons[^}]*"
                     r"horizons\s*\[\s*SF_ENS_MAX_HORIZONS\s*\][^}]*reserved[^}]*\}\s*sf_ensemble_params\s*;", text)
    assert re.search(r"typedef\s+struct\s+sf_ensemble_out\s*\{[^}]*int32_t\s*\*\s*count\s*;\s*float\s*\*\s*prob\s*;\s*int32_t\s*\*\s*first\s*;"
                     r"\s*float\s*\*\s*mean\s*;\s*int64_t\s*\*\s*loss\s*;[^}]*\}\s*sf_ensemble_out\s*;", text)
    assert text.index("Values at risk") < text.index("Ensemble statistics") < text.index("sf_ensemble_stats(")
    assert "sf_ensemble_stats" in _lib.SIGNATURES and len(_lib.SIGNATURES["sf_ensemble_stats"]) == 4
    assert C.sizeof(_lib.SfEnsembleParams) == 4 * (3 + 8 + 1) == 48 and _lib.SfEnsembleParams.horizons.offset == 12
    assert C.sizeof(_lib.SfEnsembleOut) == 5 * C.sizeof(C.c_void_p) == 40
    assert [f[0] for f in _lib.SfEnsembleOut._fields_] == ["count", "prob", "first", "mean", "loss"]
    csrc = os.path.join(ROOT, "simfire_amd", "csrc")
    # the host code of the main unit: simfire_hip.hip and the fragments it includes (sf_handle.h, sf_host_*.h)
    host = sorted(f for f in os.listdir(csrc) if f == "simfire_hip.hip" or f == "sf_handle.h" or f.startswith("sf_host_"))
    src = "".join(open(os.path.join(csrc, f)).read() for f in host)
    assert re.search(r'extern "C" int sf_ensemble_stats\(', src)
    # the kernel is the main unit's alone; the step path and the two passes do not know it
    for unit in sorted(os.listdir(csrc)):
        if unit.endswith((".hip", ".h")) and unit not in host and unit != "sf_ensemble_kernels.h":
            body = open(os.path.join(csrc, unit)).read()
            assert "sf_ensemble_kernels.h" not in body and "k_ensemble" not in body, unit
    assert src.count('#include "sf_ensemble_kernels.h"') == 1
    for name in ("static int enqueue_call(", "static int arrival_pass(sf_sim *s)\n{", "static int value_pass(sf_sim *s)\n{"):
        body = src[src.index(name):]
        body = body[:body.index("\n}\n")]
        assert "ensemble" not in body and "ens_blk" not in body, name
    kern = open(os.path.join(csrc, "sf_ensemble_kernels.h")).read()
    assert "asm" not in kern and "__shared__" not in kern


# ------------------------------------------------------------------------- 4. errors before any library call
def _engine(E=5):
    eng = _bare_engine(E=E)
    eng.arrival_on = True
    return eng


@pytest.mark.parametrize("kw", [
    dict(members=[0, 1, 2]),                                          # not 2-D
    dict(members=[[[0, 1]]]),
    dict(members=[[0.0, 1.0]]),                                       # not integers
    dict(members=[[0, 5]]),                                           # out of range
    dict(members=[[-1, 0]]),
    dict(members=np.zeros((2, 0), dtype=np.int32)),                   # K = 0
    dict(members=np.zeros((0, 3), dtype=np.int32)),                   # G = 0
    dict(members=np.zeros((1, 65536), dtype=np.int32)),               # K beyond 65535
    dict(members=np.zeros((1025, 1024), dtype=np.int32)),             # G * K beyond 2^20
    dict(members=[[0, 1]], horizons=tuple(range(9))),                 # T = 9
    dict(members=[[0, 1]], horizons=()),
    dict(members=[[0, 1]], horizons=(5, 3)),                          # descending
    dict(members=[[0, 1]], horizons=(3, 3)),
    dict(members=[[0, 1]], horizons=(-1, 4)),                         # -1 not last
    dict(members=[[0, 1]], horizons=(-2,)),
    dict(members=[[0, 1]], horizons=(1.5,)),
    dict(members=[[0, 1]], prob=False),                               # no output asked for
])
def test_python_argument_errors(kw):
    eng = _engine()
    with pytest.raises(ValueError, match="ensemble_stats"):
        eng.ensemble_stats(**kw)


@pytest.mark.parametrize("kw", [
    dict(members=None), dict(members=[[0, 4, 4]], horizons=(0, 7, -1), count=True, first=True, mean=True, loss=True),
    dict(members=np.zeros((1024, 1024), dtype=np.int64), horizons=(-1,)), dict(members=[[1]], horizons=tuple(range(8))),
])
def test_a_valid_call_reaches_the_library(kw):
    eng = _engine()
    assert isinstance(eng._L, _NoDevice)
    with pytest.raises(AssertionError, match="sf_ensemble_stats"):
        eng.ensemble_stats(**kw)


# ------------------------------------------------------------------------------ 5. NULL handle
def test_null_handle_refusal():
    from simfire_amd import _lib
    L = _lib.load()                        # (raises if the library has not been built)
    p = _lib.SfEnsembleParams(n_groups=1, group_size=1, n_horizons=1)
    p.horizons[0] = -1
    o = _lib.SfEnsembleOut(count=16)
    m = np.zeros(1, dtype=np.int32)
    assert L.sf_ensemble_stats(None, C.byref(p), m.ctypes.data_as(C.c_void_p), C.byref(o)) == _lib.SF_EINVAL
    assert b"sf_ensemble_stats" in L.sf_last_error()
