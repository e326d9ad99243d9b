"""Values at risk without a GPU: the inputs of every case of ``tests/test_values_gpu.py`` (run on ``oracle/fire_dense``), the declared
ABI, the argument errors the Python layer raises before any device call, and the NULL-handle refusals of the built library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _values_oracle as vo
from _values_worlds import CASES, VALUE_CASES, DenseStandIn, drive, make_values, make_world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("sf_values_set", "sf_values_get", "sf_values_device", "sf_values_set_weight")
LAB_ENTRIES = ("sf_set_values_dense", "sf_get_value_passes")


# ------------------------------------------------------------------------------ 1. the oracle, by hand
def test_oracle_by_hand():
    values = np.array([[5, -2, 0], [7, 1000, 3]], dtype=np.int32)
    arrival = np.array([[[0, -1, 2], [-1, 5, -1]], [[-1, -1, -1], [-1, -1, -1]], [[1, 1, 1], [1, 1, 1]]], dtype=np.int32)
    assert vo.damage(values, arrival).tolist() == [1005, 0, 1013]
    per_env = np.stack([values, values * 2, -values])
    assert vo.damage(per_env, arrival).tolist() == [1005, 0, -1013]
    assert vo.damage(values, arrival).dtype == np.int64
    big = np.full((1, 4096, 4096), vo.VALUE_MAX, dtype=np.int32)            # 2^24 cells of 2^24: beyond int32 and exact
    assert vo.damage(big[0], np.zeros_like(big)).tolist() == [1 << 48]
    assert vo.tick_loss([3, 4, 5], [10, 4, 2], [True, True, False]).tolist() == [7, 0, 0]
    # the branch: a sum of -0.0 keeps its sign while the weight is off, and loses it to "+ 0.0 * loss"
    z = vo.reward((-0.0, -0.0, -0.0, -0.0), (0, 0, 0, 0))
    assert z.tobytes() == np.float32(-0.0).tobytes()
    assert vo.reward((-0.0, -0.0, -0.0, -0.0), (0, 0, 0, 0), 0.0, 5).tobytes() == np.float32(0.0).tobytes()
    assert vo.reward((-1.0, 0.25, -10.0, -0.5), (3, 2, 1, 4), -0.001, 1500) == np.float32(-3.0 + 0.5 - 10.0 - 2.0 + float(np.float32(-0.001)) * 1500.0)


# ------------------------------------------------------------------------------ 2. the inputs of the GPU cases
_seen = {}


def _see(case):
    if case not in _seen:
        kw, R8, E, _ = make_world(case)
        _seen[case] = drive(case, CASES[case]["modes"][0], DenseStandIn(kw, R8, E))
    return _seen[case]


@pytest.mark.parametrize("case", list(VALUE_CASES))
def test_case_sees_what_it_claims(case):
    c = CASES[case]
    seen = _see(case)
    assert seen["rises"] >= 3, seen["total"]                     # the damage changes over several calls
    assert seen["ignition_value"] >= 1                           # an ignition cell inside a town: the reset's own contribution
    assert seen["negative_counted"] >= 1
    ops = c.get("ops", {})
    if any(op[0].startswith("reset") for op in ops.values()):
        assert seen["reset_after_damage"] >= 1
    if c.get("lines"):
        assert seen["line_on_burning_town"] >= 1
    if any(op[0] == "load" for op in ops.values()):
        assert [o for o in seen["ops"] if isinstance(o, tuple) and o[0] == "damage restored" and o[1] > 0], seen["ops"]
    if "values_at" in VALUE_CASES[case]:
        assert [o for o in seen["ops"] if isinstance(o, tuple) and o[0] == "values set at damage" and o[1] > 0], seen["ops"]


def test_value_planes():
    assert any(v.get("per_env") for v in VALUE_CASES.values())
    for case, v in VALUE_CASES.items():
        kw, R8, E, inits = make_world(case)
        p = make_values(case, E, inits)
        H, W = CASES[case]["H"], CASES[case]["W"]
        assert p.dtype == np.int32 and p.shape == ((E, H, W) if v.get("per_env") else (H, W))
        assert (p == 0).mean() > 0.5 and (p < 0).any() and p.max() <= 1000 and p.max() > 0
        assert not (make_values(case, E, inits, seed_offset=1) == p).all()


# ---------------------------------------------------------------------------------------------- 3. the ABI
def test_header_declares_and_lib_binds_values():
    from simfire_amd import _lib
    text = open(os.path.join(ROOT, "include", "simfire_hip.h")).read()
    lab = open(os.path.join(ROOT, "include", "simfire_hip_lab.h")).read()
    decl = {
        "sf_values_set": r"int\s+sf_values_set\s*\(\s*sf_sim\s*\*\s*sim\s*,\s*const\s+int32_t\s*\*\s*values\s*,\s*int32_t\s+per_env\s*,\s*int32_t\s+device_pointer\s*\)\s*;",
        "sf_values_get": r"int\s+sf_values_get\s*\(\s*sf_sim\s*\*\s*sim\s*,\s*int64_t\s*\*\s*damage_out[^)]*\)\s*;",
        "sf_values_device": r"int\s+sf_values_device\s*\(\s*sf_sim\s*\*\s*sim\s*,\s*void\s*\*\*\s*damage\s*,\s*int64_t\s*\*\s*damage_stride\s*,\s*void\s*\*\*\s*tick_loss\s*\)\s*;",
        "sf_values_set_weight": r"int\s+sf_values_set_weight\s*\(\s*sf_sim\s*\*\s*sim\s*,\s*float\s+w_value\s*,\s*int32_t\s+on\s*\)\s*;",
    }
    for name, pat in decl.items():
        assert re.search(pat, text), f"include/simfire_hip.h does not declare {name}"
    assert re.search(r"int\s+sf_set_values_dense\s*\(\s*sf_sim\s*\*\s*sim\s*,\s*int32_t\s+on\s*\)\s*;", lab)
    assert re.search(r"int\s+sf_get_value_passes\s*\(\s*sf_sim\s*\*\s*sim\s*,\s*int64_t\s*\*\s*out[^)]*\)\s*;", lab)
    for name, n in zip(ENTRIES + LAB_ENTRIES, (4, 2, 4, 3, 2, 2)):
        assert name in _lib.SIGNATURES, f"simfire_amd/_lib.py does not bind {name}"
        assert len(_lib.SIGNATURES[name]) == n, name
    # existing structs stay four wide
    assert re.search(r"float\s+w\[4\]", text) and "sf_values_set" in text[text.index("Values at risk"):]
    csrc = os.path.join(ROOT, "simfire_amd", "csrc")      # the host code of the main unit: simfire_hip.hip and the fragments it includes
    src = "".join(open(os.path.join(csrc, f)).read() for f in sorted(f for f in os.listdir(csrc) if f == "simfire_hip.hip" or f == "sf_handle.h" or f.startswith("sf_host_")))
    for name in ENTRIES + LAB_ENTRIES:
        assert re.search(r'extern "C" int %s\(' % name, src), name
    # the kernels are this unit's alone, and the pass hangs behind the arrival pass
    for unit in ("simfire_hip_run2.hip", "simfire_hip_run3.hip", "simfire_hip_run4.hip", "simfire_hip_cfd.hip", "sf_arrival_kernels.h", "sf_step_kernels.h"):
        assert "sf_value_kernels.h" not in open(os.path.join(ROOT, "simfire_amd", "csrc", unit)).read(), unit
    body = src[src.index("static int arrival_pass(sf_sim *s)\n{"):]
    assert "value_pass(s)" in body[:body.index("\n}\n")]


# ------------------------------------------------------------------------- 4. errors before any device call
class _NoDevice:
    """Stands where the library would: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was called: the argument error must come first")


def _bare_engine(E=3, H=6, W=7):
    from simfire_amd.engine import FireEngine
    from simfire_amd import _lib
    eng = FireEngine.__new__(FireEngine)
    eng._L, eng._h = _NoDevice(), None
    eng.H, eng.W, eng.n_envs = H, W, E
    eng.params = _lib.SfParams(n_envs=E, height=H, width=W, device=0)
    eng.values_on = eng.arrival_on = eng.async_mode = False
    eng.n_agents = 0
    return eng


@pytest.mark.parametrize("bad,kw", [
    (np.zeros((6, 8), dtype=np.int32), {}),                                  # wrong shape
    (np.zeros((2, 6, 7), dtype=np.int32), {}),                               # wrong number of environments
    (np.zeros((6, 7), dtype=np.int32), dict(per_env=True)),                  # a shared plane declared per environment
    (np.zeros((3, 6, 7), dtype=np.int32), dict(per_env=False)),
    (np.zeros((6, 7), dtype=np.float32), {}),                                # wrong dtype
    (np.full((6, 7), (1 << 24) + 1, dtype=np.int64), {}),                    # out of range
    (np.full((3, 6, 7), -(1 << 24) - 1, dtype=np.int64), {}),
])
def test_python_argument_errors(bad, kw):
    eng = _bare_engine()
    with pytest.raises(ValueError):
        eng.values_set(bad, **kw)
    assert not eng.values_on
    eng._h = None                      # (nothing to destroy)


def test_weight_must_be_finite():
    eng = _bare_engine()
    for w in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            eng.agents_set_value_weight(w)


def test_range_edge_is_accepted_by_the_python_check():
    """+-2^24 itself passes the Python check: the call reaches the library (here: the stand-in that fails the test by name)."""
    eng = _bare_engine()
    with pytest.raises(AssertionError, match="sf_values_set"):
        eng.values_set(np.full((6, 7), 1 << 24, dtype=np.int64))
    with pytest.raises(AssertionError, match="sf_values_set"):
        eng.values_set(np.full((6, 7), -(1 << 24), dtype=np.int32))


# ------------------------------------------------------------------------------ 5. NULL handles
def test_null_handle_refusals():
    from simfire_amd import _lib
    L = _lib.load()                        # (raises if the library has not been built)
    buf = np.zeros(4, dtype=np.int64)
    p = buf.ctypes.data_as(C.c_void_p)
    vp, i64 = C.c_void_p(), C.c_int64()
    assert L.sf_values_set(None, p, 0, 0) == _lib.SF_EINVAL
    assert L.sf_values_get(None, p) == _lib.SF_EINVAL
    assert L.sf_values_device(None, C.byref(vp), C.byref(i64), C.byref(vp)) == _lib.SF_EINVAL
    assert L.sf_values_set_weight(None, 1.0, 1) == _lib.SF_EINVAL
    assert L.sf_set_values_dense(None, 1) == _lib.SF_EINVAL
    assert L.sf_get_value_passes(None, p) == _lib.SF_EINVAL
