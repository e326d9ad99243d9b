"""Fire behaviour without a GPU (``sf_behavior``): the oracle's restated chain against the pinned one, worked
values for fuel model 1, the rules of head / classes / point form on a hand scene, every ``ValueError`` of ``BehaviorSpec``, and the
ABI (symbols, arities, struct layouts) against the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _behavior_oracle as bo
import _behavior_worlds as bw
import _golden
from oracle import rothermel_np as rnp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the oracle itself
def test_restated_chain_is_the_pinned_one():
    """I_R * xi / den of the restated chain reproduces ``R0`` of ``rate_of_spread(..., return_parts=True)`` bit for bit on the
    inputs of ``tests/golden/rothermel_grid.npz``, and that ``R0`` is the golden file's within the parity bound."""
    d = _golden.load("rothermel_grid.npz")
    a = {k[3:]: d[k] for k in d if k.startswith("in_")}
    _, parts = rnp.rate_of_spread(a["loc_x"], a["loc_y"], a["new_loc_x"], a["new_loc_y"], a["w_0"], a["delta"], a["M_x"], a["sigma"], a["h"],
                                  a["S_T"], a["S_e"], a["p_p"], a["M_f"], a["U"], a["U_dir"], a["slope_mag"], a["slope_dir"], return_parts=True)
    I_R, xi, den = bo.reaction_intensity(a["w_0"], a["delta"], a["M_x"], a["sigma"], a["h"], a["S_T"], a["S_e"], a["p_p"], a["M_f"], parts=True)
    ok = a["w_0"] > 0
    R0 = np.zeros(ok.shape)
    R0[ok] = (I_R[ok] * xi[ok]).astype(np.float64) / den[ok].astype(np.float64)
    assert ok.sum() > 1000 and (R0 == parts["R0"]).all()
    assert (I_R[~ok] == 0).all() and (I_R[ok] > 0).all()
    assert np.allclose(R0, d["R0"], rtol=1e-5, atol=0)


def test_fuel_model_1_worked_values():
    """NFFL / Anderson-13 fuel model 1, short grass (``simfire_amd.parameters.ShortGrass``: w_0 = 0.034 lb/ft2, delta = 1 ft, M_x =
    0.12, sigma = 3500 1/ft) with the default particle (h = 8000 BTU/lb, S_T = 0.0555, S_e = 0.01, p_p = 32 lb/ft3) at M_f = 0.03,
    worked in double precision with the equations of Rothermel (1972, INT-115) as restated by Andrews (2018, RMRS-GTR-371, table 5),
    Anderson's (1969) residence time t_r = 384 / sigma and Byram's (1959) L = 0.45 I_B ** 0.46:
      eta_S = 0.417397, eta_M = 0.616875, beta = 0.0010625, beta_op = 0.00419322, Gamma_max = 16.1837, A = 0.208656,
      Gamma = 14.2014 1/min, I_R = 939.393 BTU/ft2/min, t_r = 0.109714 min, HPA = 103.065 BTU/ft2, R (no wind, no slope) = 5.85515 ft/min
      -> I_B = 10.0577 BTU/ft/s, L = 1.30125 ft;  R = 100 ft/min -> I_B = 171.775 BTU/ft/s, L = 4.80058 ft."""
    from simfire_amd.parameters import FuelParticle, ShortGrass as f
    p = FuelParticle()
    I_R, xi, den = bo.reaction_intensity([f.w_0], [f.delta], [f.M_x], [f.sigma], p.h, p.S_T, p.S_e, p.p_p, 0.03, parts=True)
    assert I_R.dtype == np.float32 and abs(float(I_R[0]) / 939.3927812 - 1) < 1e-5
    hpa = bo.heat_per_area(I_R, [f.sigma], [f.w_0])
    assert hpa.dtype == np.float32 and abs(float(hpa[0]) / 103.0648080 - 1) < 1e-5
    R0 = float(I_R[0] * xi[0]) / float(den[0])
    assert abs(R0 / 5.855146993 - 1) < 1e-5
    R8 = np.zeros((8, 1, 2))
    R8[3, 0, 0], R8[6, 0, 1] = 5.855146993361697, 100.0
    c = bo.cells(R8, np.full((1, 2), hpa[0], dtype=np.float32))
    assert c["head"].tolist() == [[3, 6]] and all(c[k].dtype == np.float32 for k in ("ros", "intensity", "flame_length", "hpa"))
    assert np.allclose(c["intensity"][0], [10.05766001, 171.7746800], rtol=1e-5, atol=0)
    assert np.allclose(c["flame_length"][0], [1.301251104, 4.800580116], rtol=1e-5, atol=0)
    assert bo.workable(c["flame_length"], 4.0).tolist() == [[1, 0]]


def test_unburnable_cells_have_no_heat_whatever_their_sigma():
    I_R = bo.reaction_intensity([0.0, 0.034, -1.0], [1.0, 1.0, 1.0], [0.12, 0.12, 0.12], [0.0, 3500.0, 3500.0], 8000, 0.0555, 0.01, 32, 0.03)
    hpa = bo.heat_per_area(I_R, [0.0, 3500.0, 3500.0], [0.0, 0.034, -1.0])
    assert I_R[0] == 0 and I_R[2] == 0 and hpa[0] == 0 and hpa[2] == 0 and hpa[1] > 100 and np.isfinite(hpa).all()
    c = bo.cells(np.zeros((8, 1, 3)), hpa.reshape(1, 3))
    assert c["head"].tolist() == [[-1, -1, -1]] and not c["flame_length"].any() and not c["intensity"].any()


# ------------------------------------------------------------------------------------------------ the rules on the hand scene
def test_head_ties_and_empty_cells():
    R8, hpa, fm = bw.hand_scene()
    c = bo.cells(R8, hpa)
    assert c["head"][0, 0] == -1 and c["ros"][0, 0] == 0 and c["flame_length"][0, 0] == 0 and c["intensity"][0, 0] == 0
    assert c["head"][0, 1] == 2 and c["ros"][0, 1] == 7          # entries 2 and 5 tie: the lowest k
    assert c["head"][0, 2] == 0                                   # all eight tie
    assert c["head"][1, 1] == 7 and c["head"][2, 3] == 3 and c["head"][4, 0] == 1
    assert c["head"].dtype == np.int8 and np.allclose(c["intensity"], 10.0 * c["ros"], rtol=1e-6)
    assert np.allclose(c["flame_length"][2, 2], 0.45 * 1000.0 ** 0.46, rtol=1e-6)


def test_classes_and_maxima():
    R8, hpa, fm = bw.hand_scene()
    c = bo.cells(R8, hpa)
    L, I = c["flame_length"], c["intensity"]
    mf, mi, cls = bo.summary(L, I, fm, bw.mask_of(("BURNING",)))
    assert cls.tolist() == [1, 1, 1, 1, 0] and cls.dtype == np.int32      # 2.7 ft | 6.2 ft | 10.8 ft | 20.4 ft; the BURNED 7.08 ft is not selected
    assert mf == L[2, 3] and mi == I[2, 3] == np.float32(4000.0) and mf.dtype == np.float32
    mf, mi, cls = bo.summary(L, I, fm, bw.mask_of(("BURNING", "BURNED")))
    assert cls.tolist() == [1, 2, 1, 1, 0]
    mf, mi, cls = bo.summary(L, I, fm, bw.mask_of(("BURNING",)), edges=(1.0, 2.0, 3.0, 10.0))
    assert cls.tolist() == [0, 0, 1, 1, 2]
    # an edge is part of the class above it, compared as float32
    e = float(L[3, 3])
    assert bo.summary(L, I, fm, bw.mask_of(("BURNING",)), edges=(e, 8.0, 11.0, 1e30))[2].tolist() == [0, 2, 1, 1, 0]
    mf, mi, cls = bo.summary(L, I, fm, bw.mask_of(("WETLINE",)))
    assert mf == 0 and mi == 0 and cls.tolist() == [0] * 5                # nothing selected
    m = bo.masked(c, fm, bw.mask_of(("BURNING",)))
    assert (m["head"][fm != 1] == -1).all() and not m["flame_length"][fm != 1].any() and (m["flame_length"][fm == 1] == L[fm == 1]).all()
    assert bo.workable(m["flame_length"], 8.0).sum() == 25 - 2            # hidden cells show 0 and are workable


def test_point_rule():
    R8, hpa, fm = bw.hand_scene()
    L = bo.cells(R8, hpa)["flame_length"]
    burning = bw.mask_of(("BURNING",))
    pts = [(2, 2, 1), (0, 0, 1), (4, 4, 1), (4, 0, 1), (3, 2, 0), (5, 2, 1), (2, -1, 1), (3, 3, -2), (0, 0, 1), (4, 3, 7)]
    got = bo.point_flame(L, fm, burning, pts)
    want = [L[2, 3], L[1, 1], L[3, 3], 0.0, -1.0, -1.0, -1.0, -1.0, L[1, 1], L[2, 3]]
    assert got.dtype == np.float32 and got.tolist() == [float(v) for v in want]
    assert bo.point_flame(L, fm, bw.mask_of(("BURNED",)), [(4, 4, 1), (0, 0, 1)]).tolist() == [float(L[4, 4]), 0.0]


# ------------------------------------------------------------------------------------------------ BehaviorSpec
def _spec(**kw):
    from simfire_amd.behavior import BehaviorSpec
    return BehaviorSpec(4, 9, 12, **kw)


def test_spec_defaults_and_outputs():
    s = _spec()
    assert list(s.outputs) == ["flame_length"] and s.outputs["flame_length"] == ((4, 9, 12), "float32")
    assert (s.status, s.summary, s.flame_limit, s.k) == (0, 2, None, 0) and s.edges == tuple(float(np.float32(v)) for v in (4, 8, 11, 1e30))
    s = _spec(envs=[3, 3, 0], planes=("head", "hpa", "ros", "intensity"), workable=True, flame_limit=4, stats=True, status=("BURNING", 2),
              summary="BURNED", edges=(1, 2, 3, 4))
    assert list(s.outputs) == ["hpa", "ros", "intensity", "head", "workable", "max_flame", "max_intensity", "classes"]
    assert s.outputs["head"] == ((3, 9, 12), "int8") and s.outputs["workable"] == ((3, 9, 12), "uint8") and s.outputs["classes"] == ((3, 5), "int32")
    assert (s.status, s.summary, s.flame_limit) == (6, 4, 4.0)
    p = s.params()
    assert (p.status_mask, p.summary_mask, p.k, p.reserved, p.flame_limit, list(p.edges), p.points) == (6, 4, 0, 0, 4.0, [1, 2, 3, 4], None)
    assert list(_spec(planes=(), stats=True).outputs) == ["max_flame", "max_intensity", "classes"]
    assert list(_spec(planes="ros").outputs) == ["ros"]


@pytest.mark.parametrize("kw,word", [
    (dict(planes=("flames",)), "unknown plane"),
    (dict(planes=5), "planes"),
    (dict(planes=()), "nothing asked for"),
    (dict(planes=None), "nothing asked for"),
    (dict(workable=True), "flame_limit"),
    (dict(workable=1), "True or False"),
    (dict(stats="yes"), "True or False"),
    (dict(flame_limit=-1.0), "flame_limit"),
    (dict(flame_limit=float("nan")), "flame_limit"),
    (dict(flame_limit="4"), "flame_limit"),
    (dict(flame_limit=True), "flame_limit"),
    (dict(edges=(4, 8, 11)), "edges"),
    (dict(edges=(4, 8, 8, 11)), "edges"),
    (dict(edges=(4, 8, 11, float("nan"))), "edges"),
    (dict(edges=(11, 8, 4, 1)), "edges"),
    (dict(edges=(1.0, 1.0 + 1e-9, 2, 3)), "edges"),                     # equal as float32
    (dict(edges=7), "edges"),
    (dict(edges=("a", 1, 2, 3)), "edge"),
    (dict(status=64), "mask"),
    (dict(status=("SMOKING",)), "BurnStatus"),
    (dict(summary=0), "mask"),
    (dict(summary=()), "mask"),
    (dict(summary=("BURNING", 9)), "BurnStatus"),
    (dict(envs=[4]), "environment"),
    (dict(envs=[-1]), "environment"),
    (dict(envs=[0.5]), "envs"),
    (dict(envs=[[0, 1]]), "envs"),
    (dict(points=np.zeros((4, 2, 3), dtype=np.int32)), "points"),        # a host array: the point form takes device tensors only
])
def test_spec_refuses(kw, word):
    with pytest.raises(ValueError, match=word):
        _spec(**kw)


def test_env_option_is_checked_before_anything_is_created():
    from simfire_amd.vecenv import BatchedFireEnv

    class Sim:
        n_envs, _engine = 2, None
    for bad in (5, dict(limit=4), dict(edges=(3, 2, 1, 0)), dict(summary=("NOPE",)), dict(flame_limit=-2)):
        with pytest.raises(ValueError, match="BatchedFireEnv: behavior"):
            BatchedFireEnv(Sim(), 1, [[0, 0]], behavior=bad)


# ------------------------------------------------------------------------------------------------ the ABI
def _header(name="simfire_hip.h"):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_prototypes_are_bound_with_matching_arity():
    from simfire_amd import _lib
    protos = dict(re.findall(r"\bint\s+(sf_\w*behavior\w*)\s*\(([^)]*)\)\s*;", _header() + _header("simfire_hip_lab.h")))
    assert set(protos) == {"sf_behavior", "sf_get_behavior_builds"}
    for name, args in protos.items():
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name]) == len([a for a in args.split(",") if a.strip()]), name
    lib = _lib.load()
    for name in protos:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name]
    assert _lib.SIGNATURES["sf_behavior"][1:3] == [C.POINTER(_lib.SfBehaviorParams), C.POINTER(_lib.SfBehaviorOut)]


@pytest.mark.parametrize("struct,cls,total", [("sf_behavior_params", "SfBehaviorParams", 48), ("sf_behavior_out", "SfBehaviorOut", 80)])
def test_struct_layouts_match_the_header(struct, cls, total):
    from simfire_amd import _lib
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), _header(), re.S).group(1)
    size_of = {"int32_t": 4, "float": 4, "int8_t": 1, "uint8_t": 1}
    fields, size = [], 0
    for decl in body.split(";"):
        decl = decl.replace("const", "").strip()
        if not decl:
            continue
        ty, names = decl.split(None, 1)
        for nm in names.split(","):
            nm = nm.strip()
            ptr = nm.startswith("*")
            m = re.fullmatch(r"\*?\s*(\w+)(?:\[(\d+)\])?", nm)
            fields.append(m.group(1))
            if ptr:
                size = (size + 7) // 8 * 8 + 8
            else:
                size += size_of[ty] * int(m.group(2) or 1)
    ct = getattr(_lib, cls)
    assert [f[0] for f in ct._fields_] == fields
    assert C.sizeof(ct) == size == total


def test_heat_cache_flag_follows_the_terrain_not_the_wind():
    """``hpa_stale`` in ``sf_tables.h`` is set by whatever sets ``wt_stale`` and by a terrain copy, never by ``wind_rebuilt``."""
    src = open(os.path.join(ROOT, "simfire_amd", "csrc", "sf_tables.h")).read()
    body = {}
    for name in ("layers_set", "rtable_set", "wind_rebuilt", "copied"):
        at = src.index("    void %s(" % name)
        body[name] = src[at:src.index("\n    }", at)]
    assert "hpa_stale" in body["rtable_set"] and "rtable_set(tabs, n)" in body["layers_set"] and "hpa_stale" in body["copied"]
    assert "hpa_stale" not in body["wind_rebuilt"]
    assert re.search(r"hpa_stale = 1; \};", src)                           # a fresh table starts stale
