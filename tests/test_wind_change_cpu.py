"""Wind changes during an episode, the parts that need no GPU: the semantics pinned on the two oracles -
a table swapped between two updates is the reference manager with ``U`` / ``U_dir`` reassigned between two ``update()`` calls
(simfire/game/managers/fire.py:365, 490-494) -, the header and the library's exports, the argument errors raised before any device
work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import fire_dense, fire_sprites, rothermel_np
from simfire_amd.parameters import fuel_planes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

H, W, MD, PS, M_F = 24, 31, 5, 30.0, 0.03
A, B = 3, 14                       # updates before / after the shift; A < max_fire_duration: sprites of the old wind are still alive
INIT = (9, 12)
U1, D1, U2, D2 = 20 * 88.0, 90.0, 20 * 88.0, 270.0       # 20 mph, reversed


def _world():
    rng = np.random.default_rng(7)
    codes = rng.choice([1, 2, 4, 5, 9], size=(H, W))
    codes[3:6, 20:24] = 98                                # not burnable
    w0, de, mx, sg = fuel_planes(codes)
    y, x = np.mgrid[0:H, 0:W]
    elev = 40.0 * np.sin(x / 5.0) + 25.0 * np.cos(y / 4.0)
    return w0, de, mx, sg, elev


# a fire line across the fire's way down-wind of the ignition, crossed while the first wind blows, and a wet line up-wind, crossed
# after the reversal (what it is owed by then has accumulated under both winds)
LINE_X = {fire_sprites.FIRELINE: 11, fire_sprites.WETLINE: 5}
LINES = [(0, LINE_X[fire_sprites.FIRELINE], y, fire_sprites.FIRELINE) for y in range(8, 17)] + \
        [(0, LINE_X[fire_sprites.WETLINE], y, fire_sprites.WETLINE) for y in range(6, 19)]


PARTICLE = (8000.0, 0.0555, 0.01, 32.0)


def _layers(U, D):
    w0, de, mx, sg, elev = _world()
    mag, dr = fire_dense.slopes(elev, PS)
    return dict(w_0=w0, delta=de, M_x=mx, sigma=sg, U=np.full((H, W), U), U_dir=np.full((H, W), D), slope_mag=mag, slope_dir=dr)


def _table(o, U, D, libm):
    """The table of wind (U, D): ``libm`` - DenseOracle.build_rtable followed by set_rtable of what it built; else the NumPy
    formula SpriteFire evaluates in layers mode (oracle/rothermel_np.py), handed over by set_rtable."""
    w0, de, mx, sg, elev = _world()
    if libm:
        o.build_rtable(w0, de, mx, sg, elev, U, D, M_F)
        T = o.get_rtable()
    else:
        L = _layers(U, D)
        T = rothermel_np.rtable(L["w_0"], L["delta"], L["M_x"], L["sigma"], *PARTICLE, M_F, L["U"], L["U_dir"], L["slope_mag"], L["slope_dir"])
    o.set_rtable(T)
    return T


def _dense(diag, shift, libm):
    o = fire_dense.DenseOracle(shape=(H, W), n_envs=1, max_fire_duration=MD, pixel_scale=PS, update_rate=1.0, max_time=None,
                               attenuate_line_ros=True, diagonal_spread=diag)
    tables = [_table(o, U1, D1, libm)]
    o.reset([INIT])
    o.apply_mitigation(LINES)
    out = []
    for t in range(A + B):
        if t == A and shift:
            tables.append(_table(o, U2, D2, libm))
        o.step(1)
        out.append((o.fire_map(0).copy(), o.burn(0).copy(), float(o.status()[1][0]), int(o.status()[0][0, 0])))
    return out, tables


def _sprites(diag, tables):
    """``tables`` None: layers mode, layers["U"] / ["U_dir"] reassigned after A updates; else table mode over the given two tables,
    the second assigned after A updates."""
    full = lambda v: np.full((H, W), v)
    s = fire_sprites.SpriteFire((H, W), INIT, MD, PS, 1.0, layers=_layers(U1, D1) if tables is None else None,
                                rtable=None if tables is None else tables[0], M_f=M_F, particle=PARTICLE,
                                attenuate_line_ros=True, diagonal_spread=diag)
    fm = np.zeros((H, W), dtype=np.int64)
    fm[INIT[1], INIT[0]] = fire_sprites.BURNING
    fire_sprites.apply_mitigation(fm, [(x, y, t) for (_, x, y, t) in LINES])
    out, running = [], True
    for t in range(A + B):
        if t == A and tables is None:
            s.layers["U"], s.layers["U_dir"] = full(U2), full(D2)        # fire.py:365, 490-494: read at every update()
        elif t == A:
            s.rtable = tables[1]
        if running:
            fm, st = s.update(fm)
            running = st == fire_sprites.RUNNING
        out.append((fm.astype(np.uint8), s.burn.copy(), float(s.elapsed_time), int(running)))
    return out


@pytest.mark.parametrize("libm", [False, True], ids=["layers-mode", "build_rtable"])
@pytest.mark.parametrize("diag", [True, False], ids=["8-connected", "4-connected"])
def test_table_swap_between_updates_is_the_reference_with_wind_reassigned(diag, libm):
    """DenseOracle with its table replaced by that of (U2, dir2) after A updates == SpriteFire with the wind reassigned after A
    updates, bit for bit in map, burn_amounts (the lines' attenuation included) and elapsed time after every update; the line is
    crossed; and the shift matters: the final map differs from the run that keeps wind 1.

    Two pairings, because the two oracles do not share one arithmetic: build_rtable evaluates the float32 transcendentals with
    libm in float64, SpriteFire's layers mode with NumPy's float32 routines, and for this world all 8 x 24 x 31 table entries but
    the unburnable ones differ in their last bits (burn_amounts after the first update: 3.3e-5 apart).  "layers-mode": SpriteFire
    in layers mode with layers["U"] / ["U_dir"] reassigned, DenseOracle over the tables the same NumPy formula gives for the two
    winds.  "build_rtable": DenseOracle.build_rtable followed by set_rtable of what it built, SpriteFire over those two tables."""
    (dense, tables), (kept, _) = _dense(diag, True, libm), _dense(diag, False, libm)
    ref = _sprites(diag, tables if libm else None)
    for t, (d, r) in enumerate(zip(dense, ref)):
        assert d[3] == r[3], t
        assert (d[0] == r[0]).all(), (t, int((d[0] != r[0]).sum()))
        assert (d[1] == r[1]).all(), (t, float(np.abs(d[1] - r[1]).max()))
        assert d[2] == r[2], t
    final = dense[-1][0]
    assert dense[-1][3] == 1, "the fire must still be running at the end (else the comparison stops early)"
    burnt = lambda m, x: ((m[:, x] == fire_sprites.BURNING) | (m[:, x] == fire_sprites.BURNED)).any()
    assert burnt(dense[A - 1][0], LINE_X[fire_sprites.FIRELINE]), "the fire line was not crossed under the first wind"
    assert not burnt(dense[A - 1][0], LINE_X[fire_sprites.WETLINE]) and burnt(final, LINE_X[fire_sprites.WETLINE]), \
        "the wet line was not crossed after the shift"
    assert (dense[A - 1][0] == kept[A - 1][0]).all()
    assert (final != kept[-1][0]).any(), "the wind shift changed nothing"


def test_header_declares_and_library_exports_the_wind_entries():
    from simfire_amd import _lib
    header = open(os.path.join(ROOT, "include", "simfire_hip.h")).read()
    for name, n_args in (("sf_set_wind", 6), ("sf_set_wind_schedule", 5)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert len(_lib.SIGNATURES[name]) == n_args
        assert hasattr(_lib.load(), name)
    # each entry cites the lines of the reference it stands for
    for name in ("sf_set_wind", "sf_set_wind_schedule"):
        decl = header.index("int " + name + "(")
        comment = header.rfind("\n/*", 0, decl)            # the block comment in front of the entry and its constants
        assert "fire.py:365, 490-494" in header[comment:decl], name
    for word, value in (("SF_WIND_UNIFORM", 0), ("SF_WIND_FIELD", 1), ("SF_WIND_DEVICE", 2), ("SF_WIND_MAX_SEGS", 16)):
        assert re.search(r"#define\s+%s\s+%d\b" % (word, value), header), word
        assert getattr(_lib, word) == value
    assert C.sizeof(_lib.SfWindSeg) == 24


def test_argument_errors_before_any_device_work():
    """What is refused without a handle needs no device: a null handle is SF_EINVAL (ValueError) for both entries."""
    from simfire_amd import _lib
    lib = _lib.load()
    u = np.zeros(1)
    env = np.zeros(1, dtype=np.int32)
    rc = lib.sf_set_wind(None, 1, env.ctypes.data, u.ctypes.data, u.ctypes.data, 0)
    assert rc == _lib.SF_EINVAL and b"sf_set_wind" in lib.sf_last_error()
    with pytest.raises(ValueError):
        _lib.check(rc)
    seg = _lib.SfWindSeg(0, 0, 100.0, 0.0)
    rc = lib.sf_set_wind_schedule(None, 1, env.ctypes.data, 1, C.cast(C.pointer(seg), C.c_void_p))
    assert rc == _lib.SF_EINVAL and b"sf_set_wind_schedule" in lib.sf_last_error()
