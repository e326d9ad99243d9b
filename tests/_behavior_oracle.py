"""ORACLE of ``sf_behavior`` (test infrastructure, never imported by the product): the definitions of
fire behaviour per cell restated in NumPy with the dtype of every step spelled out.

* ``reaction_intensity``: the float32 chain of ``oracle/rothermel_np.py`` lines 61-73 (rothermel.py:74-92), restated - with
  ``xi`` and ``den`` beside it, so that ``tests/test_behavior_cpu.py`` can hold the restatement against the pinned ``R0``.
* everything behind it is float64 with ONE rounding per output: ``HPA = f32(f64(I_R) * (384 / f64(sigma)))``,
  ``R_head = max_k R8[k]``, ``I_B = f32(f64(HPA) * R_head / 60)``, ``L = f32(0.45 * I_B64 ** 0.46)``, both 0 where the float64
  ``I_B`` is not > 0.

Units are the reference's: feet, minutes, pounds, BTU.
"""
import numpy as np

F32 = np.float32
DEFAULT_EDGES = (4.0, 8.0, 11.0, 1e30)


def _f32(a, n=None):
    a = np.asarray(a, dtype=F32)
    return np.ascontiguousarray(np.broadcast_to(a, (n,)) if a.ndim == 0 else a.reshape(-1))


def reaction_intensity(w_0, delta, M_x, sigma, h, S_T, S_e, p_p, M_f, parts=False):
    """``I_R`` float32 [n] (BTU/ft2/min), 0 where ``w_0 <= 0``; with ``parts`` also (xi, den) float32 [n] (1 where ``w_0 <= 0``):
    the propagating flux ratio and ``p_b * eps * Q_ig`` of rothermel.py:94, 121-128."""
    w_0 = _f32(w_0)
    n = w_0.shape[0]
    delta, M_x, sigma = _f32(delta, n), _f32(M_x, n), _f32(sigma, n)
    h, S_T, S_e, p_p, M_f = _f32(h, n), _f32(S_T, n), _f32(S_e, n), _f32(p_p, n), _f32(M_f, n)
    I_out, xi_out, den_out = np.zeros(n, dtype=F32), np.ones(n, dtype=F32), np.ones(n, dtype=F32)
    ok = w_0 > 0                                                      # rothermel.py:54
    if ok.any():
        w_0, delta, M_x, sigma = w_0[ok], delta[ok], M_x[ok], sigma[ok]
        h, S_T, S_e, p_p, M_f = h[ok], S_T[ok], S_e[ok], p_p[ok], M_f[ok]
        one = np.ones_like(w_0)
        eta_S = np.minimum(0.174 * S_e ** -0.19, one)                     # :74
        r_M = np.minimum(M_f / M_x, one)                                  # :76
        eta_M = 1 - 2.59 * r_M + 5.11 * r_M ** 2 - 3.52 * r_M ** 3        # :77
        w_n = w_0 * (1 - S_T)                                             # :79
        p_b = w_0 / delta                                                 # :81
        beta = p_b / p_p                                                  # :83
        beta_op = 3.348 * sigma ** -0.8189                                # :85
        s15 = sigma ** 1.5
        gamma_max = s15 / (495 + 0.0594 * s15)                            # :87
        A = 133 * sigma ** -0.7913                                        # :88
        ratio = beta / beta_op
        gamma = gamma_max * ratio ** A * np.exp(A * (1 - ratio))          # :90
        I_R = gamma * w_n * h * eta_M * eta_S                             # :92
        xi = np.exp((0.792 + 0.681 * sigma ** 0.5) * (beta + 0.1)) / (192 + 0.2595 * sigma)  # :94
        eps = np.exp(-138 / sigma)                                        # :121
        Q_ig = 250 + 1116 * M_f                                           # :123
        den = p_b * eps * Q_ig                                            # :128
        assert I_R.dtype == F32 and xi.dtype == F32 and den.dtype == F32
        I_out[ok], xi_out[ok], den_out[ok] = I_R, xi, den
    return (I_out, xi_out, den_out) if parts else I_out


def heat_per_area(I_R, sigma, w_0):
    """``HPA`` float32 (BTU/ft2), the shape of ``I_R``: ``I_R * t_r`` with Anderson's residence time ``t_r = 384 / sigma`` minutes,
    in float64 from the float32 ``I_R`` and ``sigma``, rounded once; 0 where ``w_0 <= 0`` (whatever sigma is there)."""
    I_R = np.asarray(I_R, dtype=F32)
    s = np.broadcast_to(np.asarray(sigma, dtype=F32), I_R.shape).astype(np.float64)
    burn = np.broadcast_to(np.asarray(w_0, dtype=F32), I_R.shape) > 0
    out = np.zeros(I_R.shape, dtype=F32)
    out[burn] = (I_R.astype(np.float64)[burn] * (384.0 / s[burn])).astype(F32)
    return out


def hpa_plane(layers, particle, M_f):
    """``HPA`` [H, W] of a terrain: ``layers`` = (w_0, delta, M_x, sigma, ...) planes, ``particle`` = (h, S_T, S_e, p_p)."""
    w_0, delta, M_x, sigma = (np.asarray(a, dtype=np.float64) for a in layers[:4])
    h, S_T, S_e, p_p = particle
    I_R = reaction_intensity(w_0, delta, M_x, sigma, h, S_T, S_e, p_p, M_f).reshape(w_0.shape)
    return heat_per_area(I_R, sigma, w_0)


def cells(R8, hpa):
    """The unmasked planes of one environment from its table ``R8`` float64 [8, H, W] and ``hpa`` float32 [H, W]:
    dict(hpa, ros, intensity, flame_length float32, head int8)."""
    R8 = np.asarray(R8, dtype=np.float64)
    m = R8.max(axis=0)
    head = R8.argmax(axis=0)                                             # (the first maximum: the lowest k)
    head = np.where((R8 != 0).any(axis=0), head, -1).astype(np.int8)
    ib64 = np.asarray(hpa, dtype=F32).astype(np.float64) * m / 60.0
    pos = ib64 > 0
    ib64 = np.where(pos, ib64, 0.0)
    L = np.zeros(ib64.shape, dtype=np.float64)
    L[pos] = 0.45 * ib64[pos] ** 0.46
    return dict(hpa=np.asarray(hpa, dtype=F32), ros=m.astype(F32), intensity=ib64.astype(F32), flame_length=L.astype(F32), head=head)


def in_mask(fire_map, mask):
    """bool [H, W]: the cells whose BurnStatus ``mask`` (bit s = BurnStatus s; 0 or None: every cell) selects."""
    fm = np.asarray(fire_map).astype(np.int64) & 7
    if not mask:
        return np.ones(fm.shape, dtype=bool)
    return ((int(mask) >> fm) & 1).astype(bool)


def masked(planes, fire_map, status_mask):
    """The planes as a call with ``status_mask`` shows them: 0 (head: -1) outside the mask."""
    sel = in_mask(fire_map, status_mask)
    return {k: np.where(sel, v, np.int8(-1) if k == "head" else v.dtype.type(0)).astype(v.dtype) for k, v in planes.items()}


def workable(flame_plane, flame_limit):
    return (np.asarray(flame_plane, dtype=F32) <= F32(flame_limit)).astype(np.uint8)


def summary(flame, intensity, fire_map, summary_mask, edges=DEFAULT_EDGES):
    """(max_flame float32, max_intensity float32, classes int32 [5]) over the cells ``summary_mask`` selects, from the UNMASKED
    float32 planes; the class comparison runs on the float32 values."""
    sel = in_mask(fire_map, summary_mask)
    L, I = np.asarray(flame, dtype=F32)[sel], np.asarray(intensity, dtype=F32)[sel]
    e = np.asarray(edges, dtype=F32)
    cls = (L[:, None] >= e[None, :]).sum(axis=1)
    return (F32(L.max()) if L.size else F32(0), F32(I.max()) if I.size else F32(0),
            np.bincount(cls, minlength=5).astype(np.int32))


def point_flame(flame, fire_map, summary_mask, pts):
    """float32 [k]: per point (column, row, id) the largest flame length over the cells of its 3 x 3 block that are on the grid and
    selected by ``summary_mask`` (0: none); -1 for id <= 0 or a cell off the grid."""
    flame = np.asarray(flame, dtype=F32)
    H, W = flame.shape
    sel = in_mask(fire_map, summary_mask)
    out = np.empty(len(pts), dtype=F32)
    for j, (x, y, pid) in enumerate(np.asarray(pts).tolist()):
        if pid <= 0 or not (0 <= x < W and 0 <= y < H):
            out[j] = -1
            continue
        y0, y1, x0, x1 = max(y - 1, 0), min(y + 2, H), max(x - 1, 0), min(x + 2, W)
        v = flame[y0:y1, x0:x1][sel[y0:y1, x0:x1]]
        out[j] = v.max() if v.size else 0
    return out
