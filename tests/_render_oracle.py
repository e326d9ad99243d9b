"""NumPy restatement of the frames of ``render`` (simfire_amd/csrc/sf_render_kernels.h).

Every step is written in the arithmetic the kernels use, so that the GPU tests compare bit for bit:
- the fuel colour: FuelLayer._update_texture_dryness (simfire/utils/layers.py:744-768) - pct in float64, alpha = float32(pct / 2),
  then Pillow's ImagingBlend per channel in float32 (truncated; clipped when alpha is outside [0, 1]);
- FBFM codes: FuelModelRGB13[code] * 255.0 truncated to uint8 (layers.py:654-667, sprites.py:136-160);
- contour levels: matplotlib's automatic choice for ax.contour(z) (MaxNLocator(8, min_n_ticks=1)) in plain float64, trimmed to the
  levels strictly inside (zmin, zmax), [zmin] if none is; a cell is a contour pixel iff min(z, z_n) < L <= max(z, z_n) for a level
  L and its right or lower neighbour n;
- sprites on top, then the integer downscale ("nearest", "mean", "sprites").
"""
import math

import numpy as np

BROWN = (205, 133, 63)                      # DRY_TERRAIN_BROWN_IMG (simfire/enums.py:45-47)
BURNED = (139, 69, 19)                      # BURNED_RGB_COLOR
BURNING = (255, 153, 51)
LINE = (255, 0, 0)                          # FIRELINE and SCRATCHLINE
WETLINE = (212, 241, 249)
AGENT = (221, 160, 221)

FBFM_RGB13 = {
    1: [1.0, 1.0, 0.745098039], 2: [1.0, 1.0, 0.0], 3: [0.901960784, 0.77254902, 0.043137255], 4: [1.0, 0.82745098, 0.498039216],
    5: [1.0, 0.666666667, 0.4], 6: [0.803921569, 0.666666667, 0.4], 7: [0.537254902, 0.439215686, 0.266666667],
    8: [0.82745098, 1.0, 0.745098039], 9: [0.439215686, 0.658823529, 0.0], 10: [0.149019608, 0.450980392, 0.0],
    11: [0.909803922, 0.745098039, 1.0], 12: [0.478431373, 0.556862745, 0.960784314], 13: [0.77254902, 0.0, 1.0],
    91: [0.517647, 0.0, 0.541176], 92: [0.623529, 0.631373, 0.941176], 93: [0.913725, 0.45098, 1.0], 98: [0.0, 0.0, 1.0],
    99: [0.74902, 0.74902, 0.74902], -32768: [1.0, 1.0, 1.0], -9999: [1.0, 1.0, 1.0], 32767: [1.0, 1.0, 1.0],
}


# ------------------------------------------------------------------------------------------------------------- fuel colours
def blend(base, alpha):
    """Pillow's Image.blend(base, BROWN, alpha) per channel for float32 alpha of any shape -> uint8 [..., 3]."""
    a = np.asarray(alpha, dtype=np.float32)[..., None]
    in1 = np.asarray(base, dtype=np.int64)
    d = (np.asarray(BROWN, dtype=np.int64) - in1).astype(np.float32)
    v = in1.astype(np.float32) + a * d                       # float32 multiply, then float32 add
    inside = (a >= 0) & (a <= 1)
    clipped = np.where(v <= 0, np.float32(0), np.where(v >= 255, np.float32(255), v))
    return np.where(inside, v, clipped).astype(np.int64).astype(np.uint8)


def dryness_alpha(w_0, delta, M_x):
    pct = np.asarray(w_0, dtype=np.float64) / 0.2296 + np.asarray(delta, dtype=np.float64) / 7 + \
        (0.2 - np.asarray(M_x, dtype=np.float64)) / 0.2
    pct = pct / 3
    return (pct / 2).astype(np.float32)


def fuel_rgb(w_0, delta, M_x, base):
    """The functional FuelLayer.image of cells with these fuel scalars: uint8 [..., 3]."""
    return blend(base, dryness_alpha(w_0, delta, M_x))


def fbfm_rgb(codes):
    """FBFM13 codes -> uint8 [..., 3]; a code without a colour is white."""
    codes = np.asarray(codes)
    out = np.full(codes.shape + (3,), 255, dtype=np.uint8)
    for c, v in FBFM_RGB13.items():
        out[codes == c] = (np.asarray(v, dtype=np.float64) * 255.0).astype(np.uint8)
    return out


# ---------------------------------------------------------------------------------------------------------- contour levels
def _divmod(a, b):
    return divmod(float(a), float(b))


def contour_levels(zmin, zmax):
    """matplotlib's automatic levels for ax.contour(z) with z.min() = zmin, z.max() = zmax, strictly inside; [zmin] if none."""
    zmin, zmax = float(zmin), float(zmax)
    expander, tiny = 1e-13, 1e-14
    vmin, vmax = zmin, zmax
    if not (math.isfinite(vmin) and math.isfinite(vmax)):
        vmin, vmax = -expander, expander
    else:
        mabs = max(abs(vmin), abs(vmax))
        if mabs < (1e6 / tiny) * np.finfo(float).tiny:
            vmin, vmax = -expander, expander
        elif vmax - vmin <= mabs * tiny:
            if vmax == 0 and vmin == 0:
                vmin, vmax = -expander, expander
            else:
                vmin -= expander * abs(vmin)
                vmax += expander * abs(vmax)
    nbins = 8
    dv = abs(vmax - vmin)
    meanv = (vmax + vmin) / 2
    offset = 0.0 if abs(meanv) / dv < 100 else math.copysign(10 ** (math.log10(abs(meanv)) // 1), meanv)
    scale = 10 ** (math.log10(dv / nbins) // 1)
    _vmin, _vmax = vmin - offset, vmax - offset
    base = [1, 1.5, 2, 2.5, 3, 4, 5, 6, 8, 10]
    steps = [(0.1 * b) * scale for b in base[:-1]] + [b * scale for b in base] + [(10 * base[1]) * scale]
    raw = (_vmax - _vmin) / nbins
    istep = next((i for i, s in enumerate(steps) if s >= raw), len(steps) - 1)
    ticks = []
    for step in steps[:istep + 1][::-1]:
        best = _divmod(_vmin, step)[0] * step
        tol = 1e-10
        if abs(offset) > 0:
            digits = math.log10(abs(offset) / step)
            tol = min(0.4999, max(1e-10, 10 ** (digits - 12)))
        d, m = _divmod(_vmin - best, step)
        low = d + 1 if abs(m / step - 1) < tol else d
        d, m = _divmod(_vmax - best, step)
        high = d if abs(m / step - 0) < tol else d + 1
        ticks = [k * step + best for k in np.arange(low, high + 1)]
        if sum(1 for t in ticks if _vmin <= t <= _vmax) >= 1:
            break
    levels = [t + offset for t in ticks]
    inside = [L for L in levels if zmin < L < zmax]
    return inside if inside else [zmin]


def contour_mask(z, levels=None):
    """bool [H, W]: the contour pixels of elevation z."""
    z = np.asarray(z, dtype=np.float64)
    if levels is None:
        levels = contour_levels(z.min(), z.max())
    m = np.zeros(z.shape, dtype=bool)
    for L in levels:
        lo, hi = np.minimum(z[:, :-1], z[:, 1:]), np.maximum(z[:, :-1], z[:, 1:])
        m[:, :-1] |= (lo < L) & (L <= hi)
        lo, hi = np.minimum(z[:-1], z[1:]), np.maximum(z[:-1], z[1:])
        m[:-1] |= (lo < L) & (L <= hi)
    return m


# --------------------------------------------------------------------------------------------------------------- the frame
def agent_cells(agents, H, W):
    """(row, column) of the entries of an [k, 3] (column, row, id) list that update_agent_positions leaves on a fresh map."""
    out = []
    if agents is None:
        return out
    a = np.asarray(agents).reshape(-1, 3)
    for j, (x, y, i) in enumerate(a):
        if not (i > 0 and 0 <= x < W and 0 <= y < H):
            continue
        win = True
        for (x2, y2, i2) in a[j + 1:]:
            if i2 > 0 and 0 <= x2 < W and 0 <= y2 < H and (i2 == i or (x2 == x and y2 == y)):
                win = False
        if win:
            out.append((int(y), int(x)))
    return out


def frame(status, fuel, contours_mask, agents=None, background="fuel", contours=True):
    """Full-resolution frame uint8 [H, W, 3] and sprite priority int [H, W] (0 none, 1 burning, 2 fireline, 3 scratchline,
    4 wetline, 5 agent).  status: BurnStatus [H, W]; fuel: uint8 [H, W, 3] fuel colours; contours_mask: bool [H, W]."""
    s = np.asarray(status).astype(np.int64) & 7
    H, W = s.shape
    img = np.full((H, W, 3), 255, dtype=np.uint8) if background == "white" else np.array(fuel, dtype=np.uint8, copy=True)
    if contours:
        img[contours_mask] = 0
    prio = np.zeros((H, W), dtype=np.int64)
    for v, col, p in ((2, BURNED, 0), (1, BURNING, 1), (3, LINE, 2), (4, LINE, 3), (5, WETLINE, 4)):
        img[s == v] = col
        prio[s == v] = p
    for (y, x) in agent_cells(agents, H, W):
        img[y, x] = AGENT
        prio[y, x] = 5
    return img, prio


def downscale(img, prio, scale, mode):
    """uint8 [ceil(H / scale), ceil(W / scale), 3]; the last partial block uses the cells it has."""
    if scale == 1:
        return img.copy()
    H, W = prio.shape
    oh, ow = -(-H // scale), -(-W // scale)
    if mode == "nearest":
        return img[::scale, ::scale].copy()
    out = np.empty((oh, ow, 3), dtype=np.uint8)
    for oy in range(oh):
        for ox in range(ow):
            bi = img[oy * scale:(oy + 1) * scale, ox * scale:(ox + 1) * scale].reshape(-1, 3).astype(np.int64)
            bp = prio[oy * scale:(oy + 1) * scale, ox * scale:(ox + 1) * scale].reshape(-1)
            if mode == "sprites" and bp.max() > 0:
                out[oy, ox] = bi[int(np.argmax(bp))]
            else:
                n = bi.shape[0]
                out[oy, ox] = (bi.sum(axis=0) + n // 2) // n
    return out


def render(status, fuel, contours_mask, scale=1, mode=None, agents=None, background="fuel", contours=True):
    """The frame of ``render`` for one environment (channels last)."""
    if mode is None:
        mode = "sprites" if scale > 1 else "nearest"
    img, prio = frame(status, fuel, contours_mask, agents=agents, background=background, contours=contours)
    return downscale(img, prio, scale, mode)
