"""NumPy restatement of ``sf_distance`` (include/simfire_hip.h) from a [H, W] status map: the literal minimum
over the selected cells of (y - y')^2 + (x - x')^2, in int64, chunked so that memory stays small.  Not the kernels' two passes.

Two cuts that change no value keep it quick on the test grids: a selected cell has distance 0 and takes no part in the search,
and a selected cell whose four neighbours are all selected (or off the grid) is left out of the candidates - for any cell outside
the set, the neighbour of such a cell one step along the longer axis towards it is selected too and strictly nearer, so the minimum
is never attained there alone.  ``tests/test_distance_cpu.py`` holds the result against ``scipy.ndimage.distance_transform_edt``."""
import numpy as np

FAR = 2 ** 31 - 1
STATUS = dict(UNBURNED=0, BURNING=1, BURNED=2, FIRELINE=3, SCRATCHLINE=4, WETLINE=5)
CHUNK = 1 << 22                      # pairs (cell, candidate) held at once


def mask_of(names):
    m = 0
    for n in names:
        m |= 1 << (STATUS[n] if isinstance(n, str) else int(n))
    return m


def selected(status_map, mask):
    """bool [H, W]: the cell's status (& 7) is selected by bit s of ``mask``."""
    s = np.asarray(status_map).astype(np.int64) & 7
    return ((int(mask) >> s) & 1).astype(bool)


def dist2(status_map, mask, max_d2=0):
    """int32 [H, W]: min over the selected cells of the squared distance; FAR with none; min(., max_d2) with max_d2 > 0."""
    src = selected(status_map, mask)
    H, W = src.shape
    out = np.full((H, W), FAR, dtype=np.int64)
    if src.any():
        out[src] = 0
        pad = np.pad(src, 1, constant_values=True)
        inner = pad[:-2, 1:-1] & pad[2:, 1:-1] & pad[1:-1, :-2] & pad[1:-1, 2:]
        sy, sx = np.nonzero(src & ~inner)
        ty, tx = np.nonzero(~src)
        step = max(1, CHUNK // max(1, len(sy)))
        for c in range(0, len(ty), step):
            y, x = ty[c:c + step, None].astype(np.int64), tx[c:c + step, None].astype(np.int64)
            out[ty[c:c + step], tx[c:c + step]] = ((y - sy[None, :]) ** 2 + (x - sx[None, :]) ** 2).min(axis=1)
    if max_d2 > 0:
        out = np.minimum(out, int(max_d2))
    assert out.max() <= FAR
    return out.astype(np.int32)


def dist2_all_candidates(status_map, mask):
    """The same minimum without the two cuts (every selected cell a candidate for every cell): small maps only."""
    src = selected(status_map, mask)
    H, W = src.shape
    if not src.any():
        return np.full((H, W), FAR, dtype=np.int32)
    sy, sx = np.nonzero(src)
    y, x = np.mgrid[0:H, 0:W]
    d = (y.reshape(-1, 1).astype(np.int64) - sy[None, :]) ** 2 + (x.reshape(-1, 1).astype(np.int64) - sx[None, :]) ** 2
    return d.min(axis=1).reshape(H, W).astype(np.int32)


def as_float(v, scale=1.0):
    """SF_DIST_F32 of int32 values: double sqrt, double divide, one rounding to float32."""
    return (np.sqrt(np.asarray(v).astype(np.float64)) / scale).astype(np.float32)


def at_points(plane, points):
    """int32 [k]: ``plane`` [H, W] gathered at ``points`` [k, 3] = (column, row, id); -1 for id <= 0 or a cell off the grid."""
    H, W = plane.shape
    p = np.asarray(points).astype(np.int64)
    ok = (p[:, 2] > 0) & (p[:, 0] >= 0) & (p[:, 0] < W) & (p[:, 1] >= 0) & (p[:, 1] < H)
    out = np.full(len(p), -1, dtype=np.int32)
    out[ok] = plane[p[ok, 1], p[ok, 0]]
    return out


def points_as_float(vals, scale=1.0):
    """SF_DIST_F32 of gathered values: -1 stays -1.0."""
    v = np.asarray(vals)
    out = np.full(v.shape, -1.0, dtype=np.float32)
    out[v >= 0] = as_float(v[v >= 0], scale)
    return out
