"""The yardstick of the reach tests (``sf_reach``), NumPy only and independent of the library: the reach of the
seed cells through the open cells by plain repeated dilation to the fixed point, and its count, value and point answers."""
import numpy as np

NAMES = {"UNBURNED": 0, "BURNING": 1, "BURNED": 2, "FIRELINE": 3, "SCRATCHLINE": 4, "WETLINE": 5}
LINES = ("FIRELINE", "SCRATCHLINE", "WETLINE")


def mask_of(names):
    """Names or ints -> the mask (bit s = BurnStatus s)."""
    m = 0
    for s in names:
        m |= 1 << (NAMES[s] if isinstance(s, str) else int(s))
    return m


def selected(status_map, mask):
    """bool [H, W]: cells whose status & 7 the mask selects."""
    s = np.asarray(status_map).astype(np.int64) & 7
    return ((mask >> s) & 1).astype(bool)


def dilate(a, connectivity):
    """bool [H, W]: the cells with a neighbour in ``a`` (4- or 8-neighbourhood; the cell itself does not count)."""
    H, W = a.shape
    p = np.zeros((H + 2, W + 2), dtype=bool)
    p[1:-1, 1:-1] = a
    out = p[:-2, 1:-1] | p[2:, 1:-1] | p[1:-1, :-2] | p[1:-1, 2:]
    if connectivity == 8:
        out = out | p[:-2, :-2] | p[:-2, 2:] | p[2:, :-2] | p[2:, 2:]
    return out


def reach(status_map, source_mask, through_mask, connectivity, passable=None):
    """bool [H, W]: the smallest set R with c in R iff open(c) and a neighbour of c is a seed or in R."""
    assert connectivity in (4, 8) and not source_mask & through_mask
    seed = selected(status_map, source_mask)
    open_ = selected(status_map, through_mask)
    if passable is not None:
        open_ = open_ & (np.asarray(passable) != 0)
    r = np.zeros_like(seed)
    while True:
        nxt = r | (dilate(seed | r, connectivity) & open_)
        if (nxt == r).all():
            return r
        r = nxt


def first_round(status_map, source_mask, through_mask, connectivity, passable=None):
    """bool [H, W]: the open neighbours of the seeds (what any first round must have reached)."""
    open_ = selected(status_map, through_mask)
    if passable is not None:
        open_ = open_ & (np.asarray(passable) != 0)
    return dilate(selected(status_map, source_mask), connectivity) & open_


def count(r):
    return int(r.sum())


def seeds(status_map, source_mask):
    return int(selected(status_map, source_mask).sum())


def value(r, values):
    """The value plane (int [H, W]) summed over the reach, as a Python int."""
    return int(np.asarray(values, dtype=np.int64)[r].sum())


def point_in(r, pts):
    """pts int [k, 3] = (column, row, id) -> int32 [k]: 1 / 0, -1 for id <= 0 or a cell off the grid."""
    H, W = r.shape
    out = np.full(len(pts), -1, dtype=np.int32)
    for j, (x, y, i) in enumerate(np.asarray(pts).tolist()):
        if i > 0 and 0 <= x < W and 0 <= y < H:
            out[j] = int(r[y, x])
    return out
