"""The worlds of ``tests/test_distance_gpu.py`` and the loops that drive them, on the cases of ``tests/_arrival_worlds.py``.  A handle
is anything with the older API (``reset``, ``step``, ``apply_mitigation``, ``fire_map``): the GPU test drives an engine and asks it for
distances at every query point; ``tests/test_distance_cpu.py`` drives ``_arrival_worlds.DenseStandIn`` through the same loops and
checks with ``_dist_oracle`` that the query points show what the GPU cases claim to cover (``seen``)."""
import numpy as np

import _arrival_worlds as aw
import _dist_oracle as do

CALLS = (1, 2, 3, 5, 7, 11)                       # updates per call; a query behind each
MASKS = (("BURNING",), ("BURNING", "BURNED"), ("UNBURNED",), ("FIRELINE", "SCRATCHLINE", "WETLINE"),
         ("UNBURNED", "BURNING", "BURNED", "FIRELINE", "SCRATCHLINE", "WETLINE"))
CAPS = (0, 1, 2, 25, 1000)                        # max_d2, 0 = none
EPISODE_CASES = ("24x40", "33x17", "70x1030_wide", "72x80_win", "136x64_team")
PAIRS = [(case, mode) for case in EPISODE_CASES for mode in aw.CASES[case]["modes"]]
EDGE_CASES = ("33x17", "70x1030_wide")
FIRELINE = 3


def queries(case, mode):
    """[(updates of the call, status names, max_d2)]: the masks cycle with the calls, the caps two at a time from an offset the mode
    picks, so that the modes of a case pair them differently and every mode meets every mask and every cap."""
    off = aw.CASES[case]["modes"].index(mode)
    return [(n, MASKS[i % len(MASKS)], CAPS[(2 * i + off) % len(CAPS)]) for i, n in enumerate(CALLS)]


def run_episode(case, mode, h, inits, on_query):
    """reset, then per call: ``h.step(n)`` and ``on_query(i, n, names, max_d2)``."""
    h.reset(inits)
    for i, (n, names, cap) in enumerate(queries(case, mode)):
        h.step(n)
        on_query(i, n, names, cap)


def border_rows(E, H, W):
    """Fire lines for ``apply_mitigation`` as rows (env, column, row, FIRELINE): environment 0 the four corners only, 1 the whole top
    and bottom rows, 2 the whole first and last columns, every further one pieces of all four borders."""
    rows = []
    for e in range(E):
        if e == 0:
            cells = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]
        elif e == 1:
            cells = [(x, 0) for x in range(W)] + [(x, H - 1) for x in range(W)]
        elif e == 2:
            cells = [(0, y) for y in range(H)] + [(W - 1, y) for y in range(H)]
        else:
            cells = [(x, 0) for x in range(0, W, 5)] + [(x, H - 1) for x in range(2, W, 7)] + [(0, y) for y in range(1, H, 4)] + \
                    [(W - 1, y) for y in range(3, H, 6)]
        rows += [(e, x, y, FIRELINE) for x, y in cells]
    return rows


def edge_scene(h, E, H, W, inits):
    """reset, two updates (a ``run`` mode then keeps the cells in its blocked plane), then the fire lines of ``border_rows``."""
    h.reset(inits)
    h.step(2)
    h.apply_mitigation(border_rows(E, H, W))


def lone_corner_map(H, W):
    """A fire map whose only BURNING cell is (H - 1, W - 1)."""
    m = np.zeros((H, W), dtype=np.uint8)
    m[H - 1, W - 1] = 1
    return m


def seen(status_map, names, max_d2):
    """What a query point shows, as a set of words (the claims of the GPU cases)."""
    src = do.selected(status_map, do.mask_of(names))
    d2 = do.dist2(status_map, do.mask_of(names))
    out = set()
    if not src.any():
        return {"empty set"}
    if src[0].any():
        out.add("source on row 0")
    if src[-1].any():
        out.add("source on row H-1")
    if src[:, 0].any():
        out.add("source in column 0")
    if src[:, -1].any():
        out.add("source in column W-1")
    if not src.any(axis=0).all():
        out.add("column with no source")
    if (d2 == 2).any():
        out.add("value of exactly 2")
    if max_d2 > 0 and (d2 > max_d2).any():
        out.add("value above the cap")
    if src.all():
        out.add("all selected")
    return out


CLAIMS = {"source on row 0", "source on row H-1", "source in column 0", "source in column W-1", "empty set", "value above the cap",
          "value of exactly 2", "column with no source"}
