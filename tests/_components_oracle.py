"""The yardstick of ``sf_components``, written independently of the kernel's method: a breadth-first fill from
every selected cell that has no number yet, in row-major order, so component j + 1 is the one whose first cell comes j-th.  Plain
NumPy and a queue; ``tests/test_components_cpu.py`` checks it against ``scipy.ndimage.label`` on random maps and on every scene."""
from collections import deque

import numpy as np

STATUS = {"UNBURNED": 0, "BURNING": 1, "BURNED": 2, "FIRELINE": 3, "SCRATCHLINE": 4, "WETLINE": 5}
BORDER = 64
N4 = ((-1, 0), (0, -1), (0, 1), (1, 0))
N8 = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))


def mask_of(names):
    if isinstance(names, (int, np.integer)):
        return int(names)
    m = 0
    for s in names:
        m |= 1 << (STATUS[s] if isinstance(s, str) else int(s))
    return m


def selected(fire_map, select_mask, member=None):
    """bool [H, W]: bit status & 7 of the mask, and ``member`` not 0."""
    s = np.asarray(fire_map).astype(np.int64) & 7
    sel = ((int(select_mask) >> s) & 1).astype(bool)
    if member is not None:
        sel &= np.asarray(member) != 0
    return sel


def label(sel, conn):
    """(int32 labels [H, W], C): the fill.  A border of False around the plane spares the bounds checks."""
    H, W = sel.shape
    P = W + 2
    pad = np.zeros((H + 2, P), dtype=bool)
    pad[1:-1, 1:-1] = sel
    free = pad.ravel().tolist()
    lab = [0] * len(free)
    offs = [dy * P + dx for dy, dx in (N8 if conn == 8 else N4)]
    c = 0
    for start in np.flatnonzero(pad.ravel()).tolist():         # ascending: row-major
        if not free[start]:
            continue
        c += 1
        free[start] = False
        lab[start] = c
        q = deque((start,))
        while q:
            at = q.popleft()
            for o in offs:
                nb = at + o
                if free[nb]:
                    free[nb] = False
                    lab[nb] = c
                    q.append(nb)
    return np.asarray(lab, dtype=np.int32).reshape(H + 2, P)[1:-1, 1:-1].copy(), c


def components(fire_map, select_mask, conn, member=None, values=None, cap=64, points=None):
    """Every output of ``sf_components`` for one environment, as NumPy arrays of the library's dtypes."""
    fire_map = np.asarray(fire_map)
    H, W = fire_map.shape
    sel = selected(fire_map, select_mask, member)
    lab, C = label(sel, conn)
    sizes = np.bincount(lab.ravel(), minlength=C + 1)[1:].astype(np.int64)
    ys, xs = np.nonzero(sel)
    ids = lab[ys, xs] - 1
    flat = ys * W + xs
    first = np.full(max(C, 1), H * W, dtype=np.int64)
    np.minimum.at(first, ids, flat)
    box = np.empty((max(C, 1), 4), dtype=np.int64)
    box[:, :2], box[:, 2:] = max(H, W), -1
    np.minimum.at(box[:, 0], ids, xs); np.minimum.at(box[:, 1], ids, ys)
    np.maximum.at(box[:, 2], ids, xs); np.maximum.at(box[:, 3], ids, ys)
    touch = np.zeros(max(C, 1), dtype=np.int64)
    status = fire_map.astype(np.int64) & 7
    for dy, dx in (N8 if conn == 8 else N4):
        ny, nx = ys + dy, xs + dx
        on = (ny >= 0) & (ny < H) & (nx >= 0) & (nx < W)
        ny, nx, who = ny[on], nx[on], ids[on]
        out = ~sel[ny, nx] & (status[ny, nx] < 6)
        np.bitwise_or.at(touch, who[out], 1 << status[ny[out], nx[out]])
    edge = (ys == 0) | (ys == H - 1) | (xs == 0) | (xs == W - 1)
    np.bitwise_or.at(touch, ids[edge], BORDER)
    val = np.zeros(max(C, 1), dtype=np.int64)
    if values is not None:
        np.add.at(val, ids, np.asarray(values).astype(np.int64)[ys, xs])
    n = min(C, cap)
    r = dict(count=np.int32(C), selected=np.int32(sel.sum()), labels=lab,
             cells=np.zeros(cap, dtype=np.int32), value=np.zeros(cap, dtype=np.int64), first=np.full(cap, -1, dtype=np.int32),
             bbox=np.full((cap, 4), -1, dtype=np.int32), touch=np.zeros(cap, dtype=np.int32), largest=np.zeros(2, dtype=np.int32))
    r["cells"][:n], r["value"][:n], r["first"][:n], r["bbox"][:n], r["touch"][:n] = sizes[:n], val[:n], first[:n], box[:n], touch[:n]
    if C:
        big = int(np.argmax(sizes))                            # (the first of equal sizes: the lower number)
        r["largest"][:] = (big + 1, sizes[big])
    if points is not None:
        pts = np.asarray(points)
        pl = np.full(len(pts), -1, dtype=np.int32)
        for j, (x, y, pid) in enumerate(pts.tolist()):
            if pid > 0 and 0 <= x < W and 0 <= y < H:
                pl[j] = lab[y, x]
        r["point_label"] = pl
    return r
