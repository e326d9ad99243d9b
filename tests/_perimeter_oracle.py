"""The yardstick of ``sf_perimeter``: a tracer of directed crack edges on the lattice of cell corners, all
integers, written from the definition in include/simfire_hip.h and independent of the kernels (no ranks, no doubling: it walks).

Cell (x = column, y = row) is the square [x, x + 1] x [y, y + 1], y down.  An edge leaves its tail vertex in direction d (0: +x,
1: +y, 2: -x, 3: -y) and exists iff its right cell is in S and its left cell is not.  ``answer`` checks itself on every call:
every edge lies in exactly one loop, the signed areas add up to |S|, and the number of edges equals the count of row and column
differences of the zero-padded mask.  ``components`` (scipy) counts loops and holes a second way for the CPU tests.
"""
import numpy as np

DX = (1, 0, -1, 0)
DY = (0, 1, 0, -1)
#: (right cell, left cell) of an edge relative to its tail, per direction
RIGHT = ((0, 0), (-1, 0), (-1, -1), (0, -1))
LEFT = ((0, -1), (0, 0), (-1, 0), (-1, -1))


def mask_of_status(fire_map, status_mask):
    """S of a status mask: bit s selects BurnStatus s."""
    m = np.asarray(fire_map).astype(np.int64) & 7
    return ((int(status_mask) >> m) & 1).astype(bool)


def mask_of_arrival(arrival, at_update):
    """S of a horizon: ``arrival`` as ``FireEngine.arrival`` gives it (-1 never)."""
    a = np.asarray(arrival)
    return (a >= 0) & (a <= int(at_update))


def edge_planes(S):
    """bool [4, H + 1, W + 1]: edge d at vertex (vx, vy)."""
    S = np.asarray(S, dtype=bool)
    H, W = S.shape
    P = np.zeros((H + 2, W + 2), dtype=bool)
    P[1:-1, 1:-1] = S

    def cell(dx, dy):                             # the cell (vx + dx, vy + dy) for every vertex
        return P[1 + dy:H + 2 + dy, 1 + dx:W + 2 + dx]
    return np.stack([cell(*RIGHT[d]) & ~cell(*LEFT[d]) for d in range(4)])


def cheap(S):
    """(edges, cells, front) without tracing."""
    S = np.asarray(S, dtype=bool)
    P = np.pad(S, 1)
    edges = int((P[1:] != P[:-1]).sum() + (P[:, 1:] != P[:, :-1]).sum())
    inner = P[:-2, 1:-1] & P[2:, 1:-1] & P[1:-1, :-2] & P[1:-1, 2:]
    return edges, int(S.sum()), (S & ~inner).astype(np.uint8)


def answer(S, connectivity, simplify=True):
    """Every output of ``sf_perimeter`` for one environment: dict(edges, cells, front, loops, holes, n_vertices, vertices [nv, 2] =
    (x, y), loop_start [loops + 1], loop_area [loops], loop_edges [loops]), int32 arrays."""
    S = np.asarray(S, dtype=bool)
    H, W = S.shape
    assert connectivity in (4, 8)
    E = edge_planes(S)
    P = np.pad(S, 1)

    def inside(x, y):
        return bool(P[y + 1, x + 1])
    n_edges, n_cells, front = cheap(S)
    assert int(E.sum()) == n_edges
    vy, vx, dd = np.nonzero(E.transpose(1, 2, 0))                    # sorted by (vy, vx, d): id order
    ids = ((vy * (W + 1) + vx) * 4 + dd).tolist()
    assert ids == sorted(ids)
    seen = set()
    verts, starts, areas, lens = [], [0], [], []
    for eid in ids:                                                   # a loop starts at its smallest-id edge
        if eid in seen:
            continue
        x, y, d = (eid >> 2) % (W + 1), (eid >> 2) // (W + 1), eid & 3
        loop = []
        cur = eid
        while True:
            assert cur not in seen, "an edge lies in two loops"
            seen.add(cur)
            loop.append((x, y, d))
            hx, hy = x + DX[d], y + DY[d]
            ar = inside(hx + RIGHT[d][0], hy + RIGHT[d][1])
            al = inside(hx + LEFT[d][0], hy + LEFT[d][1])
            if connectivity == 4:
                nd = d + 1 if not ar else (d if not al else d + 3)
            else:
                nd = d + 3 if al else (d if ar else d + 1)
            x, y, d = hx, hy, nd & 3
            assert E[d, y, x], "the successor is no edge"
            cur = (y * (W + 1) + x) * 4 + d
            if cur == eid:
                break
        m = len(loop)
        pts = np.array([(p[0], p[1]) for p in loop], dtype=np.int64)
        nxt = np.roll(pts, -1, axis=0)
        twice = int((pts[:, 0] * nxt[:, 1] - nxt[:, 0] * pts[:, 1]).sum())
        assert twice % 2 == 0 and twice != 0
        dirs = [p[2] for p in loop]
        corner = [dirs[k] != dirs[k - 1] for k in range(m)]
        assert corner[0], "the start vertex is no corner"
        keep = [k for k in range(m) if corner[k] or not simplify]
        verts.extend((loop[k][0], loop[k][1]) for k in keep)
        starts.append(len(verts))
        areas.append(twice // 2)
        lens.append(m)
    assert len(seen) == n_edges, "an edge lies in no loop"
    assert sum(areas) == n_cells
    return dict(edges=n_edges, cells=n_cells, front=front, loops=len(areas), holes=sum(1 for a in areas if a < 0), n_vertices=len(verts),
                vertices=np.array(verts, dtype=np.int32).reshape(-1, 2), loop_start=np.array(starts, dtype=np.int32),
                loop_area=np.array(areas, dtype=np.int32), loop_edges=np.array(lens, dtype=np.int32))


def components(S, connectivity):
    """(outer loops, holes) by ``scipy.ndimage.label``: the c-connected components of S, and the (12 - c)-connected components of
    the zero-padded complement minus the one outside."""
    from scipy import ndimage
    four = ndimage.generate_binary_structure(2, 1)
    eight = ndimage.generate_binary_structure(2, 2)
    S = np.asarray(S, dtype=bool)
    outer = ndimage.label(S, structure=eight if connectivity == 8 else four)[1]
    comp = ndimage.label(~np.pad(S, 1), structure=four if connectivity == 8 else eight)[1]
    return int(outer), int(comp) - 1
