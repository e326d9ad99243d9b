"""Fire travel time straight from the definition (``sf_travel``): a float32 heap Dijkstra.

``T = 0`` on sources; on a passable cell ``T(c) = min_k float32(T(c + SRC_OFFSETS[k]) + w_k(c))`` over the on-grid neighbours that are
source or passable, with ``w_k(c) = float32(float64(pixel_scale) / float64(rt[k][c]))`` (+inf where ``rt[k][c]`` is not > 0).  Every
dtype is spelled out: a sum is ONE ``np.float32 + np.float32``.  float32 addition is monotone and the weights are >= 0, so the greatest
solution is unique, Dijkstra settles it and any order of relaxations reaches the same bits (``relax_to_fixpoint``, which the self-test
of ``tests/test_travel_cpu.py`` holds against the heap).  ``pred``, the point rule, the cap and the summary are written out below."""
import heapq

import numpy as np

from _reach_oracle import mask_of, selected  # noqa: F401

BLOCKED = np.float32(-1.0)
INF = np.float32(np.inf)
SRC_OFFSETS = ((+1, +1), (0, +1), (-1, +1), (+1, 0), (-1, 0), (+1, -1), (0, -1), (-1, -1))      # (dx, dy): the fire comes from c + offset
DIAGONAL = tuple(ox != 0 and oy != 0 for ox, oy in SRC_OFFSETS)


def cells(m, source_mask, through_mask, passable=None, sources=None):
    """(source, open) as bool planes, open = passable and not a source: ``source_mask`` / ``through_mask`` select status bytes & 7;
    ``sources`` adds source cells, ``passable`` removes passable ones.  A cell that is both is a source."""
    src = selected(m, source_mask) if source_mask else np.zeros(m.shape, dtype=bool)
    if sources is not None:
        src = src | (np.asarray(sources) != 0)
    pas = selected(m, through_mask)
    if passable is not None:
        pas = pas & (np.asarray(passable) != 0)
    return src, pas & ~src


def weights(R8, pixel_scale, conn=8):
    """float32 [8, H, W]: the division in float64, rounded once; +inf where the rate is not > 0 and, with ``conn`` 4, on diagonals."""
    R8 = np.asarray(R8, dtype=np.float64)
    w = np.full(R8.shape, np.inf, dtype=np.float32)
    ok = R8 > 0.0
    with np.errstate(over="ignore"):
        w[ok] = (np.float64(pixel_scale) / R8[ok]).astype(np.float32)
    if conn == 4:
        for k in range(8):
            if DIAGONAL[k]:
                w[k] = INF
    return w


def dijkstra(src, opn, w, max_minutes=0.0):
    """float32 [H, W]: T on source and open cells (+inf: no route, or none within the cap), undefined elsewhere (+inf)."""
    H, W = src.shape
    T = np.full((H, W), INF, dtype=np.float32)
    T[src] = np.float32(0.0)
    cap = np.float32(max_minutes)
    heap = [(0.0, int(y), int(x)) for y, x in np.argwhere(src)]
    heapq.heapify(heap)
    done = np.zeros((H, W), dtype=bool)
    while heap:
        d, y, x = heapq.heappop(heap)
        if done[y, x]:
            continue
        done[y, x] = True
        d32 = np.float32(d)                            # (exact: d came from a float32)
        for k, (ox, oy) in enumerate(SRC_OFFSETS):
            cy, cx = y - oy, x - ox                    # the cell whose neighbour k is (y, x)
            if not (0 <= cy < H and 0 <= cx < W) or not opn[cy, cx] or done[cy, cx]:
                continue
            c = d32 + w[k, cy, cx]                     # np.float32 + np.float32
            assert c.dtype == np.float32
            if cap > 0 and c > cap:
                continue
            if c < T[cy, cx]:
                T[cy, cx] = c
                heapq.heappush(heap, (float(c), cy, cx))
    return T


def _neighbour(a, k, fill):
    """``a`` of the neighbour c + SRC_OFFSETS[k] of every cell c (``fill`` past the grid)."""
    ox, oy = SRC_OFFSETS[k]
    H, W = a.shape
    out = np.full((H, W), fill, dtype=a.dtype)
    ys, yd = (slice(oy, H), slice(0, H - oy)) if oy >= 0 else (slice(0, H + oy), slice(-oy, H))
    xs, xd = (slice(ox, W), slice(0, W - ox)) if ox >= 0 else (slice(0, W + ox), slice(-ox, W))
    out[yd, xd] = a[ys, xs]
    return out


def relax_to_fixpoint(src, opn, w, max_minutes=0.0, order=None):
    """The same plane by relaxation: whole-grid sweeps (Jacobi) or, with ``order`` (a Generator), sweeps that update a random half of
    the cells only - a chaotic order.  Ends when a full sweep changes nothing."""
    T = np.where(src, np.float32(0.0), INF).astype(np.float32)
    cap = np.float32(max_minutes)
    ok = src | opn
    while True:
        Tn = np.where(ok, T, INF)
        best = T.copy()
        for k in range(8):
            c = _neighbour(Tn, k, INF) + w[k]
            assert c.dtype == np.float32
            if cap > 0:
                c = np.where(c > cap, INF, c)
            best = np.minimum(best, c)
        better = opn & (best < T)
        if not better.any():
            return T
        if order is not None:
            part = better & (order.random(T.shape) < 0.5)
            better = part if part.any() else better
        T = np.where(better, best, T)


def pred_of(T, src, opn, w):
    """int8 [H, W]: on open cells with a finite T the lowest k with float32(T(n_k) + w_k) == T, else -1."""
    Tn = np.where(src | opn, T, INF)
    p = np.full(T.shape, -1, dtype=np.int8)
    want = opn & np.isfinite(T)
    for k in range(7, -1, -1):
        hit = want & ((_neighbour(Tn, k, INF) + w[k]) == T)
        p[hit] = k
    assert (p[want] >= 0).all()
    return p


def points_of(T, src, opn, w, pts, max_minutes=0.0):
    """float32 [k] for ``pts`` [k, 3] = (column, row, id): T on a source or open cell; on any other cell the least
    float32(T(n_k) + w_k) over its source or open neighbours (+inf: none); capped; -1 for id <= 0 or off the grid."""
    H, W = T.shape
    cap = np.float32(max_minutes)
    out = []
    for x, y, ident in np.asarray(pts).tolist():
        if ident <= 0 or not (0 <= x < W and 0 <= y < H):
            out.append(np.float32(-1.0))
            continue
        if src[y, x] or opn[y, x]:
            v = T[y, x]
        else:
            v = INF
            for k, (ox, oy) in enumerate(SRC_OFFSETS):
                ny, nx = y + oy, x + ox
                if 0 <= ny < H and 0 <= nx < W and (src[ny, nx] or opn[ny, nx]):
                    c = T[ny, nx] + w[k, y, x]
                    if c < v:
                        v = c
        if cap > 0 and not v <= cap:
            v = cap
        out.append(np.float32(v))
    return np.array(out, dtype=np.float32)


def answer(m, R8, pixel_scale, source_mask, through_mask, conn=8, passable=None, sources=None, pts=None, max_minutes=0.0):
    """Every output from one search: dict(minutes, pred, reached, last, T[, point_minutes]).  ``max_minutes`` is compared as the
    float32 it rounds to."""
    src, opn = cells(m, source_mask, through_mask, passable, sources)
    w = weights(R8, pixel_scale, conn)
    cap = np.float32(max_minutes)
    T = dijkstra(src, opn, w, cap)
    fin = opn & np.isfinite(T)
    shown = np.where(np.isinf(T), cap, T) if cap > 0 else T
    out = dict(minutes=np.where(src | opn, shown, BLOCKED).astype(np.float32), pred=pred_of(T, src, opn, w), reached=int(fin.sum()),
               last=np.float32(T[fin].max()) if fin.any() else np.float32(0.0), T=T)
    if pts is not None:
        out["point_minutes"] = points_of(T, src, opn, w, pts, cap)
    return out


def hops_of(pred):
    """int [H, W]: the additions on the route ``pred`` names from every cell that has a pred to the cell where it ends (0 elsewhere).
    Raises if a route runs in a circle."""
    H, W = pred.shape
    hops = np.where(pred >= 0, -1, 0).astype(np.int64)
    for y0, x0 in np.argwhere(pred >= 0).tolist():
        chain, y, x = [], y0, x0
        while hops[y, x] < 0:
            chain.append((y, x))
            assert len(chain) <= H * W
            ox, oy = SRC_OFFSETS[pred[y, x]]
            y, x = y + oy, x + ox
        n = int(hops[y, x])
        for cy, cx in reversed(chain):
            n += 1
            hops[cy, cx] = n
    return hops
