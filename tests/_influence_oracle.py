"""The yardstick of ``sf_influence``, straight from the definition: the codes sanitised, then from every cell a
walk up its parent chain that credits each ancestor, with a visited set for cycles.  ``answer_peel`` restates the sums by peeling
leaves (linear time; what the tests of large grids use, held against ``answer`` by the self-test); ``history_codes`` is the rule that
turns parent masks and arrivals into the ignition tree, ``points`` the point and route rule.  Pure Python / NumPy, no device."""
import numpy as np

SRC_OFFSETS = ((+1, +1), (0, +1), (-1, +1), (+1, 0), (-1, 0), (+1, -1), (0, -1), (-1, -1))      # (dx, dy): travel.SRC_OFFSETS
GRAPH_OFFSETS = ((+1, 0), (+1, +1), (0, +1), (-1, +1), (-1, 0), (-1, -1), (0, -1), (+1, -1))    # graph.py:125-134, bit j of a parent mask
CYCLE = -2


def sanitise(pred):
    """int8 [H, W]: the code where it is 0..7 and the neighbour it names is on the grid, else -1."""
    pred = np.asarray(pred).astype(np.int64)
    H, W = pred.shape
    ok = (pred >= 0) & (pred <= 7)
    off = np.array(SRC_OFFSETS)[np.where(ok, pred, 0)]
    y, x = np.mgrid[0:H, 0:W]
    nx, ny = x + off[..., 0], y + off[..., 1]
    ok &= (nx >= 0) & (nx < W) & (ny >= 0) & (ny < H)
    return np.where(ok, pred, -1).astype(np.int8)


def parents(codes):
    """Flat parent index per flat cell, -1 without one (``codes`` sanitised)."""
    H, W = codes.shape
    c = codes.ravel().astype(np.int64)
    off = np.array(SRC_OFFSETS)[np.where(c >= 0, c, 0)]
    return np.where(c >= 0, np.arange(H * W) + off[:, 1] * W + off[:, 0], -1)


def _weights(n, include, weights):
    w1 = np.ones(n, dtype=np.int64) if include is None else (np.asarray(include).ravel() != 0).astype(np.int64)
    wv = None if weights is None else np.asarray(weights).ravel().astype(np.int64) * w1
    return w1, wv


def _counts(codes, par, cyc):
    has_child = np.zeros(par.size, dtype=bool)
    has_child[par[par >= 0]] = True
    return dict(forest=int((par >= 0).sum()), roots=int(((par < 0) & has_child).sum()), cyclic=int(cyc.sum()))


def _finish(codes, par, cells, value, cyc, w1, wv, inclusive):
    H, W = codes.shape
    if inclusive:
        cells = cells + w1
        value = None if value is None else value + wv
    cells[cyc] = CYCLE
    out = dict(cells=cells.reshape(H, W).astype(np.int32), pred=codes, **_counts(codes, par, cyc))
    if value is not None:
        value[cyc] = 0
        out["value"] = value.reshape(H, W).astype(np.int64)
    return out


def answer(pred, include=None, weights=None, inclusive=False):
    """The definition: dict(cells int32 [H, W], value int64 [H, W] with weights, pred int8 [H, W], forest, roots, cyclic)."""
    codes = sanitise(pred)
    par = parents(codes)
    n = par.size
    w1, wv = _weights(n, include, weights)
    cells = [0] * n
    value = [0] * n
    cyc = np.zeros(n, dtype=bool)
    for d in range(n):
        seen = {d}
        a = int(par[d])
        while a >= 0 and a not in seen:              # every ancestor of d, once
            seen.add(a)
            cells[a] += int(w1[d])
            if wv is not None:
                value[a] += int(wv[d])
            a = int(par[a])
        if a == d:                                   # the chain came back to d: d lies on a cycle
            cyc[d] = True
    return _finish(codes, par, np.array(cells, dtype=np.int64), None if wv is None else np.array(value, dtype=np.int64), cyc, w1, wv, inclusive)


def answer_peel(pred, include=None, weights=None, inclusive=False):
    """The same answer by peeling leaves: a cell is done when all its children are; what is never done lies on a cycle."""
    codes = sanitise(pred)
    par = parents(codes)
    n = par.size
    w1, wv = _weights(n, include, weights)
    left = np.bincount(par[par >= 0], minlength=n).tolist()
    parl, w1l = par.tolist(), w1.tolist()
    wvl = None if wv is None else wv.tolist()
    cells, value = [0] * n, [0] * n
    todo = [c for c in range(n) if left[c] == 0 and parl[c] >= 0]
    while todo:
        c = todo.pop()
        p = parl[c]
        cells[p] += cells[c] + w1l[c]
        if wvl is not None:
            value[p] += value[c] + wvl[c]
        left[p] -= 1
        if left[p] == 0 and parl[p] >= 0:
            todo.append(p)
    cyc = np.array(left) > 0
    return _finish(codes, par, np.array(cells, dtype=np.int64), None if wv is None else np.array(value, dtype=np.int64), cyc, w1, wv, inclusive)


def history_codes(masks, arrival):
    """int8 [H, W]: the ignition tree.  ``masks``: uint8 parent masks (bit j = neighbour ``GRAPH_OFFSETS[j]``), ``arrival``: int32, -1 =
    never.  A cell that never burned has no parent; else the candidates are the neighbours its mask names that are on the grid and
    burned strictly earlier; the newest wins, ties go to the lowest code; none is a root."""
    masks, arrival = np.asarray(masks), np.asarray(arrival)
    H, W = arrival.shape
    out = np.full((H, W), -1, dtype=np.int8)
    for y in range(H):
        for x in range(W):
            a = int(arrival[y, x])
            if a < 0:
                continue
            best, best_a = -1, -1
            for code, (dx, dy) in enumerate(SRC_OFFSETS):
                j = GRAPH_OFFSETS.index((dx, dy))
                nx, ny = x + dx, y + dy
                if not (int(masks[y, x]) >> j) & 1 or not (0 <= nx < W and 0 <= ny < H):
                    continue
                an = int(arrival[ny, nx])
                if 0 <= an < a and an > best_a:
                    best, best_a = code, an
            out[y, x] = best
    return out


def points(ans, pts, max_route=0):
    """The point rule on an answer: dict(point_cells [k], point_value [k] where the answer has a value, point_route [k, R] and
    point_hops [k] with ``max_route`` = R > 0).  ``pts``: int [k, 3] = (column, row, id)."""
    codes = ans["pred"]
    H, W = codes.shape
    k, R = len(pts), int(max_route)
    pc = np.full(k, -1, dtype=np.int32)
    pv = np.zeros(k, dtype=np.int64)
    route = np.full((k, R), -1, dtype=np.int32)
    hops = np.full(k, -1, dtype=np.int32)
    for j, (x, y, ident) in enumerate(np.asarray(pts).tolist()):
        if ident <= 0 or not (0 <= x < W and 0 <= y < H):
            continue
        pc[j] = ans["cells"][y, x]
        if "value" in ans:
            pv[j] = ans["value"][y, x]
        if R:
            r = 0
            while True:
                route[j, r] = y * W + x
                r += 1
                c = int(codes[y, x])
                if c < 0:
                    hops[j] = r - 1
                    break
                if r == R:
                    hops[j] = -2
                    break
                x, y = x + SRC_OFFSETS[c][0], y + SRC_OFFSETS[c][1]
    out = dict(point_cells=pc)
    if "value" in ans:
        out["point_value"] = pv
    if R:
        out.update(point_route=route, point_hops=hops)
    return out


def masks_from_edges(edges, H, W):
    """uint8 [H, W] parent masks from graph edges (source x, source y, x, y), as ``FireSpreadGraph`` holds them."""
    m = np.zeros((H, W), dtype=np.uint8)
    for sx, sy, x, y in np.asarray(edges).tolist():
        m[y, x] |= 1 << GRAPH_OFFSETS.index((sx - x, sy - y))
    return m


def dag_descendants(edges, H, W):
    """int64 [H, W]: the number of cells reachable from each cell over the graph's edges, the cell itself not counted
    (``len(nx.descendants(...))``) - a plain depth-first search per cell."""
    kids = {}
    for sx, sy, x, y in np.asarray(edges).tolist():
        kids.setdefault(sy * W + sx, []).append(y * W + x)
    out = np.zeros(H * W, dtype=np.int64)
    for c in kids:
        seen, stack = {c}, [c]
        while stack:
            for d in kids.get(stack.pop(), ()):
                if d not in seen:
                    seen.add(d)
                    stack.append(d)
        out[c] = len(seen) - 1
    return out.reshape(H, W)
