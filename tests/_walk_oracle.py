"""Walking distance straight from the definition (``sf_walk``): level-by-level dilation in NumPy.

``d = 0`` on targets; a walkable cell gets level L when a 4- (8-) neighbour that is a target or walkable has level L - 1 - so every
level is one dilation of the cells reached so far, cut to the walkable cells.  The point rule and the tie rule of ``point_step`` are
written out per point.  Slow on purpose (a corridor costs a dilation per cell): the tests keep their paths short."""
import numpy as np

from _reach_oracle import mask_of, selected  # noqa: F401

FAR, BLOCKED = 2 ** 31 - 1, -1
MOVES = ((-1, 0), (1, 0), (0, -1), (0, 1))              # (d_row, d_column) of move codes 1..4
DIAGONALS = ((-1, -1), (-1, 1), (1, -1), (1, 1))


def _dilate(a, conn):
    out = a.copy()
    out[1:, :] |= a[:-1, :]
    out[:-1, :] |= a[1:, :]
    out[:, 1:] |= a[:, :-1]
    out[:, :-1] |= a[:, 1:]
    if conn == 8:
        out[1:, 1:] |= a[:-1, :-1]
        out[1:, :-1] |= a[:-1, 1:]
        out[:-1, 1:] |= a[1:, :-1]
        out[:-1, :-1] |= a[1:, 1:]
    return out


def cells(m, target_mask, through_mask, passable=None, targets=None):
    """(target, walk) as bool planes: ``target_mask`` / ``through_mask`` select status bytes & 7; ``targets`` adds cells, ``passable``
    removes walkable ones."""
    tgt = selected(m, target_mask) if target_mask else np.zeros(m.shape, dtype=bool)
    if targets is not None:
        tgt = tgt | (np.asarray(targets) != 0)
    walk = selected(m, through_mask)
    if passable is not None:
        walk = walk & (np.asarray(passable) != 0)
    return tgt, walk


def true_moves(m, target_mask, through_mask, conn=4, passable=None, targets=None):
    """(d, levels) without a cap: int64 [H, W] with FAR / BLOCKED, and the largest finite value."""
    tgt, walk = cells(m, target_mask, through_mask, passable, targets)
    d = np.where(tgt, 0, np.where(walk, FAR, BLOCKED)).astype(np.int64)
    reached = tgt.copy()
    front = tgt
    todo = walk & ~tgt
    L = 0
    while True:
        front = _dilate(front, conn or 4) & todo
        if not front.any():
            break
        L += 1
        d[front] = L
        todo = todo & ~front
        reached |= front
    return d, L


def moves(m, target_mask, through_mask, conn=4, passable=None, targets=None, max_moves=0):
    """The plane form, int32 [H, W]: every value above ``max_moves`` (FAR included) becomes ``max_moves``."""
    d, _ = true_moves(m, target_mask, through_mask, conn, passable, targets)
    if max_moves:
        d = np.where(d > max_moves, max_moves, d)
    return d.astype(np.int32)


def reached(m, target_mask, through_mask, conn=4, passable=None, targets=None, max_moves=0):
    d, _ = true_moves(m, target_mask, through_mask, conn, passable, targets)
    return int(((d > 0) & (d <= (max_moves or FAR - 1))).sum())


def levels(m, target_mask, through_mask, conn=4, passable=None, targets=None, max_moves=0):
    L = true_moves(m, target_mask, through_mask, conn, passable, targets)[1]
    return min(L, max_moves) if max_moves else L


def points(m, pts, target_mask, through_mask, conn=4, passable=None, targets=None, max_moves=0):
    return points_of(true_moves(m, target_mask, through_mask, conn, passable, targets)[0], pts, conn, max_moves)


def answer(m, target_mask, through_mask, conn=4, passable=None, targets=None, pts=None, max_moves=0):
    """Every output from one search: dict(moves, reached, levels[, point_moves, point_step])."""
    d, L = true_moves(m, target_mask, through_mask, conn, passable, targets)
    out = dict(moves=(np.where(d > max_moves, max_moves, d) if max_moves else d).astype(np.int32),
               reached=int(((d > 0) & (d <= (max_moves or FAR - 1))).sum()), levels=min(L, max_moves) if max_moves else L)
    if pts is not None:
        out["point_moves"], out["point_step"] = points_of(d, pts, conn, max_moves)
    return out


def points_of(d, pts, conn=4, max_moves=0):
    """(point_moves, point_step) int32 [k] for ``pts`` [k, 3] = (column, row, id).  The walker may stand on any cell; its value is 0
    on a target, else 1 + the least value of a target or walkable neighbour; its step is the lowest move code that attains it (only
    the four moves are steps; with connectivity 8 the step is reported as 0).  ``d``: the plane of ``true_moves``."""
    H, W = d.shape
    pm, ps = [], []
    for x, y, ident in np.asarray(pts).tolist():
        if ident <= 0 or not (0 <= x < W and 0 <= y < H):
            pm.append(-1)
            ps.append(-1)
            continue
        if d[y, x] == 0:
            pm.append(0)
            ps.append(0)
            continue
        best, step = FAR, 0
        for code, (dy, dx) in enumerate(MOVES + (DIAGONALS if conn == 8 else ()), start=1):
            ny, nx = y + dy, x + dx
            if 0 <= ny < H and 0 <= nx < W and 0 <= d[ny, nx] < FAR and d[ny, nx] + 1 < best:
                best, step = int(d[ny, nx]) + 1, code
        if conn == 8:
            step = 0
        if max_moves and best > max_moves:
            best, step = max_moves, 0
        pm.append(best)
        ps.append(step)
    return np.array(pm, dtype=np.int32), np.array(ps, dtype=np.int32)
