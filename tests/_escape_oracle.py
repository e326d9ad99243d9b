"""The yardstick of ``sf_escape``: the escape slack as a max-min Dijkstra with a heap, in NumPy and pure
Python, written from the definition in include/simfire_hip.h and sharing nothing with the kernel's level sweep.

  D(c): NEVER if T < 0 or not T < horizon (T = float32 minutes[c]); else q = (float64(T) - margin) / per_move in float64 and
        D = ceil(q) if q > 0 else 0.  A walker may stand on c at move index m (now: 0) exactly when m < D(c).
  S(c): SAFE on targets; on walkable cells min(D(c) - 1, max_n S(n) - 1) over the target-or-walkable neighbours, with SAFE - 1 = SAFE,
        NEVER - 1 = SAFE, the maximum over nothing LOST; BLOCKED elsewhere.
  Points: SAFE on a target; else min(D(c) - 1, max_n S(n) - 1) with the point's own D(c) (a walkable point: the plane's value; a
        blocked one: as if it were walkable for itself alone); LOST if no neighbour has S >= 0 ... see ``points_of``.
  point_step (connectivity 4): where 0 <= point_slack < SAFE the move code n + 1 of the LOWEST-numbered neighbour n that attains
        max_n S(n); 0 on a target, when lost, when the slack is SAFE, and with connectivity 8; -1 where point_slack is -2.

``brute`` is the other reading of the definition - a search over the states (cell, move index) of a walker that may step or stay -
which ``self_test`` holds the Dijkstra against.
"""
import heapq

import numpy as np

SAFE, LOST, BLOCKED = 2 ** 31 - 1, -1, -2
NEVER = 2 ** 31 - 1
MAX_MOVES = 32768
# neighbour n of a cell: (d_row, d_column); 0..3 are the move codes 1..4 of the action word, 4..7 the diagonals
NEIGHBOURS = ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1))


def deadlines(minutes, per_move=1.0, margin=0.0, horizon=64.0):
    """int64 [H, W]: the deadline of every cell, NEVER where the fire does not close it within the horizon."""
    T = np.asarray(minutes, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        finite = ~(T < np.float32(0)) & (T.astype(np.float64) < np.float64(horizon))
        q = (T.astype(np.float64) - np.float64(margin)) / np.float64(per_move)
    D = np.full(T.shape, NEVER, dtype=np.int64)
    qf = q[finite]
    D[finite] = np.where(qf > 0, np.ceil(qf), 0).astype(np.int64)
    return D


def move_bound(per_move, margin, horizon):
    return int(np.ceil((np.float64(horizon) - np.float64(margin)) / np.float64(per_move)))


def cell_sets(fire_map, target_mask, through_mask, passable=None, targets=None, D=None, unreached_safe=False):
    """(target, walkable non-target) as bool [H, W]."""
    s = np.asarray(fire_map).astype(np.int64) & 7
    tgt = ((target_mask >> s) & 1).astype(bool)
    if targets is not None:
        tgt |= np.asarray(targets) != 0
    walk = ((through_mask >> s) & 1).astype(bool)
    if passable is not None:
        walk &= np.asarray(passable) != 0
    walk &= ~tgt
    if unreached_safe:
        never = walk & (D == NEVER)
        tgt |= never
        walk &= ~never
    return tgt, walk


def _dec(s):
    return SAFE if s == SAFE else s - 1


def slack_plane(tgt, walk, D, conn):
    """int64 [H, W]: max-min Dijkstra from the targets - a cell is settled with the largest slack any route gives it."""
    H, W = tgt.shape
    nn = NEIGHBOURS[:8 if conn == 8 else 4]
    S = np.full((H, W), BLOCKED, dtype=np.int64)
    S[walk] = LOST
    S[tgt] = SAFE
    Dl, walkl = D.tolist(), walk.tolist()
    best = S.tolist()
    heap = [(-SAFE, int(y), int(x)) for y, x in np.argwhere(tgt)]
    heapq.heapify(heap)
    while heap:
        neg, y, x = heapq.heappop(heap)
        s = -neg
        if s < best[y][x]:
            continue
        via = _dec(s)
        for dy, dx in nn:
            ny, nx = y + dy, x + dx
            if 0 <= ny < H and 0 <= nx < W and walkl[ny][nx]:
                own = SAFE if Dl[ny][nx] == NEVER else Dl[ny][nx] - 1
                cand = min(own, via)
                if cand >= 0 and cand > best[ny][nx]:
                    best[ny][nx] = cand
                    heapq.heappush(heap, (-cand, ny, nx))
    return np.array(best, dtype=np.int64)


def points_of(S, D, tgt, walk, pts, conn):
    """(point_slack, point_step) int32 [k] of points [k, 3] = (column, row, id)."""
    H, W = S.shape
    nn = NEIGHBOURS[:8 if conn == 8 else 4]
    val, step = [], []
    for x, y, pid in np.asarray(pts).tolist():
        if pid <= 0 or not (0 <= x < W and 0 <= y < H):
            val.append(BLOCKED)
            step.append(-1)
            continue
        if tgt[y, x]:
            val.append(SAFE)
            step.append(0)
            continue
        around = [(int(S[y + dy, x + dx]) if 0 <= y + dy < H and 0 <= x + dx < W and (tgt[y + dy, x + dx] or walk[y + dy, x + dx]) else None)
                  for dy, dx in nn]
        have = [s for s in around if s is not None]
        top = max(have) if have else LOST
        if top == LOST:
            val.append(LOST)
            step.append(0)
            continue
        own = SAFE if D[y, x] == NEVER else int(D[y, x]) - 1
        v = max(min(own, _dec(top)), LOST)
        val.append(v)
        step.append(around.index(top) + 1 if 0 <= v < SAFE and conn != 8 else 0)
    return np.array(val, dtype=np.int32), np.array(step, dtype=np.int32)


def answer(fire_map, minutes, target_mask, through_mask, conn=4, passable=None, targets=None, pts=None, per_move=1.0, margin=0.0,
           horizon=64.0, unreached_safe=False):
    """Every output of ``sf_escape`` for one environment."""
    D = deadlines(minutes, per_move, margin, horizon)
    tgt, walk = cell_sets(fire_map, target_mask, through_mask, passable, targets, D, unreached_safe)
    S = slack_plane(tgt, walk, D, conn)
    finite = walk & (D != NEVER)
    out = dict(slack=S.astype(np.int32), safe=int((walk & (S == SAFE)).sum()), escapable=int((walk & (S >= 0) & (S < SAFE)).sum()),
               lost=int((walk & (S == LOST)).sum()), top=int(D[finite].max()) if finite.any() else 0)
    if pts is not None:
        out["point_slack"], out["point_step"] = points_of(S, D, tgt, walk, pts, conn)
    return out


# ---------------------------------------------------------------------------------------------- the other reading: states (cell, move)
def _grow(a, conn):
    """bool [H, W]: the cells with a neighbour in ``a``."""
    g = np.zeros_like(a)
    H, W = a.shape
    for dy, dx in NEIGHBOURS[:8 if conn == 8 else 4]:
        ys, yd = (slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0)))
        xs, xd = (slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0)))
        g[yd, xd] |= a[ys, xs]
    return g


def brute(tgt, walk, D, conn):
    """(S int64 [H, W], alive): ``alive[m]`` bool [H, W] for m = 0 .. M + 1 - a walker standing on the cell at move index m, who may
    step to a neighbour or stay, move by move, still gets to a target without ever standing on a cell c at an index >= D(c);
    ``alive[M + 1]`` stands for every later index (only NEVER cells can be stood on then).  S is SAFE where the last one holds, the
    largest alive index elsewhere, LOST if there is none."""
    finite = walk & (D != NEVER)
    M = int(D[finite].max()) if finite.any() else 0
    late = tgt.copy()                         # for ever: through NEVER cells only
    never = walk & (D == NEVER)
    while True:
        more = late | (never & _grow(late, conn))
        if (more == late).all():
            break
        late = more
    alive = [None] * (M + 2)
    alive[M + 1] = late
    for m in range(M, -1, -1):
        nxt = alive[m + 1]
        alive[m] = tgt | (walk & (D > m) & (nxt | _grow(nxt, conn)))
    S = np.full(tgt.shape, BLOCKED, dtype=np.int64)
    S[walk] = LOST
    for m in range(M + 1):
        S[walk & alive[m]] = m
    S[late] = SAFE
    return S, alive


def brute_point(alive, D, tgt, walk, x, y, conn):
    """The point rule read off the states: the largest index at which a walker may still stand on (x, y) - its own deadline - with a
    neighbour that is alive one move later."""
    H, W = tgt.shape
    if tgt[y, x]:
        return SAFE
    M = len(alive) - 2
    nb = [(y + dy, x + dx) for dy, dx in NEIGHBOURS[:8 if conn == 8 else 4]
          if 0 <= y + dy < H and 0 <= x + dx < W and (tgt[y + dy, x + dx] or walk[y + dy, x + dx])]
    if D[y, x] == NEVER and any(alive[M + 1][c] for c in nb):
        return SAFE
    for w in range(min(int(D[y, x]) - 1, M), -1, -1):
        if any(alive[w + 1][c] for c in nb):
            return w
    return LOST


def self_test(seed=3001, maps=24, H=12, W=14):
    """Random maps, both connectivities, three wall densities, with and without ``unreached_safe``: the Dijkstra equals the search
    over states on the plane, and the point rule equals it on every cell.  Returns the number of cells compared."""
    rng = np.random.default_rng(seed)
    seen = 0
    kinds = set()
    for i in range(maps):
        wall = (0.1, 0.3, 0.5)[i % 3]
        conn = (4, 8)[(i // 3) % 2]
        flag = bool((i // 6) % 2)
        u = rng.random((H, W))
        m = np.where(u < wall, 3, 0).astype(np.uint8)
        m[rng.integers(0, H), rng.integers(0, W)] = 2
        if i % 4 == 0:
            m[rng.integers(0, H), rng.integers(0, W)] = 2
        mins = rng.integers(0, 20, size=(H, W)).astype(np.float32)
        mins[rng.random((H, W)) < 0.25] = np.inf
        mins[rng.random((H, W)) < 0.05] = -1.0
        D = deadlines(mins, 1.0, 0.0, 64.0)
        tgt, walk = cell_sets(m, 4, 1, None, None, D, flag)
        S = slack_plane(tgt, walk, D, conn)
        B, alive = brute(tgt, walk, D, conn)
        assert (S == B).all(), (i, conn, flag, np.argwhere(S != B)[:5].tolist())
        pts = np.array([(x, y, 1) for y in range(H) for x in range(W)], dtype=np.int32)
        val, step = points_of(S, D, tgt, walk, pts, conn)
        for (x, y, _), v, st in zip(pts.tolist(), val.tolist(), step.tolist()):
            assert v == brute_point(alive, D, tgt, walk, x, y, conn), (i, conn, flag, x, y, v)
            if tgt[y, x] or walk[y, x]:
                assert v == S[y, x], (i, x, y)
            if conn == 4 and 0 <= v < SAFE:
                dy, dx = NEIGHBOURS[st - 1]
                assert S[y + dy, x + dx] >= v + 1 or S[y + dy, x + dx] == SAFE       # the step raises the slack
            else:
                assert st == 0
        seen += H * W
        kinds.update(np.unique(np.clip(S, -2, 1)).tolist() + ([SAFE] if (S == SAFE).any() else []))
    assert {BLOCKED, LOST, 0, 1, SAFE} <= kinds, kinds
    return seen
