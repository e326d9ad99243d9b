"""The cases of ``tests/test_values_gpu.py`` and the loop that drives them: the worlds, call lengths, modes and ops of
``tests/_arrival_worlds.py`` with a value plane on top.  Handle A is the reference: any engine with the older API, stepped ONE update
at a time with its maps fetched after each; ``tests/_arrival_oracle.MapArrival`` turns them into the expected arrival and
``tests/_values_oracle.damage`` sums the plane over it.  Handle B carries the value plane in the mode under test and makes the same
updates in calls of uneven length.  ``tests/test_values_cpu.py`` runs the same loop with ``oracle/fire_dense`` standing in for A
and no B, to check that every case sees what it claims to cover."""
import numpy as np

from _arrival_oracle import BURNING, MapArrival
from _arrival_worlds import CASES, STEPS, DenseStandIn, make_world, mode_settings      # noqa: F401  (re-exported for the tests)
from _values_oracle import damage

# The arrival cases that are run with values, and what differs: ``per_env`` - a plane per environment; ``values_at`` - the index
# of the call behind which B gets its plane (the "late" case: recording is enabled by the case's own op, the plane two calls
# later, in the middle of the episode).  Every other case sets the plane right behind the reset.
VALUE_CASES = {
    "24x40": {}, "33x17": dict(per_env=True), "72x80_win": {}, "64x64_kwin": {}, "136x64_team": {}, "70x1030_wide": {},
    "24x40_md8": {}, "24x40_md1": {}, "24x40_lines": {}, "24x40_resets": {}, "72x80_resets": dict(per_env=True), "24x40_fork": {},
    "24x40_state": {}, "24x40_late": dict(values_at=6),
}
PAIRS = [(case, mode) for case in VALUE_CASES for mode in CASES[case]["modes"]]


def make_values(case, E, inits, seed_offset=0):
    """int32 [H, W] or [E, H, W] (``per_env``): mostly zero, a few rectangular towns of values 1 .. 1000 - the first around the
    ignition cell of environment 0, so that a reset's own contribution is not zero, the others anywhere - and a sprinkle of negative
    cells.  A function of the case's seed (``seed_offset``: another plane of the same kind, for the swap)."""
    c = CASES[case]
    H, W = c["H"], c["W"]
    rng = np.random.default_rng(c["seed"] + 2 + 1000 * seed_offset)
    n = E if VALUE_CASES[case].get("per_env") else 1
    out = np.zeros((n, H, W), dtype=np.int32)
    for p in range(n):
        x0, y0 = int(inits[p if n > 1 else 0][0]), int(inits[p if n > 1 else 0][1])
        boxes = [(max(0, x0 - 4), max(0, y0 - 4), min(W, x0 + 5), min(H, y0 + 5))]
        for _ in range(3):
            w, h = int(rng.integers(3, 9)), int(rng.integers(3, 9))
            x, y = int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1))
            boxes.append((x, y, x + w, y + h))
        for (xa, ya, xb, yb) in boxes:
            out[p, ya:yb, xa:xb] = rng.integers(1, 1001, size=(yb - ya, xb - xa))
        neg = rng.random((H, W)) < 0.03
        out[p][neg] = -rng.integers(1, 201, size=int(neg.sum()))
    return out if n > 1 else out[0]


def _maps(h, E):
    if hasattr(h, "fire_maps"):
        return h.fire_maps()
    return np.stack([h.fire_map(e) for e in range(E)])


def drive(case, mode, a, b=None, n_envs=None, torch=None, swap_at=None, check=None):
    """Drives A (and B) through the case.  Behind every call of B and behind every op: ``B.damage()`` and ``B.values_torch()[0]``
    equal the oracle's sum for every environment.  ``swap_at``: behind that call B gets another plane (``make_values`` with
    ``seed_offset=1``) and the oracle sums under it from there on.  ``check(tag, want)``: called instead of the built-in comparison
    (the twin test compares two handles of its own).  Returns what the case saw on A."""
    c, vc = CASES[case], VALUE_CASES[case]
    kw, R8, E, inits = make_world(case, n_envs)
    H, W = c["H"], c["W"]
    rng = np.random.default_rng(c["seed"] + 1)
    K = c.get("lines", 0)
    values = make_values(case, E, inits)
    exp = MapArrival(E, H, W)
    seen = dict(rises=0, total=[], reset_after_damage=0, ignition_value=0, line_on_burning_town=0, negative_counted=0, ops=[], launches=[])
    a.reset(inits)
    late = bool(c.get("late"))
    values_at = vc.get("values_at")
    valued = values_at is None
    if b is not None:
        b.reset(inits)
        if not late:
            b.enable_arrival(True)
        if valued:
            b.values_set(values)
    maps = _maps(a, E)
    for e in range(E):
        exp.see(e, maps[e], 0)
    snap = None

    def want():
        return damage(values, exp.exp)

    def note():
        d = want()
        if seen["total"] and int(d.sum()) != seen["total"][-1]:
            seen["rises"] += 1
        seen["total"].append(int(d.sum()))
        v = np.broadcast_to(values, exp.exp.shape)
        seen["negative_counted"] = max(seen["negative_counted"], int(((v < 0) & (exp.exp >= 0)).sum()))

    def compare(tag):
        if b is None or not valued:
            return
        w = want()
        if check is not None:
            check(tag, w)
            return
        got = b.damage()
        assert got.dtype == np.int64 and (got == w).all(), (tag, "damage", got.tolist(), w.tolist())
        dev = b.values_torch()[0].cpu().numpy()
        assert dev.dtype == np.int64 and (dev == w).all(), (tag, "values_torch", dev.tolist(), w.tolist())

    def new_episode(envs):
        d = want()
        for e in envs:
            seen["reset_after_damage"] += int(d[e] != 0)
            exp.restart(e)
        m = _maps(a, E)
        for e in envs:
            exp.see(e, m[e], 0)
        d = want()
        seen["ignition_value"] += sum(int(d[e] != 0) for e in envs)

    seen["ignition_value"] += int((want() != 0).sum())
    compare((case, mode, "reset"))
    n_calls = c.get("calls", 14)
    for i in range(n_calls):
        n = STEPS[i % len(STEPS)]
        pts = np.zeros((n, E, max(K, 1), 3), dtype=np.int32)
        for s in range(n):
            if K:
                m = _maps(a, E)
                rows = []
                for e in range(E):
                    ys, xs = np.nonzero(m[e] == BURNING)
                    for j in range(K):
                        if len(xs) and rng.random() < 0.5:          # on a burning cell, or next to one
                            q = int(rng.integers(len(xs)))
                            x = int(np.clip(xs[q] + rng.integers(-1, 2), 0, W - 1))
                            y = int(np.clip(ys[q] + rng.integers(-1, 2), 0, H - 1))
                        else:
                            x, y = int(rng.integers(W)), int(rng.integers(H))
                        t = int(rng.choice([0, 3, 4, 5]))            # (0: padding)
                        pts[s, e, j] = (x, y, t)
                        if t:
                            rows.append((e, x, y, t))
                            v = values[e] if values.ndim == 3 else values
                            seen["line_on_burning_town"] += int(m[e][y, x] == BURNING and v[y, x] != 0)
                if rows:
                    a.apply_mitigation(rows)
            a.step(1)
            m = _maps(a, E)
            st = a.status()[0]
            for e in range(E):
                exp.see(e, m[e], st[e, 1])
        note()
        if b is not None:
            if K:
                b.step_mitigated(pts)
            else:
                b.step(n)
            seen["launches"].append((n, (b.last_launch_kind(), b.cell_layout())))
        compare((case, mode, i, n))
        op = c.get("ops", {}).get(i)
        if op:
            seen["ops"].append(op[0])
            hs = [h for h in (a, b) if h is not None]
            if op[0] in ("reset_envs", "reset_where_mask"):
                envs = sorted(int(e) for e in rng.choice(E, size=op[1], replace=False))
                xy = np.stack([rng.integers(W, size=E), rng.integers(H, size=E)], axis=1).astype(np.int32)
                for e in envs:
                    a.reset_env(e, int(xy[e, 0]), int(xy[e, 1]))
                if b is not None and op[0] == "reset_envs":
                    b.reset_envs(envs, xy[envs])
                elif b is not None:
                    mask = torch.zeros(E, dtype=torch.uint8, device="cuda")
                    mask[envs] = 1
                    b.reset_where(mask, xy)
                new_episode(envs)
            elif op[0] == "reset_where_none":
                envs = [int(e) for e in np.flatnonzero(a.status()[0][:, 0] != 1)]
                xy = np.stack([rng.integers(W, size=E), rng.integers(H, size=E)], axis=1).astype(np.int32)
                for e in envs:
                    a.reset_env(e, int(xy[e, 0]), int(xy[e, 1]))
                if b is not None:
                    b.reset_where(None, xy)
                seen["ops"].append(("not running", len(envs)))
                new_episode(envs)
            elif op[0] == "reset_env":
                e = int(np.argmax(np.abs(want())))
                x, y = int(rng.integers(W)), int(rng.integers(H))
                for h in hs:
                    h.reset_env(e, x, y)
                new_episode([e])
            elif op[0] == "copy":
                src = int(np.argmax((exp.exp >= 0).sum(axis=(1, 2))))
                dst = [e for e in range(E) if e != src][:op[1]]
                for h in hs:
                    h.copy_envs([src] * len(dst), dst)
                for d in dst:
                    exp.exp[d] = exp.exp[src]
            elif op[0] == "save":
                envs = [e for e in range(E) if e % 2 == 0]
                blob_b = None
                if b is not None:
                    if op[1]:
                        out = torch.empty((len(envs), b.state_bytes()), dtype=torch.uint8, device="cuda")
                        blob_b = b.save_state(envs, out=out)
                    else:
                        blob_b = b.save_state(envs)
                snap = (envs, a.save_state(envs), blob_b, exp.exp[envs].copy())
            elif op[0] == "load":
                envs, blob_a, blob_b, e_then = snap
                seen["ops"].append(("damage restored", int(np.abs(damage(values, exp.exp)[envs] - damage(values[envs] if values.ndim == 3 else values, e_then)).sum())))
                a.load_state(envs, blob_a)
                if b is not None:
                    b.load_state(envs, blob_b)
                exp.exp[envs] = e_then
            elif op[0] == "enable":
                m = _maps(a, E)
                exp.exp[m != BURNING] = -1          # cells that burned out before this moment stay "never"
                if b is not None:
                    b.enable_arrival(True)
            compare((case, mode, i, n, op[0]))
        if values_at == i:                       # the plane in the middle of the episode: a recount from the plane as it stands
            seen["ops"].append(("values set at damage", int(np.abs(want()).sum())))
            if b is not None:
                b.values_set(values)
            valued = True
            compare((case, mode, i, n, "values_set"))
        if swap_at == i:
            values = make_values(case, E, inits, seed_offset=1)
            if b is not None:
                b.values_set(values)
            compare((case, mode, i, n, "swap"))
    return seen
