"""The cases of ``tests/test_arrival_gpu.py`` and the loop that drives them.  Handle A is the reference: any engine with the older
API, stepped ONE update at a time with its maps fetched after each (``tests/_arrival_oracle.py`` turns them into the expected
arrival).  Handle B records arrival in the mode under test and makes the same updates in calls of uneven length.
``tests/test_arrival_cpu.py`` runs the same loop with ``oracle/fire_dense`` standing in for A and no B, to check that every case
sees what it claims to cover."""
import numpy as np

from _arrival_oracle import BURNING, MapArrival

STEPS = (1, 2, 3, 5, 7, 11, 23)           # updates per call of B, cycled: piece boundaries fall everywhere relative to md
E_STAND_IN = 264                          # "cu+8" where there is no device to ask

# the mode names of tests/test_env_state_gpu.py (MODES) and three more
EXTRA_MODES = {
    "auto": dict(fused=-1),
    "run_noteam": dict(fused=2, tuning=dict(run_team=1)),      # two-word rows in the plain kernel: the bitmap's planes 1 / 2 are not kept
    "auto_many": dict(fused=-1),
}

# ops: {index of the call they follow: op}.  Ops run on both handles right behind the call, while B's layout is what the call left.
CASES = {
    "24x40": dict(H=24, W=40, modes=("fused0", "fused1", "run"), seed=7101),
    "33x17": dict(H=33, W=17, modes=("fused0", "fused1", "run"), seed=7102),
    "72x80_win": dict(H=72, W=80, modes=("run_win", "run"), seed=7103),
    "64x64_kwin": dict(H=64, W=64, modes=("run_kwin",), seed=7104),
    "136x64_team": dict(H=136, W=64, modes=("run_team",), seed=7105),
    "70x1030_wide": dict(H=70, W=1030, modes=("auto", "run_noteam"), seed=7106, E=3, calls=7),
    "24x40_md8": dict(H=24, W=40, md=8, modes=("auto",), seed=7107),
    "64x64_many": dict(H=64, W=64, modes=("auto_many",), seed=7108, E="cu+8", calls=7),
    "24x40_md1": dict(H=24, W=40, md=1, modes=("run", "fused1"), seed=7109),
    "24x40_md5": dict(H=24, W=40, md=5, modes=("run", "fused0"), seed=7110),
    # control lines through step_mitigated, several updates per call
    "24x40_lines": dict(H=24, W=40, modes=("run", "fused0"), seed=7111, lines=3),
    # the four resets in the middle of a run
    "24x40_resets": dict(H=24, W=40, modes=("run", "fused0"), seed=7112,
                         ops={3: ("reset_envs", 2), 5: ("reset_where_mask", 2), 7: ("reset_where_none",), 8: ("reset_env",)}, calls=12),
    "72x80_resets": dict(H=72, W=80, modes=("run_win",), seed=7113,
                         ops={3: ("reset_envs", 2), 4: ("reset_where_mask", 2), 6: ("reset_where_none",), 8: ("reset_env",)}, calls=11),
    # one environment forked into many, then every fork draws lines of its own
    "24x40_fork": dict(H=24, W=40, modes=("run", "fused0"), seed=7114, lines=2, ops={4: ("copy", 3)}),
    # snapshot, go on, restore (host blobs / device blobs)
    "24x40_state": dict(H=24, W=40, modes=("run", "fused0"), seed=7115, ops={3: ("save", False), 5: ("load",), 6: ("save", True), 8: ("load",)},
                        calls=11),
    # recording switched on in the middle of an episode
    "24x40_late": dict(H=24, W=40, modes=("run", "fused0"), seed=7116, ops={4: ("enable",)}, late=True),
    "72x80_late": dict(H=72, W=80, modes=("run_win",), seed=7117, ops={3: ("enable",)}, late=True),
}
PAIRS = [(case, mode) for case in CASES for mode in CASES[case]["modes"]]


def mode_settings(mode):
    from test_env_state_gpu import MODES
    return MODES[mode] if mode in MODES else EXTRA_MODES[mode]


def make_world(case, n_envs=None):
    """(engine kwargs without n_envs, R table, E, ignitions [E, 2]) of a case; ``n_envs``: the value of E = "cu+8"."""
    from test_env_state_gpu import _world
    c = CASES[case]
    H, W = c["H"], c["W"]
    rng = np.random.default_rng(c["seed"])
    E = int(rng.integers(4, 8))
    if "E" in c:
        E = int(c["E"]) if c["E"] != "cu+8" else int(n_envs if n_envs is not None else E_STAND_IN)
    kw, R8 = _world(rng, H, W, c.get("md", 4), bool(rng.integers(2)))
    dead = R8.sum(axis=0) == 0.0
    R8 = np.maximum(R8, 12.0)                         # fires that go on for several times max_fire_duration ...
    R8[:, dead] = 0.0                                 # ... around cells that never burn
    kw.update(max_time=(None if E > 5 or rng.random() < 0.7 else float(rng.integers(20, 40))), update_rate=1.0,
              pixel_scale=float(rng.choice([5.0, 20.0, 30.0])))
    inits = np.stack([rng.integers(W // 4, W - W // 4, size=E), rng.integers(H // 4, H - H // 4, size=E)], axis=1).astype(np.int32)
    return kw, R8, E, inits


class DenseStandIn:
    """Handle A without a device: one single-environment ``oracle/fire_dense`` per environment and the log of what was done to it;
    a fork or a restore replays a log into a fresh oracle."""

    def __init__(self, kw, R8, E):
        self.kw, self.R8, self.n_envs = dict(kw), R8, E
        self.o, self.logs = [None] * E, [[] for _ in range(E)]

    def _fresh(self, log):
        from oracle import fire_dense
        o = fire_dense.DenseOracle(n_envs=1, **self.kw)
        o.set_rtable(self.R8)
        for op in log:
            self._apply(o, op)
        return o

    @staticmethod
    def _apply(o, op):
        if op[0] == "reset":
            o.reset([op[1]])
        elif op[0] == "mit":
            o.apply_mitigation([(0, x, y, t) for (x, y, t) in op[1]])
        else:
            o.step(op[1])

    def _do(self, e, op):
        if op[0] == "reset":
            self.logs[e] = [op]
            self.o[e] = self._fresh(self.logs[e])
            return
        self.logs[e].append(op)
        self._apply(self.o[e], op)

    def reset(self, xy):
        for e in range(self.n_envs):
            self._do(e, ("reset", (int(xy[e][0]), int(xy[e][1]))))

    def reset_env(self, e, x, y):
        self._do(e, ("reset", (int(x), int(y))))

    def apply_mitigation(self, rows):
        for e in range(self.n_envs):
            mine = [(int(x), int(y), int(t)) for (q, x, y, t) in rows if q == e]
            if mine:
                self._do(e, ("mit", mine))

    def step(self, n):
        for e in range(self.n_envs):
            self._do(e, ("step", int(n)))

    def fire_map(self, e):
        return self.o[e].fire_map(0)

    def burn(self, e):
        return self.o[e].burn(0)

    def status(self):
        st, el = zip(*(o.status() for o in self.o))
        return np.concatenate(st), np.concatenate(el)

    def copy_envs(self, src, dst):
        for s, d in zip(src, dst):
            self.logs[d] = list(self.logs[s])
            self.o[d] = self._fresh(self.logs[d])

    def save_state(self, envs):
        return [list(self.logs[e]) for e in envs]

    def load_state(self, envs, snap):
        for e, log in zip(envs, snap):
            self.logs[e] = list(log)
            self.o[e] = self._fresh(log)


def expected_launch(mode, c, n, updates_after, lines):
    """(last_launch_kind, cell_layout) B must show behind a call of n updates, or None where the plan depends on more than the mode."""
    if c.get("md", 4) > 5:
        return (3, 0)                                        # sprite planes of two bytes: the per-cell kernel
    if mode in ("fused0", "fused1"):
        return (int(mode[-1]), 0)
    if mode in ("run", "run_win", "run_team", "run_noteam"):
        return (2, 1)
    if mode in ("run_kwin", "auto_many"):                    # k_win in front while every fire is surely young, in calls of >= 2 updates
        return (4, 1) if n >= 2 and not lines and 1 + 2 * updates_after <= 56 else None
    if mode == "auto":                                       # two-word rows: the team launch from two updates on
        return (2, 1) if n >= 2 and not lines else None
    raise KeyError(mode)


def _maps(h, E):
    if hasattr(h, "fire_maps"):
        return h.fire_maps()
    return np.stack([h.fire_map(e) for e in range(E)])


def drive(case, mode, a, b=None, n_envs=None, torch=None):
    """Drives A (and B) through the case.  Behind every call of B: the launch structure the mode names ran and left its layout;
    ``B.arrival(e)`` equals the expected array of every environment; B's maps, status rows and elapsed times equal A's; then the
    case's op for this call on both handles and the same comparisons again; then the burn amounts (last: fetching them converts B
    to the row-major planes).  Returns what the case saw on A."""
    c = CASES[case]
    kw, R8, E, inits = make_world(case, n_envs)
    H, W, md = c["H"], c["W"], c.get("md", 4)
    rng = np.random.default_rng(c["seed"] + 1)
    K = c.get("lines", 0)
    exp = MapArrival(E, H, W)
    seen = dict(cells=0, span=0, reset_after_arrivals=0, on_burning=0, launches=[], ops=[])
    a.reset(inits)
    if b is not None:
        b.reset(inits)
        if not c.get("late"):
            b.enable_arrival(True)
    recording = not c.get("late")
    maps = _maps(a, E)
    for e in range(E):
        exp.see(e, maps[e], 0)
    snap = None
    updates = 0
    few = list(range(E)) if E <= 16 else [0, 1, 2, E // 2, E - 2, E - 1]

    def note():
        seen["cells"] = max(seen["cells"], int((exp.exp >= 0).sum()))
        seen["span"] = max(seen["span"], int(exp.exp.max()))

    def compare(tag, burn=False):
        if b is None:
            return
        st_a, el_a = a.status()
        st_b, el_b = b.status()
        assert (st_a == st_b).all() and (el_a == el_b).all(), (tag, "status")
        assert (_maps(a, E) == b.fire_maps()).all(), (tag, "fire maps")
        if recording:
            if E <= 16:
                got = np.stack([b.arrival(e) for e in range(E)])
            else:
                got = b.arrival_torch().cpu().numpy() - 1
            bad = np.argwhere(got != exp.exp)
            assert not len(bad), (tag, "arrival", len(bad), bad[:5].tolist(), [(int(got[tuple(i)]), int(exp.exp[tuple(i)])) for i in bad[:5]])
        if burn:
            for e in few:
                assert (a.burn(e) == b.burn(e)).all(), (tag, "burn", e)

    def new_episode(envs):
        for e in envs:
            if int((exp.exp[e] >= 0).sum()) >= 2:
                seen["reset_after_arrivals"] += 1
            exp.restart(e)
        m = _maps(a, E)
        for e in envs:
            exp.see(e, m[e], 0)

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
                            seen["on_burning"] += int(m[e][y, x] == BURNING)
                if rows:
                    a.apply_mitigation(rows)
            a.step(1)
            updates += 1
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
            want = expected_launch(mode, c, n, updates, bool(K))
            got = (b.last_launch_kind(), b.cell_layout())
            seen["launches"].append((n, got))
            if want is not None:
                assert got == want, (case, mode, i, n, got, want)
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
                e = int(np.argmax((exp.exp >= 0).sum(axis=(1, 2))))
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
                a.load_state(envs, blob_a)
                if b is not None:
                    b.load_state(envs, blob_b)
                exp.exp[envs] = e_then
            elif op[0] == "enable":
                # cells that burned out before this moment stay "never"; a sprite that is live now (no control lines in these cases:
                # its cell shows BURNING) carries its true update
                m = _maps(a, E)
                exp.exp[m != BURNING] = -1
                seen["ops"].append(("live at enable", int((exp.exp >= 0).sum()), "burned out", int((m == 2).sum())))
                if b is not None:
                    b.enable_arrival(True)
                recording = True
            compare((case, mode, i, n, op[0]))
        compare((case, mode, i, n, "burn"), burn=True)
    note()
    if b is not None and recording:
        raw = b.arrival_torch().cpu().numpy()
        assert raw.dtype == np.int32 and raw.shape == (E, H, W)
        for e in few:
            assert (raw[e] - 1 == b.arrival(e)).all(), (case, mode, "arrival_torch", e)
    return seen
