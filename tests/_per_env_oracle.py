"""ORACLE (test infrastructure): per-environment terrain for ``oracle/fire_dense.c``.

``DenseOracle`` holds one R table for all of its environments.  ``PerEnvOracle`` holds E one-environment
``DenseOracle``s behind the multi-environment interface the tests drive (``set_rtable(R8, env=None)``,
``reset``, ``apply_mitigation`` with an environment column, ``step(n)``, ``fire_map(e)``, ``status()``
with the rows stacked ...), so that every environment spreads over a table of its own, like a
``FireEngine(per_env_terrain=True)``.

Every environment also keeps the history of calls that made its state (its tables included), so that a fork
or a restore of the device (``copy_envs``, ``load_state``) can be mirrored by replaying the source's
history into a fresh oracle: ``copy_env``.
"""
import numpy as np

from oracle import fire_dense


class PerEnvOracle:
    def __init__(self, shape, n_envs=1, **kw):
        self.H, self.W = int(shape[0]), int(shape[1])
        self.n_envs = int(n_envs)
        self._kw = dict(kw, shape=(self.H, self.W))
        self._o = [fire_dense.DenseOracle(n_envs=1, **self._kw) for _ in range(self.n_envs)]
        self._log = [[] for _ in range(self.n_envs)]     # calls that made each environment's state, in order, from its last reset
        self._tab = [None] * self.n_envs                 # the table each environment spreads over now

    def _envs(self, env):
        return range(self.n_envs) if env is None else [int(env)]

    # ------------------------------------------------------------------ tables
    def set_rtable(self, R8, env=None):
        R8 = np.array(R8, dtype=np.float64)
        assert R8.shape == (8, self.H, self.W)
        for e in self._envs(env):
            self._tab[e] = R8
            self._do(e, ("table", R8))

    def get_rtable(self, env=0):
        return self._o[int(env)].get_rtable()

    def build_rtable(self, w_0, delta, M_x, sigma, elevation, U, U_dir, M_f, particle=(8000.0, 0.0555, 0.01, 32.0), env=None):
        for e in self._envs(env):
            self._o[e].build_rtable(w_0, delta, M_x, sigma, elevation, U, U_dir, M_f, particle=particle)
            self._tab[e] = self._o[e].get_rtable()
            self._log[e].append(("table", self._tab[e]))

    # ------------------------------------------------------------------ state
    def _do(self, e, op):
        self._log[e].append(op)
        self._apply(self._o[e], op)

    @staticmethod
    def _apply(o, op):
        kind = op[0]
        if kind == "table":
            o.set_rtable(op[1])
        elif kind == "reset":
            o.reset([op[1]])
        elif kind == "mit":
            o.apply_mitigation(op[1])
        elif kind == "map":
            o.load_fire_map(0, op[1])
        elif kind == "burn":
            o.set_burn(0, op[1])
        elif kind == "step":
            o.step(op[1])
        else:
            raise ValueError(kind)

    def reset(self, init_xy):
        xy = np.asarray(init_xy, dtype=np.int32).reshape(-1, 2)
        if xy.shape[0] == 1 and self.n_envs > 1:
            xy = np.repeat(xy, self.n_envs, axis=0)
        assert xy.shape[0] == self.n_envs
        for e in range(self.n_envs):
            self.reset_env(e, xy[e, 0], xy[e, 1])

    def reset_env(self, env, x, y):
        e = int(env)
        self._log[e] = [] if self._tab[e] is None else [("table", self._tab[e])]
        self._do(e, ("reset", (int(x), int(y))))

    def apply_mitigation(self, pts):
        """pts: rows (env, x, y, type); each environment gets its rows in the order given."""
        q = np.asarray(pts, dtype=np.int32).reshape(-1, 4)
        for e in range(self.n_envs):
            mine = q[q[:, 0] == e]
            if len(mine):
                mine = mine.copy()
                mine[:, 0] = 0
                self._do(e, ("mit", mine))

    def load_fire_map(self, env, fire_map):
        self._do(int(env), ("map", np.array(fire_map, dtype=np.uint8)))

    def set_burn(self, env, burn):
        self._do(int(env), ("burn", np.array(burn, dtype=np.float64)))

    def step(self, n=1, threads=1):
        """``threads`` > 1: the environments side by side (their oracles share nothing; ctypes lets go of the GIL in the call)."""
        if threads > 1 and self.n_envs > 1:
            from concurrent.futures import ThreadPoolExecutor
            with ThreadPoolExecutor(min(int(threads), self.n_envs)) as ex:
                list(ex.map(lambda e: self._do(e, ("step", int(n))), range(self.n_envs)))
        else:
            for e in range(self.n_envs):
                self._do(e, ("step", int(n)))

    def copy_env(self, src, dst, terrain=False, source=None):
        """Environment ``dst`` takes the state of environment ``src`` of ``source`` (default: this oracle) - and its table if
        ``terrain``; otherwise ``dst`` goes on over the table it had."""
        source = self if source is None else source
        src, dst = int(src), int(dst)
        o = fire_dense.DenseOracle(n_envs=1, **self._kw)
        log = list(source._log[src])
        for op in log:
            self._apply(o, op)
        tab = source._tab[src] if terrain else self._tab[dst]
        if not terrain:
            log.append(("table", tab))
            o.set_rtable(tab)
        self._o[dst], self._log[dst], self._tab[dst] = o, log, tab

    # ------------------------------------------------------------------ results
    def fire_map(self, env=0):
        return self._o[int(env)].fire_map(0)

    def burn(self, env=0):
        return self._o[int(env)].burn(0)

    def parents(self, env=0):
        return self._o[int(env)].parents(0)

    def status(self):
        """(int32 [E, 8] = running, steps, counts[0..5]; float64 [E] elapsed_time)"""
        rows, el = zip(*(o.status() for o in self._o))
        return np.concatenate(rows, axis=0), np.concatenate(el, axis=0)
