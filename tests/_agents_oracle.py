"""NumPy restatement of one ``sf_agents_step`` tick (steps a - f of DESIGN.md section 16) for one handle, driven through the
engine API that existed before the agents: ``status()``, ``fire_map(e)``, ``apply_mitigation``, ``step(n)``, ``reset_env``.  The
yardstick of ``tests/test_agents_gpu.py`` (a twin handle is driven by this class) and, with a fake provider of maps and result
rows, of the hand-worked scenario in ``tests/test_agents_cpu.py``.  Test infrastructure only."""
import numpy as np

UNBURNED, BURNING, BURNED = 0, 1, 2


class AgentsOracle:
    """``eng``: anything with ``status() -> (int32 [E, 8], elapsed)``, ``fire_map(e) -> [H, W]``, ``apply_mitigation(rows of
    (env, x, y, type))``, ``step(n)`` and ``reset_env(e, x, y)``."""

    def __init__(self, eng, n_envs, H, W, n_agents, ignitions=None, n_updates=1, weights=(-1.0, 0.0, 0.0, 0.0), only_unburned=True,
                 done_on_burn=False, max_ticks=0, auto_reset=True):
        self.eng, self.E, self.H, self.W, self.K = eng, int(n_envs), int(H), int(W), int(n_agents)
        self.ignitions = None if ignitions is None else np.asarray(ignitions, dtype=np.int32).reshape(self.E, 2)
        self.n_updates, self.only_unburned, self.done_on_burn = int(n_updates), bool(only_unburned), bool(done_on_burn)
        self.max_ticks, self.auto_reset = int(max_ticks), bool(auto_reset)
        self.w = [float(np.float32(v)) for v in weights]          # the C struct holds floats; the kernel widens them
        self.pos = np.zeros((self.E, self.K, 2), dtype=np.int32)   # (column, row)
        self.start = np.zeros((self.E, self.K, 2), dtype=np.int32)
        self.ep_len = np.zeros(self.E, dtype=np.int32)
        self.ep_ret = np.zeros(self.E, dtype=np.float64)

    def place(self, envs, xy, also_start=True):
        xy = np.asarray(xy, dtype=np.int32).reshape(len(envs), self.K, 2)
        for i, e in enumerate(envs):
            self.pos[e] = xy[i]
            if also_start:
                self.start[e] = xy[i]
                self.ep_len[e] = 0
                self.ep_ret[e] = 0.0

    def xyid(self):
        """int32 [E, K, 3] = (column, row, id = j + 1): what ``observe`` takes as agents."""
        ids = np.broadcast_to(np.arange(1, self.K + 1, dtype=np.int32)[None, :, None], (self.E, self.K, 1))
        return np.ascontiguousarray(np.concatenate([self.pos, ids], axis=2))

    def step(self, actions):
        """``actions``: int [E, K].  Returns dict(reward float32 [E], done uint8 [E], terms int32 [E, 4], final_len int32 [E],
        final_ret float64 [E], points int32 [E, K, 3])."""
        E, K = self.E, self.K
        actions = np.asarray(actions).reshape(E, K)
        r0 = np.array(self.eng.status()[0], dtype=np.int64)
        running = r0[:, 0] == 1
        terms = np.zeros((E, 4), dtype=np.int32)
        points = np.zeros((E, K, 3), dtype=np.int32)
        rows = []
        for e in range(E):
            points[e, :, :2] = self.pos[e]
            if not running[e]:
                continue
            before = None                                  # the map before this tick's points (fetched when an agent asks)
            for j in range(K):
                a = int(actions[e, j])
                if a < 0 or a > 19:
                    a = 0
                move, interact = a % 5, a // 5
                x, y = int(self.pos[e, j, 0]), int(self.pos[e, j, 1])
                nx, ny = x + (move == 4) - (move == 3), y + (move == 2) - (move == 1)
                if nx < 0 or nx >= self.W or ny < 0 or ny >= self.H:
                    terms[e, 3] += 1
                else:
                    x, y = nx, ny
                self.pos[e, j] = (x, y)
                points[e, j, :2] = (x, y)
                if interact:
                    emit = True
                    if self.only_unburned:
                        if before is None:
                            before = np.asarray(self.eng.fire_map(e))
                        emit = int(before[y, x]) == UNBURNED
                    if emit:
                        points[e, j, 2] = interact + 2
                        terms[e, 1] += 1
                        rows.append((e, x, y, interact + 2))
        if rows:
            self.eng.apply_mitigation(rows)                # (FIRELINE, then SCRATCHLINE, then WETLINE: update_mitigation's order)
        self.eng.step(self.n_updates)
        r1 = np.array(self.eng.status()[0], dtype=np.int64)
        reward = np.zeros(E, dtype=np.float32)
        done = np.ones(E, dtype=np.uint8)
        final_len = np.zeros(E, dtype=np.int32)
        final_ret = np.zeros(E, dtype=np.float64)
        for e in range(E):
            if running[e]:
                terms[e, 0] = (r1[e, 3] + r1[e, 4]) - (r0[e, 3] + r0[e, 4])
                after = np.asarray(self.eng.fire_map(e))
                terms[e, 2] = sum(int(after[self.pos[e, j, 1], self.pos[e, j, 0]]) == BURNING for j in range(K))
                r = self.w[0] * float(terms[e, 0])
                r = r + self.w[1] * float(terms[e, 1])
                r = r + self.w[2] * float(terms[e, 2])
                r = r + self.w[3] * float(terms[e, 3])
                reward[e] = np.float32(r)
                self.ep_len[e] += 1
                self.ep_ret[e] = self.ep_ret[e] + float(reward[e])
                done[e] = int(r1[e, 0] != 1 or (self.done_on_burn and terms[e, 2] > 0)
                              or (self.max_ticks > 0 and self.ep_len[e] >= self.max_ticks))
            if done[e]:
                final_len[e], final_ret[e] = self.ep_len[e], self.ep_ret[e]
        if self.auto_reset:
            for e in np.flatnonzero(done):
                self.eng.reset_env(int(e), int(self.ignitions[e, 0]), int(self.ignitions[e, 1]))
                self.pos[e] = self.start[e]
                self.ep_len[e] = 0
                self.ep_ret[e] = 0.0
        return dict(reward=reward, done=done, terms=terms, final_len=final_len, final_ret=final_ret, points=points)
