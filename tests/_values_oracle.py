"""Reference for values at risk (``sf_values_set``), NumPy only and independent of the library.  The arrival
it sums over is ``tests/_arrival_oracle.MapArrival`` fed with the maps of a handle that does not record (handle A), never the
arrival of the handle under test."""
import numpy as np

VALUE_MAX = 1 << 24


def damage(values, arrival):
    """int64 [E]: per environment the sum of ``values`` over the cells with ``arrival >= 0``.  ``values``: int [H, W] for every
    environment or [E, H, W]; ``arrival``: int [E, H, W], -1 = never."""
    arrival = np.asarray(arrival)
    v = np.broadcast_to(np.asarray(values, dtype=np.int64), arrival.shape)
    return (v * (arrival >= 0)).sum(axis=(1, 2), dtype=np.int64)


def tick_loss(before, after, was_running):
    """int64 [E]: what a tick added to the damage - ``after`` is taken behind the tick's updates and in front of its auto-reset -,
    0 for an environment that was not running before the tick."""
    return np.where(np.asarray(was_running, dtype=bool), np.asarray(after, dtype=np.int64) - np.asarray(before, dtype=np.int64), 0).astype(np.int64)


def reward(weights, terms, w_value=None, loss=0):
    """np.float32 of ``w0 t0 + w1 t1 + w2 t2 + w3 t3 [+ wv * loss]`` evaluated in double, left to right; the weights are the floats
    the C struct holds.  The fifth product is added only while ``w_value`` is not None."""
    w = [float(np.float32(x)) for x in weights]
    r = w[0] * float(terms[0])
    r = r + w[1] * float(terms[1])
    r = r + w[2] * float(terms[2])
    r = r + w[3] * float(terms[3])
    if w_value is not None:
        r = r + float(np.float32(w_value)) * float(int(loss))
    return np.float32(r)


class RewardBook:
    """The reward, episode return and final return of ``tests/_agents_oracle.AgentsOracle`` restated with the fifth term: fed every
    tick with the oracle's result (whose terms and done flags do not depend on the reward) and the tick's loss."""

    def __init__(self, n_envs, weights, w_value, auto_reset):
        self.E, self.weights, self.w_value, self.auto_reset = int(n_envs), tuple(weights), w_value, bool(auto_reset)
        self.ep_ret = np.zeros(self.E, dtype=np.float64)

    def tick(self, was_running, terms, done, loss):
        rew = np.zeros(self.E, dtype=np.float32)
        final_ret = np.zeros(self.E, dtype=np.float64)
        for e in range(self.E):
            if was_running[e]:
                rew[e] = reward(self.weights, terms[e], self.w_value, loss[e])
                self.ep_ret[e] = self.ep_ret[e] + float(rew[e])
            if done[e]:
                final_ret[e] = self.ep_ret[e]
                if self.auto_reset:
                    self.ep_ret[e] = 0.0
        return rew, final_ret
