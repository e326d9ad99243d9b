"""Reference for arrival times (``sf_enable_arrival``), independent of the library: what a caller of the
reference rebuilds from ``fire_map.npy`` after a run, and a NumPy restatement of how a pass decodes the sprite masks."""
import numpy as np

BURNING = 1


def arrival_from_maps(maps):
    """int32 [H, W]: for a sequence of maps of one environment - the map after its reset, then after every update - the first index
    at which each cell shows BURNING, else -1.  Index 0 is the reset's ignition, index u the update() call number u."""
    maps = np.asarray(maps)
    out = np.full(maps.shape[1:], -1, dtype=np.int32)
    for i, m in enumerate(maps):
        out[(m == BURNING) & (out < 0)] = i
    return out


class MapArrival:
    """The same, one map at a time, for every environment of a handle that is watched while it runs: ``see(e, map, steps)`` after
    every update of environment e (steps = update() calls it has made since its reset); ``restart(e)`` at a reset."""

    def __init__(self, n_envs, H, W):
        self.exp = np.full((n_envs, H, W), -1, dtype=np.int32)

    def restart(self, e):
        self.exp[e] = -1

    def see(self, e, fire_map, steps):
        x = self.exp[e]
        x[(np.asarray(fire_map) == BURNING) & (x < 0)] = int(steps)


def slot_of(s, N):
    return s % N          # (Python's % is non-negative for N > 0)


def decode_masks(masks, t, md, arrival1):
    """One pass over the sprite masks (any integer array) of an environment that has made ``t`` updates: writes update + 1 into
    ``arrival1`` (same shape, 0 = never) where it is still 0.  A sprite created by update s owns bit ``slot_of(s, md + 3)``; the
    updates t - md .. t are told apart, the oldest sprite of a cell wins.  Returns the number of cells written."""
    N = md + 3
    masks = np.asarray(masks).astype(np.int64)
    best = np.zeros(masks.shape, dtype=np.int64)
    for d in range(0, md + 1):                       # newest to oldest: the oldest is written last
        s = t - d
        if s < 0:
            break
        hit = (masks >> slot_of(s, N)) & 1
        best[hit == 1] = s + 1
    write = (best > 0) & (arrival1 == 0)
    arrival1[write] = best[write]
    return int(write.sum())
