"""Reference for ensemble statistics (``sf_ensemble_stats``), independent of the library: a NumPy restatement
of the definitions in ``include/simfire_hip.h``.  It works from int32 arrival arrays ``[E, H, W]`` as ``sf_get_arrival`` returns them
(the update that ignited the cell, -1 = never) and a value plane ``[H, W]`` or ``[E, H, W]``; it reads nothing else."""
import numpy as np


def reached(arrival, h):
    """bool, shape of ``arrival``: the fire has reached the cell by horizon ``h`` (an update index; < 0: no limit)."""
    arrival = np.asarray(arrival)
    return (arrival >= 0) if h < 0 else ((arrival >= 0) & (arrival <= h))


def stats(arrival, members, horizons, values=None):
    """dict: ``count`` int32 [G, T, H, W], ``prob`` float32 [G, T, H, W], ``first`` int32 [G, H, W], ``mean`` float32 [G, H, W] and,
    with ``values``, ``loss`` int64 [G, T].  ``members`` [G, K]: an environment counts as often as it is listed."""
    arrival = np.asarray(arrival, dtype=np.int32)
    members = np.asarray(members, dtype=np.int64)
    assert arrival.ndim == 3 and members.ndim == 2
    G, K = members.shape
    T = len(horizons)
    _, H, W = arrival.shape
    count = np.zeros((G, T, H, W), dtype=np.int32)
    first = np.full((G, H, W), -1, dtype=np.int32)
    mean = np.full((G, H, W), -1.0, dtype=np.float32)
    loss = np.zeros((G, T), dtype=np.int64)
    for g in range(G):
        a = arrival[members[g]]                                     # [K, H, W], duplicates repeated
        for t, h in enumerate(horizons):
            r = reached(a, h)
            count[g, t] = r.sum(axis=0)
            if values is not None:
                v = np.asarray(values, dtype=np.int64)
                v = v[members[g]] if v.ndim == 3 else np.broadcast_to(v, a.shape)
                loss[g, t] = int(v[r].sum())
        r = reached(a, horizons[-1])
        n = r.sum(axis=0)
        big = np.where(r, a, np.iinfo(np.int32).max)
        first[g] = np.where(n > 0, big.min(axis=0), -1)
        s = np.where(r, a, 0).astype(np.uint64).sum(axis=0)
        with np.errstate(invalid="ignore", divide="ignore"):
            m = (s.astype(np.float64) / n.astype(np.float64)).astype(np.float32)
        mean[g] = np.where(n > 0, m, np.float32(-1.0))
    prob = count.astype(np.float32) / np.float32(K)
    out = dict(count=count, prob=prob, first=first, mean=mean)
    if values is not None:
        out["loss"] = loss
    return out


def torch_assembly(a1, members, horizons):
    """``count`` and ``first`` assembled in torch from the raw plane ``a1`` (``arrival_torch()``: update + 1, 0 = never), the way a
    caller does it without the entry: several passes with temporaries as large as the plane."""
    import torch
    m = torch.as_tensor(np.asarray(members, dtype=np.int64), device=a1.device)
    counts, firsts = [], []
    for g in range(m.shape[0]):
        a = a1[m[g]]
        per_t = []
        for h in horizons:
            r = (a > 0) if h < 0 else ((a > 0) & (a <= h + 1))
            per_t.append(r.sum(0).to(torch.int32))
        counts.append(torch.stack(per_t))
        h = horizons[-1]
        r = (a > 0) if h < 0 else ((a > 0) & (a <= h + 1))
        big = torch.where(r, a - 1, torch.full_like(a, 2 ** 31 - 1)).amin(0)
        firsts.append(torch.where(r.any(0), big, torch.full_like(big, -1)))
    return torch.stack(counts), torch.stack(firsts)
