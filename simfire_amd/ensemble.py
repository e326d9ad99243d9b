"""Ensemble statistics: the arguments of ``ensemble_stats`` checked and turned into ``sf_ensemble_params`` / ``sf_ensemble_out``
(include/simfire_hip.h).

Pure Python: every check happens here, before a device call, so that a bad request raises ``ValueError`` the same way with or
without a GPU.  The statistics are specified in DESIGN.md section 21.
"""
import numpy as np

from . import _args
from ._lib import ENS_MAX_HORIZONS, SfEnsembleOut, SfEnsembleParams


def request(n_envs, members, horizons):
    """The checked arguments of ``ensemble_stats``: (int32 [G, K] contiguous, list of horizons)."""
    m = _args.env_list(members, n_envs, "ensemble_stats", "members", none_all=True, ndim=2)
    G, K = m.shape
    if G < 1 or not 1 <= K <= 65535 or G * K > 1 << 20:
        raise ValueError(f"ensemble_stats: {G} groups of {K} members (G >= 1, 1 <= K <= 65535, G * K <= 2**20)")
    try:
        hz = [int(h) for h in np.asarray(horizons).reshape(-1).tolist()]
    except (TypeError, ValueError):
        raise ValueError(f"ensemble_stats: horizons must be integers, got {horizons!r}") from None
    if np.asarray(horizons).dtype.kind not in "iu" or not 1 <= len(hz) <= ENS_MAX_HORIZONS:
        raise ValueError(f"ensemble_stats: 1 to {ENS_MAX_HORIZONS} integer horizons, got {horizons!r}")
    for t, h in enumerate(hz):
        if h < -1 or h > 2 ** 31 - 1 or (h == -1 and t != len(hz) - 1):
            raise ValueError(f"ensemble_stats: horizon {h} (>= 0; -1, no limit, only as the last)")
        if t and h != -1 and h <= hz[t - 1]:
            raise ValueError(f"ensemble_stats: the horizons must be strictly ascending, got {hz}")
    return m, hz


class EnsembleSpec:
    """A checked ensemble request: the outputs asked for with their shapes and dtypes."""

    def __init__(self, n_envs, H, W, members, horizons=(-1,), count=False, prob=True, first=False, mean=False, loss=False):
        self.members, self.horizons = request(n_envs, members, horizons)
        (G, K), T = self.members.shape, len(self.horizons)
        shapes = dict(count=((G, T, H, W), "int32"), prob=((G, T, H, W), "float32"), first=((G, H, W), "int32"),
                      mean=((G, H, W), "float32"), loss=((G, T), "int64"))
        want = dict(count=count, prob=prob, first=first, mean=mean, loss=loss)
        #: output name -> (shape, the torch dtype's name), in the order of ``sf_ensemble_out``
        self.outputs = {name: shapes[name] for name in shapes if want[name]}
        if not self.outputs:
            raise ValueError("ensemble_stats: no output asked for")

    def device_tensors(self):
        """The CUDA tensors the call reads: none, the members are a host array."""
        return []

    def params(self):
        p = SfEnsembleParams(n_groups=self.members.shape[0], group_size=self.members.shape[1], n_horizons=len(self.horizons))
        for t, h in enumerate(self.horizons):
            p.horizons[t] = h
        return p

    def out(self, tensors):
        """The ``sf_ensemble_out`` of the output tensors (name -> tensor, as ``outputs`` lists them)."""
        return SfEnsembleOut(**{name: t.data_ptr() for name, t in tensors.items()})
