"""Fire behaviour: the arguments of ``behavior`` checked and turned into ``sf_behavior_params`` / ``sf_behavior_out``
(include/simfire_hip.h).

Pure Python: every check happens here, before a device call, so that a bad request raises ``ValueError`` the same way with or
without a GPU.  The definitions, the kernel and the heat cache are described in DESIGN.md section 25.
"""
import math

import numpy as np

from . import _args
from ._lib import SfBehaviorOut, SfBehaviorParams

#: the planes a call can write: name -> the torch dtype's name
PLANES = {"hpa": "float32", "ros": "float32", "intensity": "float32", "flame_length": "float32", "head": "int8"}
#: the flame lengths (ft) of the fire characteristics chart: hand crews below 4, equipment below 8, nothing direct above 11
DEFAULT_EDGES = (4.0, 8.0, 11.0, 1e30)


def _number(v, what):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"behavior: {what} must be a number, got {v!r}")
    return float(v)


def request(status=None, summary=("BURNING",), flame_limit=None, edges=None):
    """The checked scalar arguments of ``behavior``: (status mask or 0 for every cell, summary mask, flame_limit or ``None``,
    the four class edges as float32)."""
    empty = status is None or (isinstance(status, (tuple, list, set, frozenset)) and len(status) == 0)
    smask = 0 if empty else _args.status_mask("behavior", status)
    summask = _args.status_mask("behavior", ("BURNING",) if summary is None else summary, "summary")
    limit = None
    if flame_limit is not None:
        limit = _number(flame_limit, "flame_limit")
        if math.isnan(limit) or limit < 0.0:
            raise ValueError(f"behavior: flame_limit must be >= 0, got {flame_limit!r}")
        limit = float(np.float32(limit))
    try:
        e = [_number(v, "an edge") for v in (DEFAULT_EDGES if edges is None else edges)]
    except TypeError:
        raise ValueError(f"behavior: edges are four increasing flame lengths, got {edges!r}") from None
    e32 = [float(np.float32(v)) for v in e]
    if len(e32) != 4 or any(math.isnan(v) for v in e32) or not (e32[0] < e32[1] < e32[2] < e32[3]):
        raise ValueError(f"behavior: edges are four increasing flame lengths (as float32), got {edges!r}")
    return smask, summask, limit, tuple(e32)


class BehaviorSpec:
    """A checked behaviour request: the outputs asked for with their shapes and dtypes, and the arrays the call reads."""

    def __init__(self, n_envs, H, W, envs=None, status=None, summary=("BURNING",), flame_limit=None, edges=None, points=None,
                 planes=("flame_length",), workable=False, stats=False):
        self.status, self.summary, self.flame_limit, self.edges = request(status, summary, flame_limit, edges)
        self.envs = _args.env_list(envs, n_envs, "behavior", none_all=True)
        n = self.n = int(self.envs.shape[0])
        if isinstance(planes, str):
            planes = (planes,)
        try:
            planes = tuple(() if planes is None else planes)
        except TypeError:
            raise ValueError(f"behavior: planes is a list of {', '.join(PLANES)}, got {planes!r}") from None
        for name in planes:
            if name not in PLANES:
                raise ValueError(f"behavior: unknown plane {name!r} (one of {', '.join(PLANES)})")
        _args.flags("behavior", workable=workable, stats=stats)
        if workable and self.flame_limit is None:
            raise ValueError("behavior: workable needs flame_limit")
        self.points, self.k = _args.query_points("behavior", points, n)
        if not (planes or workable or stats or self.k):
            raise ValueError("behavior: nothing asked for (planes, workable, stats or points)")
        shapes = {name: ((n, H, W), PLANES[name]) for name in PLANES}
        shapes.update(workable=((n, H, W), "uint8"), max_flame=((n,), "float32"), max_intensity=((n,), "float32"),
                      classes=((n, 5), "int32"), point_flame=((n, self.k), "float32"))
        asked = {name: name in planes for name in PLANES}
        asked.update(workable=bool(workable), max_flame=bool(stats), max_intensity=bool(stats), classes=bool(stats),
                     point_flame=bool(self.k))
        #: output name -> (shape, the torch dtype's name), in the order of ``sf_behavior_out``
        self.outputs = {name: shapes[name] for name in shapes if asked[name]}

    def device_tensors(self):
        """The CUDA tensors the call reads (the caller checks they live on the handle's GPU)."""
        return [self.points] if self.k else []

    def params(self):
        p = SfBehaviorParams(status_mask=self.status, summary_mask=self.summary, k=self.k, reserved=0,
                             flame_limit=0.0 if self.flame_limit is None else self.flame_limit,
                             points=self.points.data_ptr() if self.k else None)
        for i in range(4):
            p.edges[i] = self.edges[i]
        return p

    def out(self, tensors):
        """The ``sf_behavior_out`` of the output tensors (name -> tensor, as ``outputs`` lists them)."""
        return SfBehaviorOut(**{name: t.data_ptr() for name, t in tensors.items()})
