"""Fire travel time: the arguments of ``travel`` checked and turned into ``sf_travel_params`` / ``sf_travel_out``
(include/simfire_hip.h).

Pure Python: every check happens here, before a device call, so that a bad request raises ``ValueError`` the same way with or
without a GPU.  The search and its scratch are described in DESIGN.md section 26.
"""
import math

import numpy as np

from . import _args
from ._lib import SF_TRAVEL_BLOCKED, SfTravelOut, SfTravelParams  # noqa: F401

#: ``pred`` is an index into these, the order of the R table's planes: the fire comes from (column + dx, row + dy)
SRC_OFFSETS = ((+1, +1), (0, +1), (-1, +1), (+1, 0), (-1, 0), (+1, -1), (0, -1), (-1, -1))


def request(source=("BURNING",), through=("UNBURNED",), connectivity=None, max_minutes=None, scratch_bytes=0, sources=False):
    """The checked scalar arguments of ``travel``: (source mask, through mask, connectivity code, max_minutes, scratch_bytes).
    ``source`` may be empty (``None``, ``()`` or 0) only when a ``sources`` plane is given; connectivity ``None`` (code 0) is the
    simulation's ``diagonal_spread``; ``max_minutes`` ``None`` (0.0) is no cap."""
    empty = source is None or (isinstance(source, (int, np.integer)) and not isinstance(source, bool) and int(source) == 0) \
        or (isinstance(source, (tuple, list, set, frozenset)) and len(source) == 0)
    if empty:
        if not sources:
            raise ValueError("travel: no source: give source (BurnStatus members, names or ints, or a mask) or a sources plane")
        src = 0
    else:
        src = _args.status_mask("travel", source, "source")
    thr = _args.status_mask("travel", through, "through")
    what = "travel: connectivity must be 4, 8 or None (the simulation's diagonal_spread)"
    conn = 0 if connectivity is None else _args.bounded_int(connectivity, 0, 8, what)
    if conn not in (0, 4, 8):
        raise ValueError(f"{what}, got {connectivity!r}")
    mm = 0.0
    if max_minutes is not None:
        if isinstance(max_minutes, bool) or not isinstance(max_minutes, (int, float, np.integer, np.floating)) \
                or math.isnan(float(max_minutes)) or float(max_minutes) < 0:
            raise ValueError(f"travel: max_minutes must be None or a number >= 0, got {max_minutes!r}")
        mm = float(np.float32(max_minutes))                   # (the cap the search compares with is this float32)
    return src, thr, conn, mm, _args.bounded_int(scratch_bytes, 0, None, "travel: scratch_bytes must be an integer >= 0")


def scratch_need(H, W):
    """Bytes of scratch ``travel`` needs per listed environment of a chunk when no ``minutes`` plane is asked for: the working
    array, float32 [H, W], rounded up to 256."""
    return (4 * int(H) * int(W) + 255) // 256 * 256


class TravelSpec:
    """A checked travel request: the outputs asked for with their shapes and dtypes, and the arrays the call reads."""

    def __init__(self, n_envs, H, W, source=("BURNING",), through=("UNBURNED",), envs=None, connectivity=None, passable=None, sources=None,
                 points=None, max_minutes=None, plane=True, pred=False, reached=False, last=False, activations=False, scratch_bytes=0):
        self.source, self.through, self.connectivity, self.max_minutes, self.scratch = request(
            source, through, connectivity, max_minutes, scratch_bytes, sources=sources is not None)
        self.envs = _args.env_list(envs, n_envs, "travel", none_all=True)
        n = self.n = int(self.envs.shape[0])
        _args.flags("travel", plane=plane, pred=pred, reached=reached, last=last, activations=activations)
        if not (plane or pred or reached or last or activations) and points is None:
            raise ValueError("travel: nothing asked for (plane, pred, reached, last or points)")
        need = scratch_need(H, W)
        if 0 < self.scratch < need:
            raise ValueError(f"travel: scratch_bytes {self.scratch} is less than one environment's need ({need} bytes)")
        if W > 8192:
            raise ValueError(f"travel: grids wider than 8192 cells are not supported (width {W})")
        self.passable, self.passable_per_env = _args.dense_plane("travel", "passable", passable, n_envs, H, W)
        self.sources, self.sources_per_env = _args.dense_plane("travel", "sources", sources, n_envs, H, W)
        self.points, self.k = _args.query_points("travel", points, n)
        shapes = dict(minutes=((n, H, W), "float32"), pred=((n, H, W), "int8"), point_minutes=((n, self.k), "float32"),
                      reached=((n,), "int32"), last=((n,), "float32"), activations=((n,), "int32"))
        asked = dict(minutes=bool(plane), pred=bool(pred), point_minutes=bool(self.k), reached=bool(reached), last=bool(last),
                     activations=bool(activations))
        #: output name -> (shape, the torch dtype's name), in the order of ``sf_travel_out``
        self.outputs = {name: shapes[name] for name in shapes if asked[name]}

    def device_tensors(self):
        """The CUDA tensors the call reads (the caller checks they live on the handle's GPU)."""
        return [t for t in (self.passable, self.sources, self.points) if t is not None]

    def params(self):
        return SfTravelParams(source_mask=self.source, through_mask=self.through, connectivity=self.connectivity, k=self.k,
                              max_minutes=self.max_minutes, passable_per_env=self.passable_per_env, sources_per_env=self.sources_per_env,
                              passable=self.passable.data_ptr() if self.passable is not None else None,
                              sources=self.sources.data_ptr() if self.sources is not None else None,
                              points=self.points.data_ptr() if self.k else None, scratch_bytes=self.scratch)

    def out(self, tensors):
        """The ``sf_travel_out`` of the output tensors (name -> tensor, as ``outputs`` lists them)."""
        return SfTravelOut(**{name: t.data_ptr() for name, t in tensors.items()})
