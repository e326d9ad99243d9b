"""Escape routes: the arguments of ``escape`` checked and turned into ``sf_escape_params`` / ``sf_escape_out``
(include/simfire_hip.h).

Pure Python: every check happens here, before a device call, so that a bad request raises ``ValueError`` the same way with or
without a GPU.  The search, its scratch and the meaning of the slack are described in DESIGN.md section 30.
"""
import math

import numpy as np

from . import _args
from ._lib import (SF_ESCAPE_BLOCKED, SF_ESCAPE_LOST, SF_ESCAPE_MAX_MOVES, SF_ESCAPE_SAFE, SF_ESCAPE_UNREACHED_SAFE,  # noqa: F401
                   SfEscapeOut, SfEscapeParams)

#: the move codes of ``point_step`` (the action word of DESIGN.md section 16): (d_row, d_column) - those of ``walk``
MOVES = {1: (-1, 0), 2: (1, 0), 3: (0, -1), 4: (0, 1)}


def _number(name, v, positive):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(float(v)) \
            or (float(v) <= 0 if positive else float(v) < 0):
        raise ValueError(f"escape: {name} must be a finite number {'> 0' if positive else '>= 0'}, got {v!r}")
    return float(v)


def move_bound(minutes_per_move, margin_minutes, horizon_minutes):
    """The largest deadline a cell can have, in moves: ``ceil((horizon - margin) / minutes_per_move)`` in float64, as the library
    forms it."""
    return math.ceil((np.float64(horizon_minutes) - np.float64(margin_minutes)) / np.float64(minutes_per_move))


def request(target=(), through=("UNBURNED",), connectivity=4, minutes_per_move=1.0, margin_minutes=0.0, horizon_minutes=None,
            unreached_safe=False, scratch_bytes=0, targets=False):
    """The checked scalar arguments of ``escape``: (target mask, through mask, connectivity code, minutes_per_move, margin_minutes,
    horizon_minutes, flags, scratch_bytes).  ``target`` may be empty (``None``, ``()`` or 0) only when a ``targets`` plane is
    given."""
    empty = target is None or (isinstance(target, (int, np.integer)) and not isinstance(target, bool) and int(target) == 0) \
        or (isinstance(target, (tuple, list, set, frozenset)) and len(target) == 0)
    if empty:
        if not targets:
            raise ValueError("escape: no target: give target (BurnStatus members, names or ints, or a mask) or a targets plane")
        tgt = 0
    else:
        tgt = _args.status_mask("escape", target, "target")
    thr = _args.status_mask("escape", through, "through")
    what = "escape: connectivity must be 4 (the agents' moves) or 8"
    conn = 4 if connectivity is None else _args.bounded_int(connectivity, 0, 8, what)
    if conn not in (0, 4, 8):
        raise ValueError(f"{what}, got {connectivity!r}")
    _args.flags("escape", unreached_safe=unreached_safe)
    mpm = _number("minutes_per_move", minutes_per_move, True)
    margin = _number("margin_minutes", margin_minutes, False)
    if horizon_minutes is None:
        raise ValueError("escape: horizon_minutes is needed (a finite number > 0)")
    horizon = _number("horizon_minutes", horizon_minutes, True)
    bound = move_bound(mpm, margin, horizon)
    if bound > SF_ESCAPE_MAX_MOVES:
        raise ValueError(f"escape: the horizon is {bound} moves away, more than {SF_ESCAPE_MAX_MOVES}")
    return (tgt, thr, conn or 4, mpm, margin, horizon, SF_ESCAPE_UNREACHED_SAFE if unreached_safe else 0,
            _args.bounded_int(scratch_bytes, 0, None, "escape: scratch_bytes must be an integer >= 0"))


def scratch_need(H, W):
    """Bytes of scratch ``escape`` needs per listed environment of a chunk: three bit planes and two halos of the bands, four bytes
    per cell for the cells sorted by deadline, and the bounds of the deadlines' buckets."""
    bands = _args.band_count(H, W)
    return (bands * 16 * 24 + bands * 40 + 255) // 256 * 256 + (4 * int(H) * int(W) + 255) // 256 * 256 \
        + ((2 * SF_ESCAPE_MAX_MOVES + 3) * 4 + 255) // 256 * 256


class EscapeSpec:
    """A checked escape request: the outputs asked for with their shapes and dtypes, and the arrays the call reads."""

    def __init__(self, n_envs, H, W, minutes, target=(), targets=None, through=("UNBURNED",), passable=None, envs=None, connectivity=4,
                 minutes_per_move=1.0, margin_minutes=0.0, horizon_minutes=None, unreached_safe=False, points=None, plane=False,
                 step=False, summary=False, scratch_bytes=0):
        (self.target, self.through, self.connectivity, self.minutes_per_move, self.margin_minutes, self.horizon_minutes, self.flags,
         self.scratch) = request(target, through, connectivity, minutes_per_move, margin_minutes, horizon_minutes, unreached_safe,
                                 scratch_bytes, targets=targets is not None)
        self.envs = _args.env_list(envs, n_envs, "escape", none_all=True)
        n = self.n = int(self.envs.shape[0])
        _args.flags("escape", plane=plane, step=step, summary=summary)
        if not (plane or summary) and points is None:
            raise ValueError("escape: nothing asked for (plane, summary or points)")
        if step and points is None:
            raise ValueError("escape: step needs points")
        need = scratch_need(H, W)
        if 0 < self.scratch < need:
            raise ValueError(f"escape: scratch_bytes {self.scratch} is less than one environment's need ({need} bytes)")
        if W > 8192:
            raise ValueError(f"escape: grids wider than 8192 cells are not supported (width {W})")
        self.passable, self.passable_per_env = _args.dense_plane("escape", "passable", passable, n_envs, H, W)
        self.targets, self.targets_per_env = _args.dense_plane("escape", "targets", targets, n_envs, H, W)
        self.points, self.k = _args.query_points("escape", points, n)
        self.minutes = _args.cuda_tensor(minutes, "escape: minutes", ("float32",), [(n, H, W)]).contiguous()
        i32 = "int32"
        shapes = dict(slack=((n, H, W), i32), point_slack=((n, self.k), i32), point_step=((n, self.k), i32), safe=((n,), i32),
                      escapable=((n,), i32), lost=((n,), i32), top=((n,), i32))
        asked = dict(slack=bool(plane), point_slack=bool(self.k), point_step=bool(step), safe=bool(summary), escapable=bool(summary),
                     lost=bool(summary), top=bool(summary))
        #: output name -> (shape, the torch dtype's name), in the order of ``sf_escape_out``
        self.outputs = {name: shapes[name] for name in shapes if asked[name]}

    def device_tensors(self):
        """The CUDA tensors the call reads (the caller checks they live on the handle's GPU)."""
        return [t for t in (self.minutes, self.passable, self.targets, self.points) if t is not None]

    def params(self):
        return SfEscapeParams(target_mask=self.target, through_mask=self.through, connectivity=self.connectivity, k=self.k,
                              flags=self.flags, passable_per_env=self.passable_per_env, targets_per_env=self.targets_per_env,
                              passable=self.passable.data_ptr() if self.passable is not None else None,
                              targets=self.targets.data_ptr() if self.targets is not None else None,
                              points=self.points.data_ptr() if self.k else None, minutes=self.minutes.data_ptr(),
                              minutes_per_move=self.minutes_per_move, margin_minutes=self.margin_minutes,
                              horizon_minutes=self.horizon_minutes, scratch_bytes=self.scratch)

    def out(self, tensors):
        """The ``sf_escape_out`` of the output tensors (name -> tensor, as ``outputs`` lists them)."""
        return SfEscapeOut(**{name: t.data_ptr() for name, t in tensors.items()})
