"""Walking distance: the arguments of ``walk`` checked and turned into ``sf_walk_params`` / ``sf_walk_out``
(include/simfire_hip.h).

Pure Python: every check happens here, before a device call, so that a bad request raises ``ValueError`` the same way with or
without a GPU.  The search and its scratch are described in DESIGN.md section 24.
"""
import numpy as np

from . import _args
from ._lib import SF_WALK_BLOCKED, SF_WALK_FAR, SfWalkOut, SfWalkParams  # noqa: F401

#: the move codes of ``point_step`` (the action word of DESIGN.md section 16): (d_row, d_column)
MOVES = {1: (-1, 0), 2: (1, 0), 3: (0, -1), 4: (0, 1)}


def request(target=("BURNING",), through=("UNBURNED",), connectivity=4, max_moves=None, scratch_bytes=0, targets=False):
    """The checked scalar arguments of ``walk``: (target mask, through mask, connectivity code, max_moves, scratch_bytes).
    ``target`` may be empty (``None``, ``()`` or 0) only when a ``targets`` plane is given."""
    empty = target is None or (isinstance(target, (int, np.integer)) and not isinstance(target, bool) and int(target) == 0) \
        or (isinstance(target, (tuple, list, set, frozenset)) and len(target) == 0)
    if empty:
        if not targets:
            raise ValueError("walk: no target: give target (BurnStatus members, names or ints, or a mask) or a targets plane")
        tgt = 0
    else:
        tgt = _args.status_mask("walk", target, "target")
    thr = _args.status_mask("walk", through, "through")
    what = "walk: connectivity must be 4 (the agents' moves) or 8"
    conn = 4 if connectivity is None else _args.bounded_int(connectivity, 0, 8, what)
    if conn not in (0, 4, 8):
        raise ValueError(f"{what}, got {connectivity!r}")
    mm = 0 if max_moves is None else _args.bounded_int(max_moves, 0, 2 ** 31 - 1, "walk: max_moves must be None or an integer >= 0")
    return tgt, thr, conn or 4, mm, _args.bounded_int(scratch_bytes, 0, None, "walk: scratch_bytes must be an integer >= 0")


def scratch_need(H, W):
    """Bytes of scratch ``walk`` needs per listed environment of a chunk: three bit planes and two halos of the bands."""
    bands = _args.band_count(H, W)
    return (bands * 16 * 24 + bands * 40 + 255) // 256 * 256


class WalkSpec:
    """A checked walk request: the outputs asked for with their shapes and dtypes, and the arrays the call reads."""

    def __init__(self, n_envs, H, W, target=("BURNING",), through=("UNBURNED",), envs=None, connectivity=4, passable=None, targets=None,
                 points=None, max_moves=None, plane=False, step=False, reached=False, levels=False, scratch_bytes=0):
        self.target, self.through, self.connectivity, self.max_moves, self.scratch = request(
            target, through, connectivity, max_moves, scratch_bytes, targets=targets is not None)
        self.envs = _args.env_list(envs, n_envs, "walk", none_all=True)
        n = self.n = int(self.envs.shape[0])
        want = dict(plane=plane, step=step, reached=reached, levels=levels)
        _args.flags("walk", **want)
        if not (plane or reached or levels) and points is None:
            raise ValueError("walk: nothing asked for (plane, reached, levels or points)")
        if step and points is None:
            raise ValueError("walk: step needs points")
        if step and self.connectivity == 8:
            raise ValueError("walk: step needs connectivity 4 (the four moves of an agent)")
        need = scratch_need(H, W)
        if 0 < self.scratch < need:
            raise ValueError(f"walk: scratch_bytes {self.scratch} is less than one environment's need ({need} bytes)")
        if W > 8192:
            raise ValueError(f"walk: grids wider than 8192 cells are not supported (width {W})")
        self.passable, self.passable_per_env = _args.dense_plane("walk", "passable", passable, n_envs, H, W)
        self.targets, self.targets_per_env = _args.dense_plane("walk", "targets", targets, n_envs, H, W)
        self.points, self.k = _args.query_points("walk", points, n)
        shapes = dict(moves=((n, H, W), "int32"), point_moves=((n, self.k), "int32"), point_step=((n, self.k), "int32"),
                      reached=((n,), "int32"), levels=((n,), "int32"))
        asked = dict(moves=bool(plane), point_moves=bool(self.k), point_step=bool(step), reached=bool(reached), levels=bool(levels))
        #: output name -> (shape, the torch dtype's name), in the order of ``sf_walk_out``
        self.outputs = {name: shapes[name] for name in shapes if asked[name]}

    def device_tensors(self):
        """The CUDA tensors the call reads (the caller checks they live on the handle's GPU)."""
        return [t for t in (self.passable, self.targets, self.points) if t is not None]

    def params(self):
        return SfWalkParams(target_mask=self.target, through_mask=self.through, connectivity=self.connectivity, k=self.k,
                            max_moves=self.max_moves, passable_per_env=self.passable_per_env, targets_per_env=self.targets_per_env,
                            passable=self.passable.data_ptr() if self.passable is not None else None,
                            targets=self.targets.data_ptr() if self.targets is not None else None,
                            points=self.points.data_ptr() if self.k else None, scratch_bytes=self.scratch)

    def out(self, tensors):
        """The ``sf_walk_out`` of the output tensors (name -> tensor, as ``outputs`` lists them)."""
        return SfWalkOut(**{name: t.data_ptr() for name, t in tensors.items()})
