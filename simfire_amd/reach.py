"""Reach of the fire: the arguments of ``reach`` checked and turned into ``sf_reach_params`` / ``sf_reach_out``
(include/simfire_hip.h).

Pure Python: every check happens here, before a device call, so that a bad request raises ``ValueError`` the same way with or
without a GPU.  The flood fill and its scratch are described in DESIGN.md section 23.
"""
from . import _args
from ._lib import SfReachOut, SfReachParams


def request(source=("BURNING",), through=("UNBURNED",), connectivity=None, max_rounds=0, scratch_bytes=0):
    """The checked scalar arguments of ``reach``: (source mask, through mask, connectivity code, max_rounds, scratch_bytes)."""
    src = _args.status_mask("reach", source, "source")
    thr = _args.status_mask("reach", through, "through")
    if src & thr:
        raise ValueError(f"reach: source (mask {src}) and through (mask {thr}) must not share a BurnStatus")
    conn = 0
    if connectivity is not None:
        what = "reach: connectivity must be None (the simulation's diagonal_spread), 4 or 8"
        conn = _args.bounded_int(connectivity, 0, 8, what)
        if conn not in (0, 4, 8):
            raise ValueError(f"{what}, got {connectivity!r}")
    mr = _args.bounded_int(max_rounds, 0, 2 ** 31 - 1, "reach: max_rounds must be an integer >= 0")
    return src, thr, conn, mr, _args.bounded_int(scratch_bytes, 0, None, "reach: scratch_bytes must be an integer >= 0")


def scratch_need(H, W):
    """Bytes of scratch ``reach`` needs per listed environment of a chunk: two bit planes and the halo of the bands."""
    bands = _args.band_count(H, W)
    return (bands * 16 * 16 + bands * 20 + 255) // 256 * 256


class ReachSpec:
    """A checked reach request: the outputs asked for with their shapes and dtypes, and the arrays the call reads."""

    def __init__(self, n_envs, H, W, values_on, source=("BURNING",), through=("UNBURNED",), envs=None, connectivity=None, passable=None,
                 points=None, count=True, value=False, mask=False, seeds=False, rounds=False, max_rounds=0, scratch_bytes=0):
        self.source, self.through, self.connectivity, self.max_rounds, self.scratch = request(source, through, connectivity, max_rounds,
                                                                                              scratch_bytes)
        self.envs = _args.env_list(envs, n_envs, "reach", none_all=True)
        n = self.n = int(self.envs.shape[0])
        want = dict(count=count, value=value, mask=mask, seeds=seeds, rounds=rounds)
        _args.flags("reach", **want)
        if not any(want.values()) and points is None:
            raise ValueError("reach: nothing asked for (count, value, mask, seeds, rounds or points)")
        if value and not values_on:
            raise ValueError("reach: value needs a value plane (values_set)")
        need = scratch_need(H, W)
        if 0 < self.scratch < need:
            raise ValueError(f"reach: scratch_bytes {self.scratch} is less than one environment's need ({need} bytes)")
        if W > 8192:
            raise ValueError(f"reach: grids wider than 8192 cells are not supported (width {W})")
        self.passable, self.per_env = _args.dense_plane("reach", "passable", passable, n_envs, H, W)
        self.points, self.k = _args.query_points("reach", points, n)
        shapes = dict(count=((n,), "int32"), value=((n,), "int64"), mask=((n, H, W), "uint8"), seeds=((n,), "int32"),
                      point_in=((n, self.k), "int32"), rounds=((n,), "int32"))
        want["point_in"] = bool(self.k)
        #: output name -> (shape, the torch dtype's name), in the order of ``sf_reach_out``
        self.outputs = {name: shapes[name] for name in shapes if want[name]}

    def device_tensors(self):
        """The CUDA tensors the call reads (the caller checks they live on the handle's GPU)."""
        return [t for t in (self.passable, self.points) if t is not None]

    def params(self):
        return SfReachParams(source_mask=self.source, through_mask=self.through, connectivity=self.connectivity, k=self.k,
                             max_rounds=self.max_rounds, passable_per_env=self.per_env,
                             passable=self.passable.data_ptr() if self.passable is not None else None,
                             points=self.points.data_ptr() if self.k else None, scratch_bytes=self.scratch)

    def out(self, tensors):
        """The ``sf_reach_out`` of the output tensors (name -> tensor, as ``outputs`` lists them)."""
        return SfReachOut(**{name: t.data_ptr() for name, t in tensors.items()})
