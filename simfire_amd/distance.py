"""Distance fields: the arguments of ``distance`` checked and turned into ``sf_dist_params`` (include/simfire_hip.h).

Pure Python: every check happens here, before a device call, so that a bad request raises ``ValueError`` the same way with or
without a GPU.  The kernels and the scratch budget are described in DESIGN.md section 22.
"""
import numpy as np

from . import _args
from ._lib import SF_DIST_F32, SF_DIST_I32, SfDistParams


def request(status, max_dist=None, max_d2=None, dtype="float32", scale=1.0, scratch_bytes=0):
    """The checked scalar arguments of ``distance``: (status mask, max_d2, dtype code, scale, scratch_bytes)."""
    mask = _args.status_mask("distance", status)
    if max_dist is not None and max_d2 is not None:
        raise ValueError("distance: give max_dist or max_d2, not both")
    d2 = 0
    if max_dist is not None:
        d2 = _args.bounded_int(max_dist, 1, 46340, "distance: max_dist must be an integer number of cells 1..46340 or None") ** 2
    elif max_d2 is not None:
        d2 = _args.bounded_int(max_d2, 1, 2 ** 31 - 1, "distance: max_d2 must be an integer 1..2**31 - 1 or None")
    name = getattr(dtype, "name", None) or str(dtype).replace("torch.", "")
    if name not in ("int32", "float32"):
        raise ValueError(f"distance: dtype must be 'int32' or 'float32', got {dtype!r}")
    try:
        sc = float(scale)
    except (TypeError, ValueError):
        raise ValueError(f"distance: scale must be a number, got {scale!r}") from None
    if not np.isfinite(sc) or sc <= 0.0:
        raise ValueError(f"distance: scale must be finite and > 0, got {scale!r}")
    scratch = _args.bounded_int(scratch_bytes, 0, None, "distance: scratch_bytes must be an integer >= 0")
    return mask, d2, (SF_DIST_I32 if name == "int32" else SF_DIST_F32), sc, scratch


class DistSpec:
    """A checked distance request: output shape and dtype, and the arrays the call reads."""

    def __init__(self, n_envs, H, W, status, envs=None, max_dist=None, points=None, dtype="float32", scale=1.0, out=None,
                 scratch_bytes=0, max_d2=None):
        self.mask, self.max_d2, self.code, self.scale, self.scratch = request(status, max_dist, max_d2, dtype, scale, scratch_bytes)
        self.envs = _args.env_list(envs, n_envs, "distance", none_all=True)
        n = self.n = int(self.envs.shape[0])
        self.points, self.k = _args.query_points("distance", points, n)
        self.shape = (n, self.k) if self.k else (n, H, W)
        self.dtype = "int32" if self.code == SF_DIST_I32 else "float32"         # (the torch dtype's name)
        if out is not None:
            _args.cuda_tensor(out, "distance: out", (self.dtype,), [self.shape], contiguous=True)
        plane = H * ((W + 15) // 16 * 16) * 2
        if 0 < self.scratch < plane:
            raise ValueError(f"distance: scratch_bytes {self.scratch} is less than one environment's plane ({plane} bytes)")

    def device_tensors(self):
        """The CUDA tensors the call reads (the caller checks they live on the handle's GPU)."""
        return [self.points] if self.k else []

    def params(self):
        return SfDistParams(status_mask=self.mask, max_d2=self.max_d2, dtype=self.code, k=self.k, scale=self.scale,
                            points=self.points.data_ptr() if self.k else None, scratch_bytes=self.scratch)
