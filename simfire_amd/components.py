"""Connected components: the arguments of ``components`` checked and turned into ``sf_components_params`` / ``sf_components_out``
(include/simfire_hip.h).

Pure Python: every check happens here, before a device call, so that a bad request raises ``ValueError`` the same way with or
without a GPU.  The union-find, its phases and its scratch are described in DESIGN.md section 31.
"""
from . import _args
from ._lib import SF_COMPONENTS_MAX, SfComponentsOut, SfComponentsParams

#: bit 6 of ``touch``: the component has a cell on the grid's border (bits 0..5: an unselected neighbour of that BurnStatus)
TOUCH_BORDER = 64

#: the outputs a call can ask for by flag, in the order of ``sf_components_out`` (``point_label`` comes with ``points``)
FLAGS = ("count", "selected", "labels", "cells", "value", "first", "bbox", "touch", "largest")


def request(select=("BURNING",), connectivity=None, max_components=64, scratch_bytes=0):
    """The checked scalar arguments of ``components``: (select mask, connectivity code, max_components, scratch_bytes)."""
    sel = _args.status_mask("components", select, "select")
    conn = 0
    if connectivity is not None:
        what = "components: connectivity must be None (the simulation's diagonal_spread), 4 or 8"
        conn = _args.bounded_int(connectivity, 0, 8, what)
        if conn not in (0, 4, 8):
            raise ValueError(f"{what}, got {connectivity!r}")
    cap = _args.bounded_int(max_components, 1, SF_COMPONENTS_MAX, f"components: max_components must be an integer in 1..{SF_COMPONENTS_MAX}")
    return sel, conn, cap, _args.bounded_int(scratch_bytes, 0, None, "components: scratch_bytes must be an integer >= 0")


def _round(b):
    return (b + 255) // 256 * 256


def scratch_need(H, W, labels=False):
    """Bytes of scratch ``components`` needs per listed environment of a chunk: a head of 256 bytes, one bit per cell in rows of
    whole 64-bit words, a counter per row, four bytes per cell for the ranks (then the sizes), and - unless the ``labels`` output is
    asked for, which then is the label plane - four more per cell; each rounded up to 256."""
    H, W = int(H), int(W)
    n = H * W
    return 256 + _round(H * ((W + 63) // 64) * 8) + _round(4 * (H + 1)) + _round(4 * n) + (0 if labels else _round(4 * n))


def mask_of(status):
    """The ``touch`` bits of a set of BurnStatus values (members, names, ints, or a mask)."""
    return _args.status_mask("components", status, "status")


class ComponentsSpec:
    """A checked components request: the outputs asked for with their shapes and dtypes, and the arrays the call reads."""

    def __init__(self, n_envs, H, W, values_on, select=("BURNING",), envs=None, connectivity=None, member=None, points=None,
                 max_components=64, count=True, labels=False, cells=False, value=False, first=False, bbox=False, touch=False, largest=False,
                 selected=False, scratch_bytes=0):
        self.select, self.connectivity, self.cap, self.scratch = request(select, connectivity, max_components, scratch_bytes)
        self.envs = _args.env_list(envs, n_envs, "components", none_all=True)
        n = self.n = int(self.envs.shape[0])
        want = dict(count=count, selected=selected, labels=labels, cells=cells, value=value, first=first, bbox=bbox, touch=touch,
                    largest=largest)
        _args.flags("components", **want)
        if not any(want.values()) and points is None:
            raise ValueError("components: nothing asked for (" + ", ".join(FLAGS) + " or points)")
        if value and not values_on:
            raise ValueError("components: value needs a value plane (values_set)")
        need = scratch_need(H, W, labels)
        if 0 < self.scratch < need:
            raise ValueError(f"components: scratch_bytes {self.scratch} is less than one environment's need ({need} bytes)")
        if W > 8192:
            raise ValueError(f"components: grids wider than 8192 cells are not supported (width {W})")
        self.member, self.per_env = _args.dense_plane("components", "member", member, n_envs, H, W)
        self.points, self.k = _args.query_points("components", points, n)
        cap, i32 = self.cap, "int32"
        shapes = dict(count=((n,), i32), selected=((n,), i32), labels=((n, H, W), i32), cells=((n, cap), i32), value=((n, cap), "int64"),
                      first=((n, cap), i32), bbox=((n, cap, 4), i32), touch=((n, cap), i32), largest=((n, 2), i32),
                      point_label=((n, self.k), i32))
        want["point_label"] = bool(self.k)
        #: output name -> (shape, the torch dtype's name), in the order of ``sf_components_out``
        self.outputs = {name: shapes[name] for name in shapes if want[name]}

    def device_tensors(self):
        """The CUDA tensors the call reads (the caller checks they live on the handle's GPU)."""
        return [t for t in (self.member, self.points) if t is not None]

    def params(self):
        return SfComponentsParams(select_mask=self.select, connectivity=self.connectivity, k=self.k, max_components=self.cap,
                                  member_per_env=self.per_env, member=self.member.data_ptr() if self.member is not None else None,
                                  points=self.points.data_ptr() if self.k else None, scratch_bytes=self.scratch)

    def out(self, tensors):
        """The ``sf_components_out`` of the output tensors (name -> tensor, as ``outputs`` lists them)."""
        return SfComponentsOut(**{name: t.data_ptr() for name, t in tensors.items()})


def pockets_summary(r, fire_mask, cap):
    """What ``pockets`` makes of a ``components`` result ``r`` (``count``, ``cells``, ``touch``, perhaps ``value``) with torch on the
    device: ``exposed`` - the pocket touches a cell of the fire -, the sums over the pockets that do not, and ``truncated``."""
    import torch
    exposed = (r["touch"] & int(fire_mask)) != 0
    rows = torch.arange(cap, device=r["count"].device)[None, :] < r["count"][:, None]      # (rows past the count are no pockets)
    safe = rows & ~exposed
    out = dict(count=r["count"], cells=r["cells"], exposed=exposed & rows, safe_cells=(r["cells"] * safe).sum(dim=1),
               truncated=r["count"] > cap)
    if "value" in r:
        out["value"] = r["value"]
        out["safe_value"] = (r["value"] * safe).sum(dim=1)
    return out
