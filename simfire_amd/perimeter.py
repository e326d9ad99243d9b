"""Fire perimeters: the arguments of ``perimeter`` checked and turned into ``sf_perimeter_params`` / ``sf_perimeter_out``
(include/simfire_hip.h), and ``rings``, which cuts the vertex list of a traced answer into polygons.

Pure Python: every check happens here, before a device call, so that a bad request raises ``ValueError`` the same way with or
without a GPU.  The lattice, the successor rule, the canonical order and the scratch are described in DESIGN.md section 27.
"""
import numpy as np

from . import _args
from ._lib import SfPerimeterOut, SfPerimeterParams  # noqa: F401

#: the default set: what has burned or is burning
DEFAULT_STATUS = ("BURNING", "BURNED")
#: the traced outputs, in the order of ``sf_perimeter_out``
TRACED = ("loops", "holes", "n_vertices", "vertices", "loop_start", "loop_area", "loop_edges")
MAX_WIDTH = 8192


def request(status=None, at_update=None, connectivity=None, simplify=True, scratch_bytes=0, member=False):
    """The checked scalar arguments of ``perimeter``: (status mask, at_update code, connectivity code, simplify, scratch_bytes).
    Exactly one source: ``status`` (a mask 1..63 or BurnStatus members, names or ints), a ``member`` plane, or ``at_update`` >= 0;
    with none of the three the set is BURNING | BURNED.  Connectivity ``None`` (code 0) is the simulation's ``diagonal_spread``."""
    given = (status is not None) + bool(member) + (at_update is not None)
    if given > 1:
        raise ValueError("perimeter: more than one source: give exactly one of status, member and at_update")
    mask, at = 0, -1
    if at_update is not None:
        at = _args.bounded_int(at_update, 0, 2 ** 31 - 2, "perimeter: at_update must be None or an update >= 0")
    elif not member:
        mask = _args.status_mask("perimeter", DEFAULT_STATUS if status is None else status)
    what = "perimeter: connectivity must be 4, 8 or None (the simulation's diagonal_spread)"
    conn = 0 if connectivity is None else _args.bounded_int(connectivity, 0, 8, what)
    if conn not in (0, 4, 8):
        raise ValueError(f"{what}, got {connectivity!r}")
    _args.flags("perimeter", simplify=simplify)
    return mask, at, conn, int(bool(simplify)), _args.bounded_int(scratch_bytes, 0, None, "perimeter: scratch_bytes must be an integer >= 0")


def scratch_need(H, W, max_edges):
    """Bytes of scratch a traced ``perimeter`` needs per listed environment of a chunk: the bit plane of the set, the edge words with
    their ranks and eight int32 arrays of ``max_edges``, rounded up to 256 - as the header states it."""
    H, W = int(H), int(W)
    return (8 * H * ((W + 63) // 64) + 12 * (H + 1) * ((W + 16) // 16) + 32 * int(max_edges) + 255) // 256 * 256


def default_capacities(H, W, max_edges=None, max_vertices=None, max_loops=None):
    """(max_edges, max_vertices, max_loops) with the defaults filled in: min(2 H W + 2, 2^18) edges, as many vertices, a quarter as
    many loops (a loop has four edges at least)."""
    me = min(2 * int(H) * int(W) + 2, 1 << 18) if max_edges is None else max_edges
    me = _args.bounded_int(me, 0, 2 ** 31 - 1, "perimeter: max_edges must be an integer >= 0")
    mv = _args.bounded_int(me if max_vertices is None else max_vertices, 0, 2 ** 31 - 1, "perimeter: max_vertices must be an integer >= 0")
    ml = _args.bounded_int(me // 4 if max_loops is None else max_loops, 0, 2 ** 31 - 1, "perimeter: max_loops must be an integer >= 0")
    return me, mv, ml


class PerimeterSpec:
    """A checked perimeter request: the outputs asked for with their shapes and dtypes, and the plane the call reads."""

    def __init__(self, n_envs, H, W, status=None, envs=None, member=None, at_update=None, connectivity=None, simplify=True, counts=True,
                 front=False, trace=False, max_edges=None, max_vertices=None, max_loops=None, scratch_bytes=0, arrival_on=True):
        self.status, self.at_update, self.connectivity, self.simplify, self.scratch = request(
            status, at_update, connectivity, simplify, scratch_bytes, member=member is not None)
        self.envs = _args.env_list(envs, n_envs, "perimeter", none_all=True)
        n = self.n = int(self.envs.shape[0])
        _args.flags("perimeter", counts=counts, front=front, trace=trace)
        if not (counts or front or trace):
            raise ValueError("perimeter: nothing asked for (counts, front or trace)")
        if self.at_update >= 0 and not arrival_on:
            raise ValueError("perimeter: at_update needs arrival recording (enable_arrival)")
        if W > MAX_WIDTH:
            raise ValueError(f"perimeter: grids wider than {MAX_WIDTH} cells are not supported (width {W})")
        self.max_edges, self.max_vertices, self.max_loops = default_capacities(H, W, max_edges, max_vertices, max_loops)
        if trace and (self.max_vertices == 0 or self.max_loops == 0):
            raise ValueError("perimeter: trace needs max_vertices > 0 and max_loops > 0")
        self.need = scratch_need(H, W, self.max_edges) if trace else 0
        if 0 < self.scratch < self.need:
            raise ValueError(f"perimeter: scratch_bytes {self.scratch} is less than one environment's need ({self.need} bytes)")
        self.member, self.member_per_env = _args.dense_plane("perimeter", "member", member, n_envs, H, W)
        shapes = dict(edges=((n,), "int32"), cells=((n,), "int32"), front=((n, H, W), "uint8"), loops=((n,), "int32"), holes=((n,), "int32"),
                      n_vertices=((n,), "int32"), vertices=((n, self.max_vertices, 2), "int32"), loop_start=((n, self.max_loops + 1), "int32"),
                      loop_area=((n, self.max_loops), "int32"), loop_edges=((n, self.max_loops), "int32"))
        asked = dict(edges=bool(counts), cells=bool(counts), front=bool(front), **{name: bool(trace) for name in TRACED})
        #: output name -> (shape, the torch dtype's name), in the order of ``sf_perimeter_out``
        self.outputs = {name: shapes[name] for name in shapes if asked[name]}

    def device_tensors(self):
        """The CUDA tensors the call reads (the caller checks they live on the handle's GPU)."""
        return [t for t in (self.member,) if t is not None]

    def params(self):
        return SfPerimeterParams(status_mask=self.status, at_update=self.at_update, connectivity=self.connectivity, simplify=self.simplify,
                                 member_per_env=self.member_per_env, max_edges=self.max_edges, max_vertices=self.max_vertices,
                                 max_loops=self.max_loops, member=self.member.data_ptr() if self.member is not None else None,
                                 scratch_bytes=self.scratch)

    def out(self, tensors):
        """The ``sf_perimeter_out`` of the output tensors (name -> tensor, as ``outputs`` lists them)."""
        return SfPerimeterOut(**{name: t.data_ptr() for name, t in tensors.items()})


def rings(vertices, loop_start, loop_area, loops=None):
    """The polygons of ONE environment's traced answer: a list of ``(ndarray[m, 2] of (x, y), is_hole)`` in canonical order.
    ``vertices`` [max_vertices, 2], ``loop_start`` [max_loops + 1] and ``loop_area`` [max_loops] as ``perimeter`` returns them (host
    arrays or tensors).  ``loops``: the number of loops; without it the list ends where the offsets stop increasing (``perimeter``
    zeroes ``loop_start`` in front of the call, so an answer that did not fit gives no ring)."""
    v, s, a = (np.asarray(x.cpu() if hasattr(x, "cpu") else x) for x in (vertices, loop_start, loop_area))
    if v.ndim != 2 or v.shape[1] != 2 or s.ndim != 1 or a.ndim != 1 or s.shape[0] != a.shape[0] + 1:
        raise ValueError("rings: vertices [m, 2], loop_start [loops + 1] and loop_area [loops] of one environment")
    out = []
    for l in range(a.shape[0] if loops is None else min(max(int(loops), 0), a.shape[0])):
        lo, hi = int(s[l]), int(s[l + 1])
        if hi <= lo or hi > v.shape[0] or lo < 0:
            break
        out.append((v[lo:hi].copy(), bool(a[l] < 0)))
    return out
