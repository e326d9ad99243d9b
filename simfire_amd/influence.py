"""Fire influence: the arguments of ``influence`` checked and turned into ``sf_influence_params`` / ``sf_influence_out``
(include/simfire_hip.h).

Pure Python: every check happens here, before a device call, so that a bad request raises ``ValueError`` the same way with or
without a GPU.  The semantics, the kernels and the scratch are described in DESIGN.md section 28.
"""
from . import _args
from ._lib import (SF_INFLUENCE_CYCLE, SF_INFLUENCE_PRED_HISTORY, SF_INFLUENCE_PRED_PLANE, SF_INFLUENCE_WEIGHT_NONE,  # noqa: F401
                   SF_INFLUENCE_WEIGHT_PLANE, SF_INFLUENCE_WEIGHT_VALUES, SfInfluenceOut, SfInfluenceParams)
from .travel import SRC_OFFSETS  # noqa: F401  (a parent code is an index into these)

#: the neighbours of ``FireSpreadGraph`` in the order of simfire/utils/graph.py:125-134 - bit j of a spread-graph parent mask
GRAPH_OFFSETS = ((+1, 0), (+1, +1), (0, +1), (-1, +1), (-1, 0), (-1, -1), (0, -1), (+1, -1))
#: bit j of a parent mask -> the parent code (index into ``SRC_OFFSETS``) of the same neighbour
BIT_TO_CODE = (3, 0, 1, 2, 4, 7, 6, 5)
#: the longest route a point may ask for
MAX_ROUTE = 1 << 20


def _round(b):
    return (int(b) + 255) // 256 * 256


def scratch_need(H, W, cells=True, weighted=False, value=False):
    """Bytes of scratch ``influence`` needs per listed environment of a chunk, every term rounded up to 256: the codes (N = H * W
    bytes), the child counters (4 N) and each accumulator that is no output of the call - 4 N without ``cells``, 8 N with weights
    and without ``value``."""
    n = int(H) * int(W)
    return _round(n) + _round(4 * n) + (0 if cells else _round(4 * n)) + (_round(8 * n) if weighted and not value else 0)


class InfluenceSpec:
    """A checked influence request: the outputs asked for with their shapes and dtypes, and the arrays the call reads."""

    def __init__(self, n_envs, H, W, pred=None, history=False, envs=None, weights=None, include=None, inclusive=False, points=None,
                 max_route=0, cells=True, value=False, pred_out=False, counts=False, scratch_bytes=0, graph_on=False, arrival_on=False,
                 values_on=False):
        _args.flags("influence", history=history, inclusive=inclusive, cells=cells, value=value, pred_out=pred_out, counts=counts)
        if history == (pred is not None):
            raise ValueError("influence: exactly one source: a pred plane, or history=True" + (" (both given)" if history else " (none given)"))
        if history and not (graph_on and arrival_on):
            raise ValueError("influence: history needs the spread graph and arrival recording (enable_spread_graph, enable_arrival)")
        self.history = bool(history)
        self.envs = _args.env_list(envs, n_envs, "influence", none_all=True)
        n = self.n = int(self.envs.shape[0])
        self.pred, self.pred_per_env = None, 0
        if pred is not None:
            self.pred = _args.cuda_tensor(pred, "influence: pred", ("int8",), [(H, W), (n, H, W)]).contiguous()
            self.pred_per_env = int(pred.dim() == 3)
        self.weights, self.weights_per_env, self.weight_mode = None, 0, SF_INFLUENCE_WEIGHT_NONE
        if isinstance(weights, str):
            if weights != "values":
                raise ValueError(f'influence: weights must be None, "values" or an int32 CUDA tensor, got {weights!r}')
            if not values_on:
                raise ValueError('influence: weights="values" needs a value plane (values_set)')
            self.weight_mode = SF_INFLUENCE_WEIGHT_VALUES
        elif weights is not None:
            self.weights = _args.cuda_tensor(weights, "influence: weights", ("int32",), [(H, W), (n_envs, H, W)]).contiguous()
            self.weights_per_env = int(weights.dim() == 3)
            self.weight_mode = SF_INFLUENCE_WEIGHT_PLANE
        weighted = self.weight_mode != SF_INFLUENCE_WEIGHT_NONE
        if value and not weighted:
            raise ValueError('influence: value needs weights ("values" or a tensor)')
        self.include, self.include_per_env = _args.dense_plane("influence", "include", include, n_envs, H, W)
        self.inclusive = int(inclusive)
        self.max_route = _args.bounded_int(max_route, 0, MAX_ROUTE, f"influence: max_route must be an integer in 0..{MAX_ROUTE}")
        self.points, self.k = _args.query_points("influence", points, n)
        if self.max_route and not self.k:
            raise ValueError("influence: max_route needs points")
        if not (cells or value or pred_out or counts or self.k):
            raise ValueError("influence: nothing asked for (cells, value, pred_out, counts or points)")
        self.scratch = _args.bounded_int(scratch_bytes, 0, None, "influence: scratch_bytes must be an integer >= 0")
        self.need = scratch_need(H, W, cells=cells, weighted=weighted, value=value)
        if 0 < self.scratch < self.need:
            raise ValueError(f"influence: scratch_bytes {self.scratch} is less than one environment's need ({self.need} bytes)")
        if W > 8192:
            raise ValueError(f"influence: grids wider than 8192 cells are not supported (width {W})")
        k, R = self.k, self.max_route
        shapes = dict(cells=((n, H, W), "int32"), value=((n, H, W), "int64"), pred=((n, H, W), "int8"), forest=((n,), "int32"),
                      roots=((n,), "int32"), cyclic=((n,), "int32"), point_cells=((n, k), "int32"), point_value=((n, k), "int64"),
                      point_route=((n, k, R), "int32"), point_hops=((n, k), "int32"))
        asked = dict(cells=cells, value=value, pred=pred_out, forest=counts, roots=counts, cyclic=counts, point_cells=bool(k),
                     point_value=bool(k) and weighted, point_route=bool(k) and R > 0, point_hops=bool(k) and R > 0)
        #: output name -> (shape, the torch dtype's name), in the order of ``sf_influence_out``
        self.outputs = {name: shapes[name] for name in shapes if asked[name]}

    def device_tensors(self):
        """The CUDA tensors the call reads (the caller checks they live on the handle's GPU)."""
        return [t for t in (self.pred, self.weights, self.include, self.points) if t is not None]

    def params(self):
        ptr = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
        return SfInfluenceParams(pred_source=SF_INFLUENCE_PRED_HISTORY if self.history else SF_INFLUENCE_PRED_PLANE,
                                 pred_per_env=self.pred_per_env, weight_mode=self.weight_mode, weights_per_env=self.weights_per_env,
                                 include_per_env=self.include_per_env, inclusive=self.inclusive, k=self.k, max_route=self.max_route,
                                 pred=ptr(self.pred), weights=ptr(self.weights), include=ptr(self.include),
                                 points=ptr(self.points) if self.k else None, scratch_bytes=self.scratch)

    def out(self, tensors):
        """The ``sf_influence_out`` of the output tensors (name -> tensor, as ``outputs`` lists them)."""
        return SfInfluenceOut(**{name: t.data_ptr() for name, t in tensors.items()})
