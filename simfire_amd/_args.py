"""Argument checks shared by the binding (``engine.py``) and the request classes (``observe.py``, ``render.py``, ``ensemble.py``
and the seven queries ``distance.py``, ``reach.py``, ``walk.py``, ``travel.py``, ``behavior.py``, ``perimeter.py``,
``influence.py``).

Pure Python on NumPy; torch is imported inside the functions that are handed a tensor.  Every check raises before a device call,
so a bad request fails the same way with or without a GPU.  ``who`` names the caller in the message (``"reach"`` gives
``"reach: ..."``).
"""
import numpy as np


def _prefix(who):
    return f"{who}: " if who else ""


def is_tensor(x):
    return hasattr(x, "data_ptr") and hasattr(x, "is_cuda")


def env_range(e, n_envs, who="", name="envs", exc=ValueError):
    """Every environment number of ``e`` lies in 0..n_envs - 1, or ``exc``."""
    if e.size and (e.min() < 0 or e.max() >= n_envs):
        bad = int(e[(e < 0) | (e >= n_envs)][0])
        raise exc(f"{_prefix(who)}{name} holds environment {bad}, outside 0..{n_envs - 1}")


def env_list(envs, n_envs=None, who="", name="envs", lenient=False, scalar=False, none_all=False, empty=True, ndim=1):
    """Environment numbers as a contiguous int32 array of ``ndim`` dimensions.

    ``lenient``: the legacy form - a scalar counts as a list of one and whatever casts to int32 passes (a float is truncated);
    otherwise the entries must be integers.  ``scalar``: a scalar counts as a list of one in the strict form too.  ``none_all``:
    ``None`` stands for every environment in order (needs ``n_envs``).  ``empty``: whether a list of none is allowed.  With
    ``n_envs`` the numbers are checked against it (``ValueError``); without, that is left to the caller (``env_range``, which
    takes the exception type) or to the library."""
    if envs is None and none_all:
        return np.arange(n_envs, dtype=np.int32).reshape((1,) * (ndim - 1) + (-1,))
    a = np.asarray(envs)
    if lenient or scalar:
        a = np.atleast_1d(a)
    if lenient:
        a = np.ascontiguousarray(a, dtype=np.int32)
    if a.ndim != ndim or (a.size and a.dtype.kind not in "iu") or not (empty or a.size):
        form = "list" if ndim == 1 else f"{ndim}-D array [groups, members]"
        raise ValueError(f"{_prefix(who)}{name} must be a {'' if empty else 'non-empty '}{form} of environment numbers")
    a = np.ascontiguousarray(a, dtype=np.int32)
    if n_envs is not None:
        env_range(a, n_envs, who, name)
    return a


def status_mask(who, status, what="status"):
    """A set of BurnStatus values as the mask the library takes (bit s = BurnStatus s, 1..63): ``status`` is that mask, a member,
    a name, or an iterable of members, names or ints.  ``ValueError`` (named after the caller, ``who``) on anything else."""
    from .enums import BurnStatus

    def bit(s):
        if isinstance(s, str):
            if s not in BurnStatus.__members__:
                raise ValueError(f"{who}: unknown BurnStatus name {s!r}")
            return 1 << int(BurnStatus[s])
        return 1 << bounded_int(s, 0, 5, f"{who}: no BurnStatus (a member, a name or 0..5)")
    if isinstance(status, (int, np.integer)) and not isinstance(status, (bool, BurnStatus)):
        mask = int(status)
    elif isinstance(status, (str, BurnStatus)):
        mask = bit(status)
    else:
        try:
            items = list(status)
        except TypeError:
            raise ValueError(f"{who}: {what} must be a mask 1..63 or BurnStatus members, names or ints, got {status!r}") from None
        mask = 0
        for s in items:
            mask |= bit(s)
    if not 1 <= mask <= 63:
        raise ValueError(f"{who}: the {what} mask {mask} selects nothing or more than BurnStatus 0..5 (1..63)")
    return mask


def bounded_int(v, lo, hi, what):
    """``v`` as an int if it is an integer (no bool, no float) in ``lo..hi`` (``None``: unbounded), else ``ValueError(what, got v)``."""
    if isinstance(v, (bool, float)) or not isinstance(v, (int, np.integer)) or (lo is not None and int(v) < lo) \
            or (hi is not None and int(v) > hi):
        raise ValueError(f"{what}, got {v!r}")
    return int(v)


def cells(xy, shape, H, W, who, what="cell"):
    """Host cells int32 ``shape`` = [..., 2] = (x, y), every one on the ``H`` x ``W`` grid."""
    a = np.asarray(xy)
    if a.dtype.kind not in "iu":
        raise ValueError(f"{who}: {what}s must be integers, got {a.dtype}")
    if a.shape != tuple(shape):
        raise ValueError(f"{who}: {what}s must have shape {tuple(shape)}, got {a.shape}")
    a = np.ascontiguousarray(a, dtype=np.int32)
    bad = np.argwhere((a[..., 0] < 0) | (a[..., 0] >= W) | (a[..., 1] < 0) | (a[..., 1] >= H))
    if bad.size:
        i = tuple(int(v) for v in bad[0])
        raise ValueError(f"{who}: {what} ({a[i][0]}, {a[i][1]}) of entry {i if len(i) > 1 else i[0]} is outside the {H}x{W} grid")
    return a


def ignite_rows(points, n_envs, H, W, who):
    """Host ignition rows, ``[n, 3]`` = (env, x, y) or ``[n, 4]`` with a reserved 0 behind, as the contiguous int32 ``[n, 4]`` array
    the library takes: an environment outside 0..n_envs - 1 is an ``IndexError``, anything else wrong a ``ValueError`` - as
    ``reset_envs`` tells them apart.  An empty list of either width passes."""
    a = np.asarray(points)
    if a.size == 0 and a.ndim <= 2:
        return np.zeros((0, 4), dtype=np.int32)
    if a.dtype.kind not in "iu":
        raise ValueError(f"{who}: rows must be integers, got {a.dtype}")
    if a.ndim != 2 or a.shape[1] not in (3, 4):
        raise ValueError(f"{who}: rows must have shape (n, 3) = (env, x, y) or (n, 4), got {a.shape}")
    if a.shape[1] == 4 and (a[:, 3] != 0).any():
        raise ValueError(f"{who}: the fourth field of row {int(np.flatnonzero(a[:, 3] != 0)[0])} is reserved and must be 0")
    if a.min() < -2 ** 31 or a.max() >= 2 ** 31:
        raise ValueError(f"{who}: rows hold values outside int32")
    env_range(a[:, 0], n_envs, who, "rows", exc=IndexError)
    cells(a[:, 1:3], (a.shape[0], 2), H, W, who, "ignition")
    q = np.zeros((a.shape[0], 4), dtype=np.int32)
    q[:, :3] = a[:, :3]
    return q


def box(b, H, W, who, name):
    """(x0, y0, x1, y1), inclusive, on the grid, as a list of ints."""
    b = [int(v) for v in b]
    if len(b) != 4:
        raise ValueError(f"{who}: {name} is (x0, y0, x1, y1), inclusive")
    if b[0] < 0 or b[1] < 0 or b[2] >= W or b[3] >= H or b[0] > b[2] or b[1] > b[3]:
        raise ValueError(f"{who}: {name} {tuple(b)} is not x0 <= x1, y0 <= y1 on the {H}x{W} grid")
    return b


def cuda_tensor(t, what, dtypes, shapes=None, device=None, contiguous=False):
    """``t`` if it is a torch CUDA tensor of one of ``dtypes`` (names: "int32") and of one of ``shapes`` (tuples; ``None`` in one
    stands for any extent), on ``device`` and contiguous where those are asked for; else a ``ValueError`` that says all of it."""
    ok = is_tensor(t) and t.is_cuda
    if ok:
        import torch
        shape = tuple(t.shape)
        ok = isinstance(t, torch.Tensor) and t.dtype in [getattr(torch, d) for d in dtypes] \
            and (shapes is None or any(len(s) == len(shape) and all(w is None or w == v for w, v in zip(s, shape)) for s in shapes)) \
            and (device is None or t.device == device) and (not contiguous or t.is_contiguous())
    if not ok:
        forms = " or ".join("(" + ", ".join("k" if w is None else str(w) for w in s) + ("," if len(s) == 1 else "") + ")" for s in shapes or ())
        raise ValueError(f"{what} must be a {'contiguous ' if contiguous else ''}CUDA {' / '.join(dtypes)} tensor"
                         + (f" of shape {forms}" if forms else "") + (f" on {device}" if device is not None else ""))
    return t


def env_mask(mask, n_envs, who):
    """A device mask over the environments: a CUDA uint8 / bool tensor [n_envs], returned contiguous."""
    return cuda_tensor(mask, f"{who}: mask", ("uint8", "bool"), [(n_envs,)]).contiguous()


def points(x, n, last, name, host=True, k_range=None):
    """Entries per environment, [n, last] (``last`` = 2) or [n, k, last] with k in ``k_range`` = (lo, hi): a CUDA int32 tensor or,
    with ``host``, a host array of integers -> (contiguous tensor / int32 array, on_device)."""
    form = (n, last) if last == 2 else (n, None, last)
    if is_tensor(x) or not host:
        x, dev = cuda_tensor(x, name, ("int32",), [form]).contiguous(), True
    else:
        a = np.asarray(x)
        if a.dtype.kind not in "iu" and not (a.size == 0 and a.dtype.kind == "f"):
            raise ValueError(f"{name} must hold integers, got dtype {a.dtype}")
        if a.ndim != len(form) or a.shape[0] != n or a.shape[-1] != last:
            raise ValueError(f"{name} must have the shape [{n}, {'k, ' if last == 3 else ''}{last}], got {a.shape}")
        if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
            raise ValueError(f"{name} holds values outside int32")
        x, dev = np.ascontiguousarray(a, dtype=np.int32), False
    if k_range is not None and not k_range[0] <= x.shape[1] <= k_range[1]:
        raise ValueError(f"{name}: at least {k_range[0]} and at most {k_range[1]} entries per environment, got {x.shape[1]}")
    return x, dev


def query_points(who, x, n):
    """The points of a query (``distance``, ``reach``, ``walk``, ``travel``, ``behavior``): ``None``, or a CUDA int32 tensor [n, k, 3] =
    (column, row, id) with k in 1..SF_DIST_MAX_POINTS -> (contiguous tensor or ``None``, k)."""
    from ._lib import SF_DIST_MAX_POINTS
    if x is None:
        return None, 0
    x = points(x, n, 3, f"{who}: points", host=False, k_range=(1, SF_DIST_MAX_POINTS))[0]
    return x, int(x.shape[1])


def flags(who, **want):
    """Every keyword is ``True`` or ``False`` (a bool, not something truthy), or ``ValueError``."""
    for name, flag in want.items():
        if not isinstance(flag, (bool, np.bool_)):
            raise ValueError(f"{who}: {name} must be True or False, got {flag!r}")


def dense_plane(who, name, t, n_envs, H, W):
    """A uint8 plane of a query: ``None``, or a CUDA tensor [H, W] (one for every environment) or [n_envs, H, W] -> (contiguous
    tensor or ``None``, 1 if it is per environment else 0)."""
    if t is None:
        return None, 0
    return cuda_tensor(t, f"{who}: {name}", ("uint8",), [(H, W), (n_envs, H, W)]).contiguous(), int(t.dim() == 3)


def band_count(H, W):
    """Bands of 16 rows x 64 columns on an ``H`` x ``W`` grid (rows of pitch roundup(W, 16)): what the scratch of ``reach`` and
    ``walk`` is counted in."""
    return ((H + 15) // 16) * (((W + 15) // 16 * 16 + 63) // 64)
