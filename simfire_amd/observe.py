"""Observation tensors for a policy: the arguments of ``observe`` checked and turned into ``sf_obs_params`` (include/simfire_hip.h).

Pure Python: every check happens here, before a device call, so that a bad request raises ``ValueError`` the same way with or
without a GPU.  The kernel (``k_observe``, simfire_amd/csrc/sf_obs_kernels.h) and the evaluation order are described in DESIGN.md
section 12; the test suite restates them in NumPy.
"""
from typing import Dict, Optional, Sequence, Union

import numpy as np

from . import _args
from .enums import BurnStatus

#: the attribute planes of ``get_attribute_data()`` in the order of ``supported_attributes()`` (simfire/sim/simulation.py:317-332)
ATTRIBUTES = ("w_0", "sigma", "delta", "M_x", "elevation", "wind_speed", "wind_direction")

#: channel name -> SF_OBS_* code
CHANNELS: Dict[str, int] = {"fire_map": 0}
CHANNELS.update({f"burn_status:{s.name}": 1 + int(s) for s in BurnStatus})
CHANNELS.update({name: 7 + i for i, name in enumerate(ATTRIBUTES)})
CHANNELS["agent_positions"] = 14

MAX_CHANNELS = 32
MAX_AGENTS = 256
MAX_POOL = 128
POOL_MODES = {"mean": 0, "max": 1}


def _torch_dtype(dtype):
    import torch
    if dtype in (None, torch.float32, "float32"):
        return torch.float32
    if dtype in (torch.bfloat16, "bfloat16"):
        return torch.bfloat16
    raise ValueError(f"dtype must be torch.float32 or torch.bfloat16, got {dtype!r}")


class ObsSpec:
    """A checked observation request: codes, pool modes, output shape and the arrays the call reads."""

    def __init__(self, channels: Sequence[str], n_envs: int, H: int, W: int, envs=None, normalize: bool = True, pool: int = 1,
                 pool_mode: Union[str, Dict[str, str]] = "mean", crop=None, centers=None, agents=None, pad: float = 0.0,
                 dtype=None, out=None):
        if isinstance(channels, str) or not isinstance(channels, Sequence):
            raise ValueError("channels must be a list of channel names")
        channels = list(channels)
        if not 1 <= len(channels) <= MAX_CHANNELS:
            raise ValueError(f"1 to {MAX_CHANNELS} channels, got {len(channels)}")
        for c in channels:
            if c not in CHANNELS:
                raise ValueError(f"unknown channel {c!r}; known: {', '.join(CHANNELS)}")
        self.channels = channels
        self.codes = [CHANNELS[c] for c in channels]

        if isinstance(pool_mode, str):
            if pool_mode not in POOL_MODES:
                raise ValueError(f"pool_mode must be 'mean' or 'max', got {pool_mode!r}")
            self.modes = [POOL_MODES[pool_mode]] * len(channels)
        elif isinstance(pool_mode, dict):
            for k, v in pool_mode.items():
                if k not in channels:
                    raise ValueError(f"pool_mode names {k!r}, which is not one of the channels")
                if v not in POOL_MODES:
                    raise ValueError(f"pool_mode of {k!r} must be 'mean' or 'max', got {v!r}")
            self.modes = [POOL_MODES[pool_mode.get(c, "mean")] for c in channels]
        else:
            raise ValueError("pool_mode must be 'mean', 'max' or a dict {channel: mode}")

        self.envs = _args.env_list(envs, n_envs, none_all=True, empty=False)
        n = self.n = int(self.envs.shape[0])

        self.pool = _args.bounded_int(pool, None, None, "pool must be an integer")
        if not 1 <= self.pool <= MAX_POOL:
            raise ValueError(f"pool must be in 1..{MAX_POOL}, got {self.pool}")
        self.normalize = bool(normalize)
        self.pad = float(pad)

        if crop is None:
            if centers is not None:
                raise ValueError("centers are only used with a crop")
            self.crop = None
            eh, ew = H, W
            self.centers, self.centers_device = None, False
        else:
            if not isinstance(crop, (tuple, list)) or len(crop) != 2:
                raise ValueError("crop must be (height, width)")
            ch, cw = (_args.bounded_int(v, None, None, f"crop {name} must be an integer") for v, name in zip(crop, ("height", "width")))
            if not (1 <= ch <= 65535 and 1 <= cw <= 65535):
                raise ValueError(f"crop must be positive (at most 65535), got {(ch, cw)}")
            if centers is None:
                raise ValueError("a crop needs centers [n, 2] = (column, row)")
            self.crop = (ch, cw)
            eh, ew = ch, cw
            self.centers, self.centers_device = _args.points(centers, n, 2, "centers")
        if eh % self.pool or ew % self.pool:
            raise ValueError(f"the {'cropped ' if crop else ''}extent {eh} x {ew} is not divisible by pool {self.pool}")

        if agents is None:
            self.agents, self.agents_device, self.k = None, False, 0
        else:
            self.agents, self.agents_device = _args.points(agents, n, 3, "agents", k_range=(0, MAX_AGENTS))
            self.k = int(self.agents.shape[1])

        self.dtype = _torch_dtype(dtype)
        self.shape = (n, len(channels), eh // self.pool, ew // self.pool)
        if out is not None:
            if not _args.is_tensor(out) or not out.is_cuda:
                raise ValueError("out must be a CUDA tensor")
            if tuple(out.shape) != self.shape or out.dtype != self.dtype or not out.is_contiguous():
                raise ValueError(f"out must be a contiguous {self.dtype} tensor of shape {self.shape}, got "
                                 f"{out.dtype} {tuple(out.shape)}{'' if out.is_contiguous() else ' (not contiguous)'}")
        self.out = out

    def device_tensors(self):
        """The CUDA tensors the call reads (the caller checks they live on the handle's GPU)."""
        return [t for t, d in ((self.centers, self.centers_device), (self.agents, self.agents_device)) if d]

    def params(self):
        """The ``sf_obs_params`` of this request (host arrays are referenced, not copied: keep the spec alive across the call)."""
        from ._lib import SfObsParams
        p = SfObsParams()
        p.n_channels = len(self.codes)
        for i, (c, m) in enumerate(zip(self.codes, self.modes)):
            p.channels[i] = c
            p.pool_mode[i] = m
        p.normalize = int(self.normalize)
        p.pool = self.pool
        p.crop_h, p.crop_w = self.crop if self.crop else (0, 0)
        import torch
        p.dtype = 1 if self.dtype == torch.bfloat16 else 0
        p.pad = self.pad
        if self.centers is not None:
            p.centers_device = int(self.centers_device)
            p.centers = self.centers.data_ptr() if self.centers_device else self.centers.ctypes.data
        if self.agents is not None and self.k:
            p.agents_k = self.k
            p.agents_device = int(self.agents_device)
            p.agents = self.agents.data_ptr() if self.agents_device else self.agents.ctypes.data
        return p


def agents_from_map(agent_positions: np.ndarray, max_agents: Optional[int] = None) -> np.ndarray:
    """``agent_positions`` (an [H, W] map of agent ids) as the entry list ``observe`` takes: int32 [1, k, 3] = (column, row, id), one
    entry per non-zero cell.  Every id must sit on one cell and be positive (the entry list shows what ``update_agent_positions``
    leaves on a fresh map, where that is so)."""
    a = np.asarray(agent_positions)
    rows, cols = np.nonzero(a)
    ids = a[rows, cols].astype(np.int64)
    if ids.size and (ids.min() <= 0 or ids.max() >= 2 ** 31):
        raise ValueError("agent_positions holds ids outside 1..2^31-1")
    if np.unique(ids).size != ids.size:
        raise ValueError("agent_positions holds an id on more than one cell")
    cap = MAX_AGENTS if max_agents is None else max_agents
    if ids.size > cap:
        raise ValueError(f"agent_positions holds {ids.size} agents, observe takes at most {cap}")
    return np.stack([cols, rows, ids], axis=1).astype(np.int32).reshape(1, -1, 3)
