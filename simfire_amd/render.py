"""Frames of environments: the arguments of ``render`` checked and turned into ``sf_render_params`` (include/simfire_hip.h).

Pure Python: every check happens here, before a device call, so that a bad request raises ``ValueError`` the same way with or
without a GPU.  The kernels (``k_render_bg``, ``k_render``: simfire_amd/csrc/sf_render_kernels.h) and the frame are specified in
DESIGN.md section 14; the test suite restates them in NumPy.
"""
import numpy as np

from . import _args

MODES = {"nearest": 0, "mean": 1, "sprites": 2}
BACKGROUNDS = {"fuel": 0, "white": 1}
MAX_SCALE = 64
MAX_AGENTS = 256
#: the terrain colour functional fuel is blended from (``background="fuel"``) unless ``terrain_rgb`` says otherwise: this
#: project's own choice of a grass green
TERRAIN_RGB = (96, 128, 56)


class RenderSpec:
    """A checked render request: output shape and the arrays the call reads."""

    def __init__(self, n_envs: int, H: int, W: int, envs=None, scale: int = 1, mode=None, background: str = "fuel",
                 contours: bool = True, terrain_rgb=None, agents=None, channels_last: bool = True, history=None, out=None):
        self.envs = _args.env_list(envs, n_envs, scalar=True, none_all=True)
        n = self.n = int(self.envs.size)
        self.scale = _args.bounded_int(scale, None, None, "scale must be an integer")
        if not 1 <= self.scale <= MAX_SCALE:
            raise ValueError(f"scale must be 1..{MAX_SCALE}, got {self.scale}")
        if mode is None:
            mode = "sprites" if self.scale > 1 else "nearest"
        if mode not in MODES:
            raise ValueError(f"mode must be one of {sorted(MODES)}, got {mode!r}")
        self.mode = mode
        if background not in BACKGROUNDS:
            raise ValueError(f"background must be one of {sorted(BACKGROUNDS)}, got {background!r}")
        self.background = background
        if not isinstance(contours, (bool, np.bool_)):
            raise ValueError(f"contours must be True or False, got {contours!r}")
        self.contours = bool(contours)
        rgb = TERRAIN_RGB if terrain_rgb is None else tuple(terrain_rgb)
        if len(rgb) != 3:
            raise ValueError(f"terrain_rgb must be three integers 0..255, got {terrain_rgb!r}")
        self.terrain_rgb = tuple(_args.bounded_int(c, 0, 255, "terrain_rgb must be three integers 0..255") for c in rgb)
        self.channels_last = bool(channels_last)
        if history is None:
            self.source, self.first, self.count = 0, 0, 1
        else:
            first, count = history
            what = "history frames must be integers (first >= 0, count >= 1)"
            self.source, self.first, self.count = 1, _args.bounded_int(first, 0, None, what), _args.bounded_int(count, 1, None, what)
        if agents is None:
            self.agents, self.agents_device, self.k = None, False, 0
        else:
            self.agents, self.agents_device = _args.points(agents, n, 3, "agents", k_range=(0, MAX_AGENTS))
            self.k = int(self.agents.shape[1])
        self.oh, self.ow = -(-H // self.scale), -(-W // self.scale)
        frames = n * self.count
        self.shape = (frames, self.oh, self.ow, 3) if self.channels_last else (frames, 3, self.oh, self.ow)
        if out is not None:
            _args.cuda_tensor(out, "out", ("uint8",), [self.shape], contiguous=True)

    def device_tensors(self):
        """The tensors the call reads on the device (kept alive until the handle's stream got there in async mode)."""
        return [self.agents] if self.agents_device else []

    def params(self):
        from ._lib import SfRenderParams
        p = SfRenderParams()
        p.source, p.first, p.count = self.source, self.first, self.count
        p.scale, p.mode = self.scale, MODES[self.mode]
        p.background, p.contours = BACKGROUNDS[self.background], int(self.contours)
        for i, c in enumerate(self.terrain_rgb):
            p.terrain_rgb[i] = c
        p.channels_last = int(self.channels_last)
        if self.agents is not None and self.k:
            p.agents_k = self.k
            p.agents_device = int(self.agents_device)
            p.agents = self.agents.data_ptr() if self.agents_device else self.agents.ctypes.data
        return p
