"""``FireEngine``: object wrapper around one ``sf_sim`` handle of the C ABI.

This is the only module that touches the HIP library; the reference-shaped classes in
``fire.py`` / ``simulation.py`` are written on top of it.  Arrays cross the boundary as
NumPy host arrays (copied during the call); nothing here depends on torch.
"""
import ctypes as C
import os

import numpy as np

from . import _lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class FireEngine:
    """n_envs batched Rothermel fire simulations sharing one terrain on one GPU.

    Mirrors the constructor arguments of the reference's ``RothermelFireManager``
    (simfire/game/managers/fire.py:293-307)."""

    def __init__(self, shape, n_envs=1, max_fire_duration=4, pixel_scale=50.0, update_rate=1.0,
                 max_time=None, attenuate_line_ros=True, diagonal_spread=True, M_f=0.03,
                 particle=(8000.0, 0.0555, 0.01, 32.0), device=0, per_env_terrain=False, variant=None):
        # variant: another build of the library (tests only; _lib.VARIANTS)
        self._L = _lib.load(variant)
        self.H, self.W = int(shape[0]), int(shape[1])
        self.n_envs = int(n_envs)
        h, S_T, S_e, p_p = particle
        self.params = _lib.SfParams(
            n_envs=self.n_envs, height=self.H, width=self.W, max_fire_duration=int(max_fire_duration),
            diagonal_spread=int(bool(diagonal_spread)), attenuate_line_ros=int(bool(attenuate_line_ros)),
            has_max_time=int(max_time is not None), device=int(device), pixel_scale=float(pixel_scale),
            update_rate=float(update_rate), max_time=float(0.0 if max_time is None else max_time),
            h=float(h), S_T=float(S_T), S_e=float(S_e), p_p=float(p_p), M_f=float(M_f),
            per_env_terrain=int(bool(per_env_terrain)))
        self.prune_after_quit = False
        self.spread_graph = self.spread_graph_on = False
        self.async_mode = False
        self.arrival_on = False             # arrival times are recorded (enable_arrival)
        self.values_on = False              # a value plane is set (values_set)
        self.n_agents = 0                   # agents per environment (agents_create); 0: no agent state
        self.episodes_on = False            # new episodes draw their parameters on the device (episodes_set)
        self._blobs_in_flight = []          # device state blobs an enqueued save / load may still touch (async mode; released by sync)
        self._h = C.c_void_p()
        self._chk(self._L.sf_create(C.byref(self.params), C.byref(self._h)))
        if os.environ.get("SF_DEBUG_KNOBS") == "1":
            # measurement scripts under profiles/ only: initial knob values from variables named like the enumerators
            # (SF_TUNE_RUN_WAVES=8 ...) - read HERE, in the laboratory binding; the library itself never looks at the environment
            for name in _lib.TUNE:
                v = os.environ.get("SF_TUNE_" + name.upper())
                if v is not None:
                    self.set_tuning(**{name: int(v)})

    def _chk(self, rc):
        _lib.check(rc, self._L)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.sf_destroy(self._h)
            self._h = C.c_void_p()
            self._blobs_in_flight = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ construction
    def _plane(self, a, name):
        a = np.asarray(a, dtype=np.float64)
        if a.ndim == 0:
            a = np.full((self.H, self.W), float(a))
        if a.shape != (self.H, self.W):
            raise ValueError(f"The input parameter shape of {a.shape} should match the terrain "
                             f"shape of {(self.H, self.W)} ({name})")
        return np.ascontiguousarray(a)

    def set_layers(self, w_0, delta, M_x, sigma, elevation, U, U_dir, env=None):
        """``env=None``: all environments; an index: that environment only (``per_env_terrain``)."""
        arrs = [self._plane(a, n) for a, n in zip(
            (w_0, delta, M_x, sigma, elevation, U, U_dir),
            ("w_0", "delta", "M_x", "sigma", "elevation", "U", "U_dir"))]
        if env is None:
            self._chk(self._L.sf_set_layers(self._h, *[_ptr(a) for a in arrs]))
        else:
            self._chk(self._L.sf_set_layers_env(self._h, int(env), *[_ptr(a) for a in arrs]))

    def set_rtable(self, R8, env=None):
        R8 = np.ascontiguousarray(R8, dtype=np.float64)
        if R8.shape != (8, self.H, self.W):
            raise ValueError(f"R table shape {R8.shape} != {(8, self.H, self.W)}")
        if env is None:
            self._chk(self._L.sf_set_rtable(self._h, _ptr(R8)))
        else:
            self._chk(self._L.sf_set_rtable_env(self._h, int(env), _ptr(R8)))

    def get_rtable(self, env=0):
        out = np.empty((8, self.H, self.W), dtype=np.float64)
        self._chk(self._L.sf_get_rtable_env(self._h, int(env), _ptr(out)))
        return out

    def get_slopes(self):
        mag = np.empty((self.H, self.W))
        dr = np.empty((self.H, self.W))
        self._chk(self._L.sf_get_slopes(self._h, _ptr(mag), _ptr(dr)))
        return mag, dr

    # ------------------------------------------------------------------------ running
    def reset(self, init_xy):
        xy = np.ascontiguousarray(np.asarray(init_xy, dtype=np.int32).reshape(-1, 2))
        if xy.shape[0] == 1 and self.n_envs > 1:
            xy = np.ascontiguousarray(np.repeat(xy, self.n_envs, axis=0))
        if xy.shape[0] != self.n_envs:
            raise ValueError(f"need {self.n_envs} ignition points, got {xy.shape[0]}")
        self._chk(self._L.sf_reset(self._h, _ptr(xy)))

    def reset_env(self, env, x, y):
        self._chk(self._L.sf_reset_env(self._h, int(env), int(x), int(y)))

    def _ignitions(self, xy, n, name):
        """Host ignitions int32 [n, 2] = (x, y), every one on the grid (checked here: no device call has been made yet)."""
        a = np.asarray(xy)
        if a.dtype.kind not in "iu":
            raise ValueError(f"{name}: ignitions must be integers, got {a.dtype}")
        if a.shape != (n, 2):
            raise ValueError(f"{name}: ignitions must have shape {(n, 2)}, got {a.shape}")
        a = np.ascontiguousarray(a, dtype=np.int32)
        bad = np.flatnonzero((a[:, 0] < 0) | (a[:, 0] >= self.W) | (a[:, 1] < 0) | (a[:, 1] >= self.H))
        if bad.size:
            i = int(bad[0])
            raise ValueError(f"{name}: ignition ({a[i, 0]}, {a[i, 1]}) of entry {i} is outside the {self.H}x{self.W} grid")
        return a

    def reset_envs(self, envs, xy):
        """New episodes in ``envs`` (environment ``envs[i]`` ignites at ``xy[i]`` = (x, y)), one launch for all of them
        (``sf_reset_envs``).  An environment may repeat: its last ignition wins.  In async mode the call only enqueues."""
        e = np.asarray(envs)
        if e.ndim != 1 or (e.size and e.dtype.kind not in "iu"):
            raise ValueError("reset_envs: envs must be a list of environment numbers")
        e = np.ascontiguousarray(e, dtype=np.int32)
        a = self._ignitions(xy, e.shape[0], "reset_envs")
        if e.size and (e.min() < 0 or e.max() >= self.n_envs):
            raise IndexError(f"reset_envs: environment {int(e[(e < 0) | (e >= self.n_envs)][0])} out of range (n_envs = {self.n_envs})")
        if e.size:
            self._chk(self._L.sf_reset_envs(self._h, int(e.shape[0]), _ptr(e), _ptr(a)))

    def reset_where(self, mask=None, xy=None):
        """New episodes in every environment that is not running (``mask=None``; decided on the device, nothing is read back) or that
        ``mask`` selects (a torch CUDA uint8 / bool tensor [n_envs] on this GPU); environment e ignites at ``xy[e]`` - a NumPy array
        or a torch CUDA int32 tensor [n_envs, 2] (``sf_reset_where``).  A device ignition off the grid leaves its environment
        untouched.  Torch's queued work on the tensors is waited for first; in async mode they are kept alive until ``sync``."""
        tensors = []
        if mask is not None:
            import torch
            if not isinstance(mask, torch.Tensor) or not mask.is_cuda or mask.dtype not in (torch.uint8, torch.bool) \
                    or tuple(mask.shape) != (self.n_envs,):
                raise ValueError(f"reset_where: mask must be None or a CUDA uint8 / bool tensor of shape ({self.n_envs},)")
            mask = mask.contiguous()
            tensors.append(mask)
        if xy is None:
            raise ValueError("reset_where: xy (the ignitions, [n_envs, 2]) is required")
        if getattr(xy, "is_cuda", False):
            import torch
            if xy.dtype != torch.int32 or tuple(xy.shape) != (self.n_envs, 2):
                raise ValueError(f"reset_where: a device xy must be a CUDA int32 tensor of shape ({self.n_envs}, 2)")
            xy = xy.contiguous()
            tensors.append(xy)
            xy_ptr, xy_dev = C.c_void_p(xy.data_ptr()), 1
        else:
            a = self._ignitions(xy, self.n_envs, "reset_where")
            xy_ptr, xy_dev = _ptr(a), 0
        mask_ptr = C.c_void_p(mask.data_ptr()) if mask is not None else None
        if tensors:
            import torch
            torch.cuda.synchronize(tensors[0].device)
        self._chk(self._L.sf_reset_where(self._h, mask_ptr, xy_ptr, xy_dev))
        if self.async_mode:
            self._blobs_in_flight.extend(tensors)

    def time_resets(self, on=True):
        """Measurement only: record HIP events around the launches of every ``reset_envs`` / ``reset_where`` (``sf_time_resets``)."""
        self._chk(self._L.sf_time_resets(self._h, int(bool(on))))

    def reset_ms(self):
        """GPU milliseconds of the last timed batched reset's launches (``sf_get_reset_ms``; waits for them)."""
        ms = C.c_float(0.0)
        self._chk(self._L.sf_get_reset_ms(self._h, C.byref(ms)))
        return float(ms.value)

    # ------------------------------------------------------------------ agents on the device
    def agents_create(self, n_agents, ignitions=None, n_updates=1, weights=(-1.0, 0.0, 0.0, 0.0), only_unburned=True,
                      done_on_burn=False, max_ticks=0, auto_reset=True):
        """Agent state for ``n_agents`` (1..64) agents per environment (``sf_agents_create``; called again it replaces the state,
        ``n_agents=0`` frees it).  ``ignitions`` [n_envs, 2] = (x, y): where a done environment re-ignites under ``auto_reset``.
        All agents start at (0, 0) until ``agents_place``.  Argument errors are raised before any device call."""
        k = int(n_agents)
        if k < 0 or k > 64:
            raise ValueError(f"agents_create: {k} agents per environment (1..64; 0 frees)")
        w = [float(v) for v in weights]
        if len(w) != 4:
            raise ValueError("agents_create: weights are the four factors of terms[0..3]")
        if k and int(n_updates) < 1:
            raise ValueError(f"agents_create: n_updates = {n_updates} must be >= 1")
        if k and int(max_ticks) < 0:
            raise ValueError(f"agents_create: max_ticks = {max_ticks} must be >= 0")
        ign = None
        if k and ignitions is not None:
            ign = self._ignitions(ignitions, self.n_envs, "agents_create")
        elif k and auto_reset:
            raise ValueError("agents_create: auto_reset needs the ignitions")
        p = _lib.SfAgentParams(k=k, n_updates=int(n_updates), only_unburned=int(bool(only_unburned)),
                               done_on_burn=int(bool(done_on_burn)), max_ticks=int(max_ticks), auto_reset=int(bool(auto_reset)))
        for i in range(4):
            p.w[i] = w[i]
        self._chk(self._L.sf_agents_create(self._h, C.byref(p), _ptr(ign) if ign is not None else None))
        self.n_agents = k

    def agents_set_value_weight(self, w):
        """The fifth reward term of ``agents_step``: ``w * tick_loss[e]``, the value the fire reached during the tick (``values_set``;
        ``sf_values_set_weight``).  ``None`` switches it off: the reward is then bit for bit what it is without a value plane.
        Needs agents and a value plane; ``agents_create`` and ``values_set(None)`` switch it off."""
        if w is not None and not np.isfinite(float(w)):
            raise ValueError(f"agents_set_value_weight: weight {w!r} is not finite")
        self._chk(self._L.sf_values_set_weight(self._h, float(0.0 if w is None else w), int(w is not None)))

    def agents_place(self, envs, xy, also_start=True):
        """The agents of environment ``envs[i]`` stand at ``xy[i]`` (int [n, n_agents, 2] = (column, row); ``sf_agents_place``).
        ``also_start``: these cells become the start cells a done environment's agents go back to, and the environments' episode
        statistics are cleared.  In async mode the call only enqueues."""
        k = self.n_agents
        if not k:
            raise _lib.SimfireHipError("agents_place: call agents_create first")
        e = self._env_list(envs, "envs")
        a = np.asarray(xy)
        if a.dtype.kind not in "iu":
            raise ValueError(f"agents_place: cells must be integers, got {a.dtype}")
        if a.shape != (e.shape[0], k, 2):
            raise ValueError(f"agents_place: cells must have shape {(e.shape[0], k, 2)}, got {a.shape}")
        a = np.ascontiguousarray(a, dtype=np.int32)
        if e.size and (e.min() < 0 or e.max() >= self.n_envs):
            raise ValueError(f"agents_place: environment {int(e[(e < 0) | (e >= self.n_envs)][0])} out of range (n_envs = {self.n_envs})")
        if ((a[..., 0] < 0) | (a[..., 0] >= self.W) | (a[..., 1] < 0) | (a[..., 1] >= self.H)).any():
            raise ValueError(f"agents_place: a cell is outside the {self.H}x{self.W} grid")
        if e.size:
            self._chk(self._L.sf_agents_place(self._h, int(e.shape[0]), _ptr(e), _ptr(a), int(bool(also_start))))

    def agents_step(self, actions, reward=None, done=None, terms=None, final_len=None, final_ret=None):
        """One tick for every environment from a device action tensor, nothing read back (``sf_agents_step``).  ``actions``: torch
        CUDA int32 [n_envs, n_agents], word = move + 5 * interact.  Outputs, each optional, torch CUDA tensors on this GPU:
        ``reward`` float32 [n_envs], ``done`` uint8 / bool [n_envs], ``terms`` int32 [n_envs, 4], ``final_len`` int32 [n_envs],
        ``final_ret`` float64 [n_envs].  Torch's queued work on the tensors is waited for first; in async mode the call only
        enqueues and the tensors are kept alive until ``sync``."""
        import torch
        k = self.n_agents
        if not k:
            raise _lib.SimfireHipError("agents_step: call agents_create first")
        E = self.n_envs
        dev = torch.device(f"cuda:{self.params.device}")

        def chk(t, name, dtypes, shape):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype not in dtypes or tuple(t.shape) != shape \
                    or not t.is_contiguous() or t.device != dev:
                raise ValueError(f"agents_step: {name} must be a contiguous {dtypes[0]} tensor of shape {shape} on {dev}")
            return t
        chk(actions, "actions", (torch.int32,), (E, k))
        o = _lib.SfAgentOut()
        tensors = [actions]
        for t, name, dtypes, shape in ((reward, "reward", (torch.float32,), (E,)), (done, "done", (torch.uint8, torch.bool), (E,)),
                                       (terms, "terms", (torch.int32,), (E, 4)), (final_len, "final_len", (torch.int32,), (E,)),
                                       (final_ret, "final_ret", (torch.float64,), (E,))):
            if t is not None:
                setattr(o, name, chk(t, name, dtypes, shape).data_ptr())
                tensors.append(t)
        torch.cuda.synchronize(dev)
        self._chk(self._L.sf_agents_step(self._h, C.c_void_p(actions.data_ptr()), C.byref(o)))
        if self.async_mode:
            self._blobs_in_flight.extend(tensors)

    def agents_device(self):
        """Zero-copy torch view int32 [n_envs, n_agents, 3] = (column, row, id) of the agent positions on this GPU: what ``observe``
        / ``render`` take as ``agents``.  Valid until the next ``agents_create``; read it after ``sync`` in async mode."""
        import torch
        if not self.n_agents:
            raise _lib.SimfireHipError("agents_device: call agents_create first")
        p = C.c_void_p()
        self._chk(self._L.sf_agents_device(self._h, C.byref(p)))
        shape = (self.n_envs, self.n_agents, 3)

        class _Agents:
            __cuda_array_interface__ = {"shape": shape, "typestr": "<i4", "data": (p.value, False), "version": 2, "strides": None}
        return torch.as_tensor(_Agents(), device=f"cuda:{self.params.device}")

    # ------------------------------------------------------------------ drawn episodes
    def _box(self, box, name):
        b = [int(v) for v in box]
        if len(b) != 4:
            raise ValueError(f"episodes_set: {name} is (x0, y0, x1, y1), inclusive")
        if b[0] < 0 or b[1] < 0 or b[2] >= self.W or b[3] >= self.H or b[0] > b[2] or b[1] > b[3]:
            raise ValueError(f"episodes_set: {name} {tuple(b)} is not x0 <= x1, y0 <= y1 on the {self.H}x{self.W} grid")
        return b

    def episodes_set(self, seed, ignition_box=None, live_cells=False, wind_speed=None, wind_direction=None, agent_box=None):
        """Every new episode draws its parameters on the device (``sf_episodes_set``): a function of (seed, environment, episode
        index) alone.  ``ignition_box`` / ``agent_box`` (x0, y0, x1, y1), inclusive: where the ignition / every agent's start cell
        is drawn; ``live_cells``: the ignition among cells whose R table is not all zero (64 attempts; needs ``ignition_box``);
        ``wind_speed`` (lo, hi) ft/min and ``wind_direction`` (lo, hi) degrees: a uniform wind per episode (both or neither; needs
        ``per_env_terrain`` and layers, excludes wind schedules).  ``None`` leaves a part off: the ignition, the agents' start
        cells and the wind then stay what they are.  ``seed=None`` switches randomisation off and frees its buffers.  While set,
        ``agents_step`` draws for every environment its auto-reset takes, and ``episodes_begin`` for those it is told to take.
        Every environment's episode index starts at 0.  Argument errors are raised before any device call."""
        if seed is None:
            self._chk(self._L.sf_episodes_set(self._h, None))
            self.episodes_on = False
            return
        p = _lib.SfEpisodeParams(seed=int(seed) & 0xFFFFFFFFFFFFFFFF)
        flags = 0
        if live_cells and ignition_box is None:
            raise ValueError("episodes_set: live_cells needs an ignition_box")
        if ignition_box is not None:
            flags |= _lib.SF_EP_IGNITION | (_lib.SF_EP_LIVE_CELL if live_cells else 0)
            p.ign_box[:] = self._box(ignition_box, "ignition_box")
        if agent_box is not None:
            flags |= _lib.SF_EP_AGENTS
            p.agent_box[:] = self._box(agent_box, "agent_box")
        if (wind_speed is None) != (wind_direction is None):
            raise ValueError("episodes_set: wind_speed and wind_direction go together")
        if wind_speed is not None:
            u, d = [float(v) for v in wind_speed], [float(v) for v in wind_direction]
            if len(u) != 2 or len(d) != 2 or not np.isfinite(u + d).all() or u[0] < 0 or u[0] > u[1] or d[0] > d[1]:
                raise ValueError(f"episodes_set: wind_speed {tuple(u)} / wind_direction {tuple(d)} must be finite (lo, hi) ranges, "
                                 "lo <= hi, speed >= 0")
            flags |= _lib.SF_EP_WIND
            p.U[:], p.U_dir[:] = u, d
        p.flags = flags
        self._chk(self._L.sf_episodes_set(self._h, C.byref(p)))
        self.episodes_on = True

    def episodes_begin(self, mask=None, all=False):
        """New episodes with drawn parameters (``sf_episodes_begin``): in every environment (``all=True``), in those ``mask`` selects
        (a torch CUDA uint8 / bool tensor [n_envs] on this GPU) or, ``mask=None``, in those that are not running - decided on the
        device, nothing is read back.  The mask form of ``reset_where`` otherwise: torch's queued work on the mask is waited for
        first; in async mode it is kept alive until ``sync``."""
        tensors = []
        if mask is not None and not all:
            import torch
            if not isinstance(mask, torch.Tensor) or not mask.is_cuda or mask.dtype not in (torch.uint8, torch.bool) \
                    or tuple(mask.shape) != (self.n_envs,):
                raise ValueError(f"episodes_begin: mask must be None or a CUDA uint8 / bool tensor of shape ({self.n_envs},)")
            mask = mask.contiguous()
            tensors.append(mask)
            torch.cuda.synchronize(mask.device)
        mask_ptr = C.c_void_p(mask.data_ptr()) if tensors else None
        self._chk(self._L.sf_episodes_begin(self._h, mask_ptr, int(bool(all))))
        if self.async_mode:
            self._blobs_in_flight.extend(tensors)

    def episodes_torch(self):
        """Zero-copy torch views of what the last draw of every environment made (``sf_episodes_device``): ``index`` int32 [n_envs]
        (the NEXT episode's index; the bits of a uint32), ``ignition`` int32 [n_envs, 2] = (x, y), ``wind`` float64 [n_envs, 2] =
        (U ft/min, U_dir degrees).  They report draws, not a later ``set_wind``, ``reset_envs`` or ``copy_envs``.  Read-only; the
        handle's stream is waited for first.  Valid until the next ``episodes_set``."""
        import torch
        ptrs = [C.c_void_p(), C.c_void_p(), C.c_void_p()]
        self._chk(self._L.sf_episodes_device(self._h, *[C.byref(p) for p in ptrs]))
        self.sync()
        E, dev = self.n_envs, f"cuda:{self.params.device}"

        def view(ptr, shape, typestr):
            class _Buf:
                __cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr.value, False), "version": 2, "strides": None}
            return torch.as_tensor(_Buf(), device=dev)
        return dict(index=view(ptrs[0], (E,), "<i4"), ignition=view(ptrs[1], (E, 2), "<i4"), wind=view(ptrs[2], (E, 2), "<f8"))

    def apply_mitigation(self, pts):
        """pts: rows (env, x, y, type)."""
        q = np.ascontiguousarray(np.asarray(pts, dtype=np.int32).reshape(-1, 4))
        if len(q):
            self._chk(self._L.sf_apply_mitigation(self._h, _ptr(q), len(q)))

    def apply_mitigation_torch(self, pts):
        """The same scatter for a torch int32 tensor [n, 4] (env, x, y, type) that already lives on this
        GPU (e.g. the actions of a policy): no host round trip; rows with an out-of-range field are
        skipped.  The caller orders its own stream before this call (``torch.cuda.synchronize`` or an
        event), the library then works on its own stream."""
        import torch
        if pts.dtype != torch.int32 or pts.dim() != 2 or pts.shape[1] != 4 or not pts.is_cuda:
            raise ValueError("expected a CUDA int32 tensor of shape [n, 4]")
        pts = pts.contiguous()
        if pts.shape[0]:
            self._chk(self._L.sf_apply_mitigation_device(self._h, C.c_void_p(pts.data_ptr()), int(pts.shape[0])))
            self._keep_alive = pts          # until the next call: the scatter may still be queued (async mode)

    def load_fire_map(self, env, fire_map):
        m = np.asarray(fire_map)
        if m.shape != (self.H, self.W):
            raise ValueError(f"fire_map shape {m.shape} != {(self.H, self.W)}")
        if m.min() < 0 or m.max() > 5:
            raise ValueError("fire_map holds values outside BurnStatus")
        m = np.ascontiguousarray(m, dtype=np.uint8)
        self._chk(self._L.sf_load_fire_map(self._h, int(env), _ptr(m)))

    def step(self, n=1):
        self._chk(self._L.sf_step(self._h, int(n)))

    def step_timed(self, n=1):
        """Returns the GPU milliseconds spent in the n step kernels."""
        ms = C.c_float(0.0)
        self._chk(self._L.sf_step_timed(self._h, int(n), C.byref(ms)))
        return float(ms.value)

    def step_mitigated(self, pts, timed=False):
        """``for s in range(n): update_mitigation(pts[s]); step(1)`` as one call.  ``pts``: int32 [n, n_envs, k, 3] =
        (column, row, type) per environment and step - a NumPy array or a torch CUDA tensor on this GPU; entries with a
        type outside 3..5 are padding.  Returns the GPU milliseconds if ``timed``."""
        ms = C.c_float(0.0)
        if isinstance(pts, np.ndarray) or not hasattr(pts, "data_ptr"):
            q = np.ascontiguousarray(np.asarray(pts, dtype=np.int32))
            if q.ndim != 4 or q.shape[1] != self.n_envs or q.shape[3] != 3:
                raise ValueError(f"expected points of shape [n_steps, {self.n_envs}, k, 3], got {q.shape}")
            self._chk(self._L.sf_step_mitigated(self._h, q.shape[0], _ptr(q), q.shape[2], 0, C.byref(ms) if timed else None))
        else:
            import torch
            if pts.dtype != torch.int32 or pts.dim() != 4 or pts.shape[1] != self.n_envs or pts.shape[3] != 3 or not pts.is_cuda:
                raise ValueError(f"expected a CUDA int32 tensor of shape [n_steps, {self.n_envs}, k, 3]")
            pts = pts.contiguous()
            self._chk(self._L.sf_step_mitigated(self._h, int(pts.shape[0]), C.c_void_p(pts.data_ptr()), int(pts.shape[2]), 1,
                                                 C.byref(ms) if timed else None))
            self._keep_alive = pts
        return float(ms.value) if timed else None

    # ------------------------------------------------------------------------ outputs
    def fire_map(self, env=0):
        out = np.empty((self.H, self.W), dtype=np.uint8)
        self._chk(self._L.sf_get_fire_map(self._h, int(env), _ptr(out)))
        return out

    def fire_maps(self):
        out = np.empty((self.n_envs, self.H, self.W), dtype=np.uint8)
        self._chk(self._L.sf_get_fire_maps(self._h, _ptr(out)))
        return out

    def fire_map_delta(self, env=0, cap=4096):
        """Cells of ``env``'s fire map that changed since this method was last called for it (or since ``reset``, whose map is all UNBURNED):
        (flat indices int64 [n], BurnStatus values uint8 [n]), or ``None`` when there is no reference point or more than ``cap`` cells changed -
        fetch the whole map then, before anything steps (``sf_get_fire_map_delta``; ``fire_map`` / ``fire_maps`` never move the reference point)."""
        buf = getattr(self, "_delta_buf", None)
        if buf is None or buf.shape[0] < cap:
            buf = self._delta_buf = np.empty(int(cap), dtype=np.uint32)
        n = C.c_int32(0)
        self._chk(self._L.sf_get_fire_map_delta(self._h, int(env), _ptr(buf), int(cap), C.byref(n)))
        if n.value < 0:
            return None
        cells = buf[:n.value]
        return (cells >> 3).astype(np.int64), (cells & 7).astype(np.uint8)

    def run_delta(self, n, env=0, cap=4096):
        """``step(n)``, environment ``env``'s result row and elapsed_time, and the cells of its fire map that changed - one call, one wait
        (``sf_run_delta``).  Returns (row int32 [8], elapsed_time float, delta as ``fire_map_delta`` returns it)."""
        buf = getattr(self, "_delta_buf", None)
        if buf is None or buf.shape[0] < cap:
            buf = self._delta_buf = np.empty(int(cap), dtype=np.uint32)
        row = getattr(self, "_row_buf", None)
        if row is None:
            row = self._row_buf = np.zeros(8, dtype=np.int32)
            self._el_buf = np.zeros(1, dtype=np.float64)
        n_out = C.c_int32(0)
        self._chk(self._L.sf_run_delta(self._h, int(n), int(env), _ptr(row), _ptr(self._el_buf), _ptr(buf), int(cap), C.byref(n_out)))
        if n_out.value < 0:
            return row, float(self._el_buf[0]), None
        cells = buf[:n_out.value]
        return row, float(self._el_buf[0]), ((cells >> 3).astype(np.int64), (cells & 7).astype(np.uint8))

    def burn(self, env=0):
        out = np.empty((self.H, self.W), dtype=np.float64)
        self._chk(self._L.sf_get_burn(self._h, int(env), _ptr(out)))
        return out

    def set_burn(self, env, burn):
        b = np.ascontiguousarray(burn, dtype=np.float64)
        if b.shape != (self.H, self.W):
            raise ValueError(f"burn shape {b.shape} != {(self.H, self.W)}")
        self._chk(self._L.sf_set_burn(self._h, int(env), _ptr(b)))

    # ------------------------------------------------------------------ environment state
    @staticmethod
    def _env_list(envs, name):
        a = np.ascontiguousarray(np.atleast_1d(np.asarray(envs)), dtype=np.int32)
        if a.ndim != 1:
            raise ValueError(f"{name} must be a list of environment numbers")
        return a

    def copy_envs(self, src, dst, terrain=False):
        """Environment ``dst[i]`` becomes environment ``src[i]`` (one launch for all pairs; ``sf_copy_envs``).  ``terrain``: on a
        per-environment-terrain handle ``dst`` also takes ``src``'s layers and R table."""
        s, d = self._env_list(src, "src"), self._env_list(dst, "dst")
        if s.shape != d.shape:
            raise ValueError(f"src and dst differ in length ({s.shape[0]} != {d.shape[0]})")
        self._chk(self._L.sf_copy_envs(self._h, _ptr(s), _ptr(d), int(s.shape[0]), 1 if terrain else 0))

    def state_bytes(self):
        """Bytes of one environment's state blob (``sf_state_bytes``)."""
        v = C.c_int64(0)
        self._chk(self._L.sf_state_bytes(self._h, C.byref(v)))
        return v.value

    def save_state(self, envs, out=None):
        """The state of ``envs`` as blobs: numpy uint8 [n, state_bytes()], or written into ``out`` (a contiguous CUDA tensor of at
        least n * state_bytes() bytes, 16-byte aligned: device to device, nothing crosses to the host) which is returned.  In async mode
        the device form is only enqueued on the handle's stream: ``sync()`` before torch reads ``out``."""
        e = self._env_list(envs, "envs")
        nb = self.state_bytes()
        if out is None:
            blob = np.empty((e.shape[0], nb), dtype=np.uint8)
            self._chk(self._L.sf_save_state(self._h, int(e.shape[0]), _ptr(e), _ptr(blob), 0))
            return blob
        if not getattr(out, "is_cuda", False) or not out.is_contiguous() or out.numel() * out.element_size() < e.shape[0] * nb:
            raise ValueError(f"out must be a contiguous CUDA tensor of at least {e.shape[0] * nb} bytes")
        self._device_blob_call(out, lambda: self._L.sf_save_state(self._h, int(e.shape[0]), _ptr(e), C.c_void_p(out.data_ptr()), 1))
        return out

    def _device_blob_call(self, t, call):
        """A state call on a blob tensor: the handle works on its own stream, so torch's queued work (which may still write the blob, or
        still use the memory a fresh tensor was given) is waited for first; in async mode the call only enqueues, so the tensor is kept
        alive until ``sync`` (the caching allocator must not hand its memory out while the handle's stream may still touch it)."""
        import torch
        torch.cuda.synchronize(t.device)
        self._chk(call())
        if self.async_mode:
            self._blobs_in_flight.append(t)

    def load_state(self, envs, blob):
        """Environment ``envs[i]`` takes the state of blob i (numpy uint8 [n, state_bytes()] or a contiguous CUDA tensor holding the
        blobs back to back; ``sf_load_state``).  A blob from another geometry or configuration raises ValueError and changes nothing."""
        e = self._env_list(envs, "envs")
        nb = self.state_bytes()
        if getattr(blob, "is_cuda", False):
            if not blob.is_contiguous() or blob.numel() * blob.element_size() < e.shape[0] * nb:
                raise ValueError(f"blob must be a contiguous CUDA tensor of at least {e.shape[0] * nb} bytes")
            self._device_blob_call(blob, lambda: self._L.sf_load_state(self._h, int(e.shape[0]), _ptr(e), C.c_void_p(blob.data_ptr()), 1))
            return
        b = np.ascontiguousarray(blob, dtype=np.uint8)
        if b.size < e.shape[0] * nb:
            raise ValueError(f"blob holds {b.size} bytes, {e.shape[0]} environments need {e.shape[0] * nb}")
        self._chk(self._L.sf_load_state(self._h, int(e.shape[0]), _ptr(e), _ptr(b), 0))

    def status(self):
        """(int32 [E, 8]: running, steps, counts of BurnStatus 0..5; float64 [E] elapsed_time)"""
        st = np.zeros((self.n_envs, 8), dtype=np.int32)
        el = np.zeros(self.n_envs, dtype=np.float64)
        self._chk(self._L.sf_get_status(self._h, _ptr(st), _ptr(el)))
        return st, el

    def memory_bytes(self):
        v = C.c_int64(0)
        self._chk(self._L.sf_memory_bytes(self._h, C.byref(v)))
        return int(v.value)

    def geometry(self):
        """dict(tile_w, tile_h, tiles_x, tiles_y, rows_per_band, pitch, lds_wave_bytes, dense)"""
        out = np.zeros(8, dtype=np.int32)
        self._chk(self._L.sf_get_geometry(self._h, _ptr(out)))
        keys = ("tile_w", "tile_h", "tiles_x", "tiles_y", "rows_per_band", "pitch", "lds_wave_bytes", "dense")
        return dict(zip(keys, (int(v) for v in out)))

    def set_rows_per_band(self, rows):
        self._chk(self._L.sf_set_rows_per_band(self._h, int(rows)))

    def set_threshold(self, pixel_scale):
        """Ignition threshold only (``manager.pixel_scale = v`` in the reference)."""
        self._chk(self._L.sf_set_threshold(self._h, float(pixel_scale)))
        self.params.pixel_scale = float(pixel_scale)

    def set_async(self, on=True):
        """Rollout mode: ``step`` / ``apply_mitigation`` only enqueue work; ``sync`` or any getter waits."""
        self._chk(self._L.sf_set_async(self._h, int(bool(on))))
        self.async_mode = bool(on)

    def sync(self):
        self._chk(self._L.sf_sync(self._h))
        self._blobs_in_flight.clear()

    def set_fused(self, mode=-1):
        """-1 auto, 0 always k_select + k_step, 1 always one fused launch per step, 2 one environment-resident
        launch per ``step(n)`` call (k_run)."""
        self._chk(self._L.sf_set_fused(self._h, int(mode)))

    def set_tuning(self, **knobs):
        """Launch-geometry knobs (``include/simfire_hip.h``: ``SF_TUNE_*``; results never depend on them), e.g.
        ``set_tuning(run_waves=8, run_vcap=256)``."""
        for name, value in knobs.items():
            self._chk(self._L.sf_set_tuning(self._h, _lib.TUNE[name], int(value)))

    # ---- closed loop: update_mitigation(actions) + run(1) per call without a launch per step (sf_loop_*)
    def loop_start(self, k):
        """Leave the resident launch on the GPU, driven by ``loop_step``; ``k`` = points per environment and step (<= 64)."""
        self._loop_k = int(k)
        self._loop_status = np.zeros((self.n_envs, 8), dtype=np.int32)
        self._loop_elapsed = np.zeros(self.n_envs, dtype=np.float64)
        self._loop_ptrs = (C.c_void_p(self._loop_status.ctypes.data), C.c_void_p(self._loop_elapsed.ctypes.data))      # (a call is ~20 us: ctypes' data_as is 1 us a piece)
        self._loop_shape = (self.n_envs, self._loop_k, 3)
        self._chk(self._L.sf_loop_start(self._h, int(k)))

    def loop_step(self, pts=None):
        """``update_mitigation(pts); run(1)`` for every environment; ``pts`` int32 [n_envs, k, 3] = (column, row, type) or None.
        Returns (status int32 [n_envs, 8], elapsed_time float64 [n_envs]) - views that the next call overwrites."""
        if getattr(self, "_loop_k", None) is None:
            raise _lib.SimfireHipError("loop_step: call loop_start first")
        p = None
        if pts is not None:
            if not (type(pts) is np.ndarray and pts.dtype == np.int32 and pts.flags.c_contiguous):
                pts = np.ascontiguousarray(np.asarray(pts, dtype=np.int32))
            if pts.shape != self._loop_shape:
                raise ValueError(f"expected points of shape {self._loop_shape}, got {pts.shape}")
            p = pts.ctypes.data
        rc = self._L.sf_loop_step(self._h, p, self._loop_ptrs[0], self._loop_ptrs[1])
        if rc:
            self._chk(rc)
        return self._loop_status, self._loop_elapsed

    def loop_stop(self):
        self._chk(self._L.sf_loop_stop(self._h))

    def loop_restarts(self):
        v = C.c_int32()
        self._chk(self._L.sf_loop_restarts(self._h, C.byref(v)))
        return v.value

    def run_cost(self):
        """Shader clocks / 16 every environment's workgroup(s) spent in the last resident launch (uint32 [n_envs])."""
        out = np.zeros(self.n_envs, dtype=np.uint32)
        self._chk(self._L.sf_get_run_cost(self._h, _ptr(out)))
        return out

    def team_sizes(self):
        """Workgroups per environment in the last resident launch (zeros: it was not a team launch)."""
        out = np.zeros(self.n_envs, dtype=np.uint32)
        self._chk(self._L.sf_get_team_sizes(self._h, _ptr(out)))
        return out

    def join_log(self):
        """Growths of the teams in the last resident launch whose teams grow inside it: array [n, 3] of (environment, first update of the
        enlarged team, new size); rows with size 255: (environment, the device's 100 MHz wall clock when its updates were done, 255)."""
        out = np.zeros((4096, 3), dtype=np.uint32)
        n = C.c_int32()
        self._chk(self._L.sf_get_join_log(self._h, _ptr(out), 4096, C.byref(n)))
        return out[:n.value]

    def last_launches(self):
        """Environment-resident launches the last step / step_mitigated / rollout call was made of (0: per-step kernels)."""
        v = C.c_int32()
        self._chk(self._L.sf_get_last_launches(self._h, C.byref(v)))
        return int(v.value)

    def team_fallbacks(self):
        """Teams of a fixed size that found at their start that not all members were resident and whose environment was stepped by
        member 0 alone (same results; since the handle was created)."""
        v = C.c_int32()
        self._chk(self._L.sf_get_team_fallbacks(self._h, C.byref(v)))
        return int(v.value)

    def get_tuning(self, name):
        v = C.c_int32()
        self._chk(self._L.sf_get_tuning(self._h, _lib.TUNE[name], C.byref(v)))
        return v.value

    def set_prune_after_quit(self, on=True):
        """Environments that QUIT on the runtime check keep pruning when stepped again (fire.py:631-643)."""
        self._chk(self._L.sf_set_prune_after_quit(self._h, int(bool(on))))
        self.prune_after_quit = bool(on)

    def last_launch_kind(self):
        """0 k_select + k_step, 1 fused launch per step, 2 resident launch (k_run), 3 per-cell kernel, 4 the window kernel k_win in front of
        k_run (more environments than CUs, young fires), -1 none yet."""
        v = C.c_int32(-1)
        self._chk(self._L.sf_last_step_launch(self._h, C.byref(v)))
        return int(v.value)

    # neighbour order of the parent masks = adj_locs of simfire/utils/graph.py:125-134
    GRAPH_DX = (+1, +1, 0, -1, -1, -1, 0, +1)
    GRAPH_DY = (0, +1, +1, +1, 0, -1, -1, -1)

    def enable_spread_graph(self, on=True):
        """Record the fire-spread graph (FireSpreadGraph, simfire/utils/graph.py) as parent masks."""
        self._chk(self._L.sf_enable_spread_graph(self._h, int(bool(on))))
        self.spread_graph_on = bool(on)
        self.spread_graph = self.spread_graph or bool(on)        # the parent masks exist (they stay allocated once they do; a state blob carries them)

    def spread_parents(self, env=0):
        """uint8 [H, W]: bit j set <=> graph edge from neighbour j (GRAPH_DX/DY) into the cell."""
        out = np.zeros((self.H, self.W), dtype=np.uint8)
        self._chk(self._L.sf_get_spread_parents(self._h, int(env), _ptr(out)))
        return out

    def spread_edges(self, env=0):
        """Sorted list of graph edges (source_x, source_y, x, y) like ``FireSpreadGraph.graph.edges``."""
        par = self.spread_parents(env)
        out = []
        ys, xs = np.nonzero(par)
        for y, x in zip(ys, xs):
            for k in range(8):
                if (par[y, x] >> k) & 1:
                    out.append((int(x) + self.GRAPH_DX[k], int(y) + self.GRAPH_DY[k], int(x), int(y)))
        return sorted(out)

    # ---------------------------------------------------------------- layers held in HBM
    def set_layers_fbfm(self, codes, elevation, U, U_dir, env=None, table=None):
        """Layers from an FBFM13 fuel-model raster; the code -> Fuel lookup
        (``FuelLayer._get_data``, simfire/utils/layers.py:670-676) runs on the device.
        ``table``: {code: Fuel}, default ``parameters.FuelModelToFuel``.  Unknown code: ValueError."""
        from .parameters import FuelModelToFuel
        table = FuelModelToFuel if table is None else table
        codes = np.ascontiguousarray(codes, dtype=np.int32)
        if codes.shape != (self.H, self.W):
            raise ValueError(f"fuel code raster shape {codes.shape} != {(self.H, self.W)}")
        lut_codes = np.array(sorted(table), dtype=np.int32)
        lut_fuel = np.array([[table[int(c)].w_0, table[int(c)].delta, table[int(c)].M_x, table[int(c)].sigma]
                             for c in lut_codes], dtype=np.float64)
        arrs = [self._plane(a, n) for a, n in zip((elevation, U, U_dir), ("elevation", "U", "U_dir"))]
        self._chk(self._L.sf_set_layers_fbfm(self._h, -1 if env is None else int(env), _ptr(codes), len(lut_codes),
                                              _ptr(lut_codes), _ptr(lut_fuel), *[_ptr(a) for a in arrs]))

    @staticmethod
    def _noise(spec):
        """An ``sf_noise`` from None (plane untouched), a number (constant plane) or a dict of simplex parameters
        (seed, scale, octaves, persistence, lacunarity, lo, hi)."""
        n = _lib.SfNoise()
        if spec is None:
            n.kind = _lib.SF_GEN_NONE
        elif isinstance(spec, dict):
            n.kind, n.seed, n.octaves = _lib.SF_GEN_SIMPLEX, int(spec["seed"]), int(spec["octaves"])
            n.scale, n.persistence, n.lacunarity = float(spec.get("scale", 1.0)), float(spec["persistence"]), float(spec["lacunarity"])
            n.lo, n.hi = float(spec["lo"]), float(spec["hi"])
        else:
            n.kind, n.lo = _lib.SF_GEN_CONSTANT, float(spec)
        return n

    def generate_layers(self, envs, elevation=None, fuel=None, wind_speed=None, wind_direction=None):
        """Draw the layers of ``envs`` on the device and rebuild their R tables (``sf_generate_layers``): one
        launch for the planes, one for the tables, one wait.  Per plane, a ``list`` with one entry per environment, or one entry for all:
        ``None`` leaves the plane as it is, a number fills it, a dict draws simplex noise - ``elevation`` as ``workloads.perlin_elevation``
        (keys seed, octaves, persistence, lacunarity, lo, hi; scale 1), wind as ``workloads.simplex_field`` (+ scale).  ``fuel``:
        None or a tuple (w_0, delta, M_x, sigma).  Needs a ``per_env_terrain`` handle; a bad argument raises before any device work."""
        e = self._env_list(envs, "envs")
        n = int(e.shape[0])

        def per_env(v, name):
            if isinstance(v, list):
                if len(v) != n:
                    raise ValueError(f"{name}: {len(v)} entries for {n} environments")
                return list(v)
            return [v] * n
        el, fu, ws, wd = (per_env(v, k) for v, k in ((elevation, "elevation"), (fuel, "fuel"), (wind_speed, "wind_speed"),
                                                      (wind_direction, "wind_direction")))
        gens = (_lib.SfLayerGen * max(n, 1))()
        for i in range(n):
            g = gens[i]
            g.elevation, g.wind_speed, g.wind_direction = self._noise(el[i]), self._noise(ws[i]), self._noise(wd[i])
            if fu[i] is not None:
                vals = [float(v) for v in fu[i]]
                if len(vals) != 4:
                    raise ValueError("fuel: (w_0, delta, M_x, sigma)")
                g.fuel = _lib.SF_GEN_CONSTANT
                for k in range(4):
                    g.fuel_values[k] = vals[k]
        self._chk(self._L.sf_generate_layers(self._h, n, _ptr(e), C.cast(gens, C.c_void_p)))

    def set_wind(self, speed, direction, envs=None):
        """A wind change during an episode (``sf_set_wind``): the R tables of ``envs`` (default: every table in
        order - one on a shared-terrain handle) rebuilt on the device from the new wind and the unchanged fuel and elevation planes;
        nothing else of the environments' state changes.  ``speed`` (ft/min) and ``direction`` (degrees): scalars or ``[n]`` for a
        uniform wind per table, ``[H, W]`` or ``[n, H, W]`` for a field - NumPy arrays, or contiguous float64 CUDA tensors on this
        GPU, which are read in place (torch's current stream is waited for first, as for ``apply_mitigation_torch``'s caller; in
        async mode the tensors are kept alive until ``sync``).  Clears a listed environment's schedule."""
        n_tab = self.n_envs if self.params.per_env_terrain else 1
        e = None if envs is None else self._env_list(envs, "envs")
        n = n_tab if e is None else int(e.shape[0])
        on_device = [getattr(a, "is_cuda", None) is not None for a in (speed, direction)]
        if on_device[0] != on_device[1]:
            raise ValueError("set_wind: speed and direction must both be arrays or both be CUDA tensors")
        shapes = {(): 0, (n,): 0, (self.H, self.W): _lib.SF_WIND_FIELD, (n, self.H, self.W): _lib.SF_WIND_FIELD}
        if on_device[0]:
            import torch
            for t, name in ((speed, "speed"), (direction, "direction")):
                if not t.is_cuda or t.device.index != self.params.device or t.dtype != torch.float64 or not t.is_contiguous():
                    raise ValueError(f"set_wind: {name} must be a contiguous float64 CUDA tensor on device {self.params.device}")
            if tuple(speed.shape) != tuple(direction.shape) or tuple(speed.shape) not in shapes:
                raise ValueError(f"set_wind: speed {tuple(speed.shape)} / direction {tuple(direction.shape)}: scalars, [{n}], "
                                 f"[{self.H}, {self.W}] or [{n}, {self.H}, {self.W}]")
            flags = shapes[tuple(speed.shape)] | _lib.SF_WIND_DEVICE
            lead = (n,) if flags & _lib.SF_WIND_FIELD == 0 else (n, self.H, self.W)
            if tuple(speed.shape) != lead:              # one value / one field for every listed table
                speed, direction = speed.expand(lead).contiguous(), direction.expand(lead).contiguous()
            torch.cuda.synchronize(speed.device)
            u, d = C.c_void_p(speed.data_ptr()), C.c_void_p(direction.data_ptr())
        else:
            sp, dr = np.asarray(speed, dtype=np.float64), np.asarray(direction, dtype=np.float64)
            if sp.ndim == 0 or dr.ndim == 0:            # (one of the two the same everywhere)
                sp, dr = np.broadcast_arrays(sp, dr)
            if sp.shape != dr.shape or sp.shape not in shapes:
                raise ValueError(f"set_wind: speed {sp.shape} / direction {dr.shape}: scalars, [{n}], [{self.H}, {self.W}] or "
                                 f"[{n}, {self.H}, {self.W}]")
            flags = shapes[sp.shape]
            lead = (n,) if flags == 0 else (n, self.H, self.W)
            speed, direction = (np.ascontiguousarray(np.broadcast_to(a, lead)) for a in (sp, dr))
            u, d = _ptr(speed), _ptr(direction)
        self._chk(self._L.sf_set_wind(self._h, n, None if e is None else _ptr(e), u, d, flags))
        if on_device[0] and self.async_mode:
            self._blobs_in_flight.append((speed, direction))

    def set_wind_schedule(self, envs, segments):
        """Uniform winds by the episode's time, decided on the device (``sf_set_wind_schedule``).  ``segments``:
        rows ``(first_update, speed ft/min, direction degrees)`` - one list for every environment of ``envs`` (None: all), or one
        list per environment, all of the same length; the first row starts at update 0, the starts increase strictly, at most 16
        rows; an empty list clears.  The wind changes where a stepping call begins, never inside one: a call runs entirely under the
        wind of its environments' update counts at its start.  Needs a ``per_env_terrain`` handle."""
        e = np.arange(self.n_envs, dtype=np.int32) if envs is None else self._env_list(envs, "envs")
        n = int(e.shape[0])
        rows = list(segments)
        if rows and isinstance(rows[0], (list, tuple)) and rows[0] and isinstance(rows[0][0], (list, tuple)):
            if len(rows) != n:
                raise ValueError(f"set_wind_schedule: {len(rows)} schedules for {n} environments")
            per = [list(r) for r in rows]
        else:
            per = [rows] * n
        K = len(per[0]) if n else 0
        if any(len(r) != K for r in per):
            raise ValueError("set_wind_schedule: every environment of one call takes the same number of segments")
        segs = (_lib.SfWindSeg * max(n * K, 1))()
        for i, r in enumerate(per):
            for k, (first, u, d) in enumerate(r):
                segs[i * K + k] = _lib.SfWindSeg(int(first), 0, float(u), float(d))
        self._chk(self._L.sf_set_wind_schedule(self._h, n, _ptr(e), K, C.cast(segs, C.c_void_p)))

    def set_wind_lab(self, cache=True, timed=False):
        """Laboratory (``sf_set_wind_lab``): the cache of wind-independent terms off / on; HIP events around every wind change."""
        self._chk(self._L.sf_set_wind_lab(self._h, int(bool(cache)), int(bool(timed))))

    def wind_ms(self):
        """GPU milliseconds of the last timed wind change or schedule pass (``sf_get_wind_ms``)."""
        ms = C.c_float(0.0)
        self._chk(self._L.sf_get_wind_ms(self._h, C.byref(ms)))
        return ms.value

    def attribute_data(self, env=0):
        """``FireSimulation.get_attribute_data`` (simfire/sim/simulation.py:376-403) from the layers
        in GPU memory: w_0 / delta / M_x float32, sigma uint32, elevation / wind float64."""
        shp = (self.H, self.W)
        out = {"w_0": np.empty(shp, np.float32), "sigma": np.empty(shp, np.uint32), "delta": np.empty(shp, np.float32),
               "M_x": np.empty(shp, np.float32), "elevation": np.empty(shp, np.float64),
               "wind_speed": np.empty(shp, np.float64), "wind_direction": np.empty(shp, np.float64)}
        self._chk(self._L.sf_get_attribute_data(self._h, int(env), *[_ptr(out[k]) for k in (
            "w_0", "sigma", "delta", "M_x", "elevation", "wind_speed", "wind_direction")], 0))
        return out

    def attribute_data_torch(self, envs=None):
        """The same planes as torch tensors [len(envs), H, W] on this GPU (no host round trip);
        sigma as int32 (torch has no uint32 arithmetic; the values are < 2^31)."""
        import torch
        envs = list(range(self.n_envs)) if envs is None else [int(e) for e in envs]
        dev = f"cuda:{self.params.device}"
        n = len(envs)
        out = {"w_0": torch.empty((n, self.H, self.W), dtype=torch.float32, device=dev),
               "sigma": torch.empty((n, self.H, self.W), dtype=torch.int32, device=dev),
               "delta": torch.empty((n, self.H, self.W), dtype=torch.float32, device=dev),
               "M_x": torch.empty((n, self.H, self.W), dtype=torch.float32, device=dev),
               "elevation": torch.empty((n, self.H, self.W), dtype=torch.float64, device=dev),
               "wind_speed": torch.empty((n, self.H, self.W), dtype=torch.float64, device=dev),
               "wind_direction": torch.empty((n, self.H, self.W), dtype=torch.float64, device=dev)}
        torch.cuda.synchronize(dev)
        for i, e in enumerate(envs):
            self._chk(self._L.sf_get_attribute_data(self._h, e, *[C.c_void_p(out[k][i].data_ptr()) for k in (
                "w_0", "sigma", "delta", "M_x", "elevation", "wind_speed", "wind_direction")], 1))
        return out

    def observe(self, channels, envs=None, normalize=True, pool=1, pool_mode="mean", crop=None, centers=None, agents=None, pad=0.0,
                dtype=None, out=None):
        """The observation of ``envs`` (default: all, in order; repeats allowed) as a torch tensor [n, C, oh, ow] on this GPU, written by
        one launch (``sf_observe``) from whichever cell plane is current - nothing is converted, no state of the
        handle changes.  ``channels``: names of ``observe.CHANNELS``.  ``crop=(h, w)`` around ``centers`` [n, 2] = (column, row),
        ``pool`` f (mean or max, per channel with a dict), ``agents`` [n, k, 3] = (column, row, id); host arrays or CUDA int32 tensors.
        ``out``: a tensor to fill instead of a new one.  Torch's queued work is waited for before the handle's stream writes ``out``; in
        async mode the call only enqueues and the tensors are kept alive until ``sync()``."""
        import torch
        from .observe import ObsSpec
        spec = ObsSpec(channels, self.n_envs, self.H, self.W, envs=envs, normalize=normalize, pool=pool, pool_mode=pool_mode, crop=crop,
                       centers=centers, agents=agents, pad=pad, dtype=dtype, out=out)
        dev = torch.device(f"cuda:{self.params.device}")
        for t in spec.device_tensors() + ([out] if out is not None else []):
            if t.device != dev:
                raise ValueError(f"observe: a tensor on {t.device}, the simulation runs on {dev}")
        if out is None:
            out = torch.empty(spec.shape, dtype=spec.dtype, device=dev)
        p = spec.params()
        torch.cuda.synchronize(dev)
        self._chk(self._L.sf_observe(self._h, C.byref(p), spec.n, spec.envs_ptr(), C.c_void_p(out.data_ptr())))
        if self.async_mode:
            self._blobs_in_flight.extend([out] + spec.device_tensors())
        return out

    # ---------------------------------------------------------------- distance fields
    DIST_FAR = _lib.SF_DIST_FAR
    DIST_MAX_POINTS = _lib.SF_DIST_MAX_POINTS

    @staticmethod
    def _status_mask(who, status, what="status"):
        """A set of BurnStatus values as the mask the library takes (bit s = BurnStatus s, 1..63): ``status`` is that mask, a member,
        a name, or an iterable of members, names or ints.  ``ValueError`` (named after the caller, ``who``) on anything else."""
        from .enums import BurnStatus

        def bit(s):
            if isinstance(s, str):
                if s not in BurnStatus.__members__:
                    raise ValueError(f"{who}: unknown BurnStatus name {s!r}")
                return 1 << int(BurnStatus[s])
            if isinstance(s, (bool, float)) or not isinstance(s, (int, np.integer)) or not 0 <= int(s) <= 5:
                raise ValueError(f"{who}: {s!r} is no BurnStatus (a member, a name or 0..5)")
            return 1 << int(s)
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

    @staticmethod
    def _distance_request(status, max_dist=None, max_d2=None, dtype="float32", scale=1.0, scratch_bytes=0):
        """The checked scalar arguments of ``distance``: (status mask, max_d2, dtype code, scale, scratch_bytes).  ``ValueError`` on
        anything the library would refuse, before it is called."""
        mask = FireEngine._status_mask("distance", status)
        if max_dist is not None and max_d2 is not None:
            raise ValueError("distance: give max_dist or max_d2, not both")
        d2 = 0
        if max_dist is not None:
            if isinstance(max_dist, (bool, float)) or not isinstance(max_dist, (int, np.integer)) or not 1 <= int(max_dist) <= 46340:
                raise ValueError(f"distance: max_dist must be an integer number of cells 1..46340 or None, got {max_dist!r}")
            d2 = int(max_dist) ** 2
        elif max_d2 is not None:
            if isinstance(max_d2, (bool, float)) or not isinstance(max_d2, (int, np.integer)) or not 1 <= int(max_d2) <= 2 ** 31 - 1:
                raise ValueError(f"distance: max_d2 must be an integer 1..2**31 - 1 or None, got {max_d2!r}")
            d2 = int(max_d2)
        name = getattr(dtype, "name", None) or str(dtype).replace("torch.", "")
        if name not in ("int32", "float32"):
            raise ValueError(f"distance: dtype must be 'int32' or 'float32', got {dtype!r}")
        try:
            sc = float(scale)
        except (TypeError, ValueError):
            raise ValueError(f"distance: scale must be a number, got {scale!r}") from None
        if not np.isfinite(sc) or sc <= 0.0:
            raise ValueError(f"distance: scale must be finite and > 0, got {scale!r}")
        if isinstance(scratch_bytes, (bool, float)) or not isinstance(scratch_bytes, (int, np.integer)) or int(scratch_bytes) < 0:
            raise ValueError(f"distance: scratch_bytes must be an integer >= 0, got {scratch_bytes!r}")
        return mask, d2, (_lib.SF_DIST_I32 if name == "int32" else _lib.SF_DIST_F32), sc, int(scratch_bytes)

    def distance(self, status, envs=None, max_dist=None, points=None, dtype="float32", scale=1.0, out=None, scratch_bytes=0, max_d2=None):
        """How far the cells - or ``points`` - of ``envs`` (default: all, in order; any order, repeats allowed) are from the nearest cell
        whose BurnStatus ``status`` selects (``sf_distance``), exact, read from whichever cell plane is current -
        nothing is converted, no state of the handle changes.  ``status``: a mask (bit s = BurnStatus s, 1..63) or an iterable of
        ``BurnStatus`` members, names or ints.  ``max_dist``: an integer number of cells R, values are capped at R (``max_d2`` = R * R;
        the keyword ``max_d2`` takes a cap that is no square); ``None``: no cap, and a grid without a selected cell gives ``DIST_FAR``
        squared.  ``dtype``: "int32" - the squared distance - or "float32": ``sqrt(d2) / scale``.  ``points``: a torch CUDA int32
        tensor [n, k, 3] = (column, row, id) with k <= 256, e.g. ``agents_device()``; an entry with id <= 0 or off the grid gives -1.
        Returns a torch tensor [n, H, W], or [n, k] with points, on this GPU; ``out``: a tensor to fill instead.  ``scratch_bytes``: the
        most scratch the call may use (0: 128 MiB); less than one environment's plane (H * pitch * 2 bytes) is a ``ValueError``.  Torch's
        queued work is waited for first; in async mode the call only enqueues: the tensor is complete after ``sync()`` and kept alive
        until then."""
        mask, d2, code, sc, scratch = self._distance_request(status, max_dist, max_d2, dtype, scale, scratch_bytes)
        if envs is None:
            e = np.arange(self.n_envs, dtype=np.int32)
        else:
            e = np.asarray(envs)
            if e.ndim != 1 or (e.size and e.dtype.kind not in "iu"):
                raise ValueError("distance: envs must be a list of environment numbers")
            e = np.ascontiguousarray(e, dtype=np.int32)
            if e.size and (e.min() < 0 or e.max() >= self.n_envs):
                raise ValueError(f"distance: environment {int(e[(e < 0) | (e >= self.n_envs)][0])} out of range (n_envs = {self.n_envs})")
        n = int(e.shape[0])
        import torch
        dev = torch.device(f"cuda:{self.params.device}")
        k = 0
        tensors = []
        if points is not None:
            if not isinstance(points, torch.Tensor) or not points.is_cuda or points.dtype != torch.int32 or points.dim() != 3 \
                    or points.shape[0] != n or points.shape[2] != 3 or not 1 <= points.shape[1] <= self.DIST_MAX_POINTS:
                raise ValueError(f"distance: points must be a CUDA int32 tensor of shape ({n}, k, 3) with 1 <= k <= {self.DIST_MAX_POINTS}")
            if points.device != dev:
                raise ValueError(f"distance: points on {points.device}, the simulation runs on {dev}")
            points = points.contiguous()
            k = int(points.shape[1])
            tensors.append(points)
        shape = (n, k) if k else (n, self.H, self.W)
        tdtype = torch.int32 if code == _lib.SF_DIST_I32 else torch.float32
        if out is None:
            out = torch.empty(shape, dtype=tdtype, device=dev)
        elif not isinstance(out, torch.Tensor) or out.dtype != tdtype or tuple(out.shape) != shape or out.device != dev or not out.is_contiguous():
            raise ValueError(f"distance: out must be a contiguous {tdtype} tensor of shape {shape} on {dev}")
        plane = self.H * ((self.W + 15) // 16 * 16) * 2
        if 0 < scratch < plane:
            raise ValueError(f"distance: scratch_bytes {scratch} is less than one environment's plane ({plane} bytes)")
        if n == 0:
            return out
        p = _lib.SfDistParams(status_mask=mask, max_d2=d2, dtype=code, k=k, scale=sc, points=points.data_ptr() if k else None,
                              scratch_bytes=scratch)
        torch.cuda.synchronize(dev)
        self._chk(self._L.sf_distance(self._h, C.byref(p), n, _ptr(e), C.c_void_p(out.data_ptr())))
        if self.async_mode:
            self._blobs_in_flight.extend([out] + tensors)
        return out

    # ---------------------------------------------------------------- reach of the fire
    REACH_DEFAULT_SCRATCH = 256 << 20

    @staticmethod
    def _reach_request(source=("BURNING",), through=("UNBURNED",), connectivity=None, max_rounds=0, scratch_bytes=0):
        """The checked scalar arguments of ``reach``: (source mask, through mask, connectivity code, max_rounds, scratch_bytes).
        ``ValueError`` on anything the library would refuse, before it is called."""
        src = FireEngine._status_mask("reach", source, "source")
        thr = FireEngine._status_mask("reach", through, "through")
        if src & thr:
            raise ValueError(f"reach: source (mask {src}) and through (mask {thr}) must not share a BurnStatus")
        if connectivity is None:
            conn = 0
        elif isinstance(connectivity, (bool, float)) or not isinstance(connectivity, (int, np.integer)) or int(connectivity) not in (0, 4, 8):
            raise ValueError(f"reach: connectivity must be None (the simulation's diagonal_spread), 4 or 8, got {connectivity!r}")
        else:
            conn = int(connectivity)
        if isinstance(max_rounds, (bool, float)) or not isinstance(max_rounds, (int, np.integer)) or not 0 <= int(max_rounds) < 2 ** 31:
            raise ValueError(f"reach: max_rounds must be an integer >= 0, got {max_rounds!r}")
        if isinstance(scratch_bytes, (bool, float)) or not isinstance(scratch_bytes, (int, np.integer)) or int(scratch_bytes) < 0:
            raise ValueError(f"reach: scratch_bytes must be an integer >= 0, got {scratch_bytes!r}")
        return src, thr, conn, int(max_rounds), int(scratch_bytes)

    def reach_scratch_bytes(self):
        """Bytes of scratch ``reach`` needs per listed environment of a chunk: two bit planes and the halo of the bands."""
        bands = ((self.H + 15) // 16) * (((self.W + 15) // 16 * 16 + 63) // 64)
        return (bands * 16 * 16 + bands * 20 + 255) // 256 * 256

    def reach(self, source=("BURNING",), through=("UNBURNED",), envs=None, connectivity=None, passable=None, points=None, count=True,
              value=False, mask=False, seeds=False, rounds=False, max_rounds=0, scratch_bytes=0):
        """What the fire of ``envs`` (default: all, in order; any order, repeats allowed) can still get to (``sf_reach``; DESIGN.md
        section 23): the flood fill of the cells whose BurnStatus ``source`` selects through the cells ``through`` selects - and, with
        ``passable`` (a uint8 CUDA tensor [H, W] for all or [n_envs, H, W] indexed by environment number), only where it is not 0 -
        over the 8- or 4-neighbourhood (``connectivity``; None: the simulation's ``diagonal_spread``).  ``source`` / ``through``: masks
        (bit s = BurnStatus s) or iterables of ``BurnStatus`` members, names or ints, as for ``distance``; they must not overlap.  With
        through = UNBURNED and the three lines the reach holds every cell that can ever burn as long as only stepping changes the map:
        an upper bound, not a forecast.  Read from whichever cell plane is current; no state of the handle changes.
        Returns a dict of torch tensors on this GPU, one per output asked for: ``count`` int32 [n], ``value`` int64 [n] (the value
        plane of ``values_set`` summed over the reach), ``mask`` uint8 [n, H, W], ``seeds`` int32 [n] (source cells), ``rounds`` int32
        [n] (negative: ``max_rounds`` > 0 stopped the fill early, the outputs are a subset), and with ``points`` - int32 CUDA
        [n, k, 3] = (column, row, id), k <= 256, e.g. ``agents_device()`` - ``point_in`` int32 [n, k]: 1 / 0, -1 for id <= 0 or off
        the grid.  ``scratch_bytes``: the most scratch the call may use (0: 256 MiB); less than ``reach_scratch_bytes()`` is a
        ``ValueError``.  Torch's queued work is waited for first; in async mode the call only enqueues: the tensors are complete after
        ``sync()`` and kept alive until then."""
        src, thr, conn, mr, scratch = self._reach_request(source, through, connectivity, max_rounds, scratch_bytes)
        if envs is None:
            e = np.arange(self.n_envs, dtype=np.int32)
        else:
            e = np.asarray(envs)
            if e.ndim != 1 or (e.size and e.dtype.kind not in "iu"):
                raise ValueError("reach: envs must be a list of environment numbers")
            e = np.ascontiguousarray(e, dtype=np.int32)
            if e.size and (e.min() < 0 or e.max() >= self.n_envs):
                raise ValueError(f"reach: environment {int(e[(e < 0) | (e >= self.n_envs)][0])} out of range (n_envs = {self.n_envs})")
        n = int(e.shape[0])
        want = dict(count=count, value=value, mask=mask, seeds=seeds, rounds=rounds)
        for name, flag in want.items():
            if not isinstance(flag, (bool, np.bool_)):
                raise ValueError(f"reach: {name} must be True or False, got {flag!r}")
        if not any(want.values()) and points is None:
            raise ValueError("reach: nothing asked for (count, value, mask, seeds, rounds or points)")
        if value and not getattr(self, "values_on", False):
            raise ValueError("reach: value needs a value plane (values_set)")
        need = self.reach_scratch_bytes()
        if 0 < scratch < need:
            raise ValueError(f"reach: scratch_bytes {scratch} is less than one environment's need ({need} bytes)")
        if self.W > 8192:
            raise ValueError(f"reach: grids wider than 8192 cells are not supported (width {self.W})")
        import torch
        if passable is not None and (not isinstance(passable, torch.Tensor) or not passable.is_cuda or passable.dtype != torch.uint8
                                     or tuple(passable.shape) not in ((self.H, self.W), (self.n_envs, self.H, self.W))):
            raise ValueError(f"reach: passable must be a CUDA uint8 tensor of shape ({self.H}, {self.W}) or ({self.n_envs}, {self.H}, {self.W})")
        if points is not None and (not isinstance(points, torch.Tensor) or not points.is_cuda or points.dtype != torch.int32 or points.dim() != 3
                                   or points.shape[0] != n or points.shape[2] != 3 or not 1 <= points.shape[1] <= self.DIST_MAX_POINTS):
            raise ValueError(f"reach: points must be a CUDA int32 tensor of shape ({n}, k, 3) with 1 <= k <= {self.DIST_MAX_POINTS}")
        dev = torch.device(f"cuda:{self.params.device}")
        tensors = []
        per_env = 0
        if passable is not None:
            if passable.device != dev:
                raise ValueError(f"reach: passable on {passable.device}, the simulation runs on {dev}")
            per_env = int(passable.dim() == 3)
            passable = passable.contiguous()
            tensors.append(passable)
        k = 0
        if points is not None:
            if points.device != dev:
                raise ValueError(f"reach: points on {points.device}, the simulation runs on {dev}")
            points = points.contiguous()
            k = int(points.shape[1])
            tensors.append(points)
        res = {}
        if count:
            res["count"] = torch.empty((n,), dtype=torch.int32, device=dev)
        if value:
            res["value"] = torch.empty((n,), dtype=torch.int64, device=dev)
        if mask:
            res["mask"] = torch.empty((n, self.H, self.W), dtype=torch.uint8, device=dev)
        if seeds:
            res["seeds"] = torch.empty((n,), dtype=torch.int32, device=dev)
        if k:
            res["point_in"] = torch.empty((n, k), dtype=torch.int32, device=dev)
        if rounds:
            res["rounds"] = torch.empty((n,), dtype=torch.int32, device=dev)
        if n == 0:
            return res
        p = _lib.SfReachParams(source_mask=src, through_mask=thr, connectivity=conn, k=k, max_rounds=mr, passable_per_env=per_env,
                               passable=passable.data_ptr() if passable is not None else None, points=points.data_ptr() if k else None,
                               scratch_bytes=scratch)
        o = _lib.SfReachOut(**{name: t.data_ptr() for name, t in res.items()})
        torch.cuda.synchronize(dev)
        self._chk(self._L.sf_reach(self._h, C.byref(p), n, _ptr(e), C.byref(o)))
        if self.async_mode:
            self._blobs_in_flight.extend(list(res.values()) + tensors)
        return res

    def render(self, envs=None, scale=1, mode=None, background="fuel", contours=True, terrain_rgb=None, agents=None, channels_last=True,
               history=None, out=None):
        """Frames of ``envs`` (default: all, in order; repeats allowed) as a uint8 torch tensor [n, oh, ow, 3] (or [n, 3, oh, ow]) on
        this GPU, written by one launch (``sf_render``) from whichever cell plane is current - or, with
        ``history=(first, count)``, from the history ring (count frames per environment, updates first .. first + count - 1).  No state
        of the handle changes.  ``agents`` [n, k, 3] = (column, row, id) as for ``observe``.  ``out``: a tensor to fill instead of a new
        one.  In async mode the call only enqueues and the tensors are kept alive until ``sync()``."""
        import torch
        from .render import RenderSpec
        spec = RenderSpec(self.n_envs, self.H, self.W, envs=envs, scale=scale, mode=mode, background=background, contours=contours,
                          terrain_rgb=terrain_rgb, agents=agents, channels_last=channels_last, history=history, out=out)
        dev = torch.device(f"cuda:{self.params.device}")
        for t in spec.device_tensors() + ([out] if out is not None else []):
            if t.device != dev:
                raise ValueError(f"render: a tensor on {t.device}, the simulation runs on {dev}")
        if out is None:
            out = torch.empty(spec.shape, dtype=torch.uint8, device=dev)
        p = spec.params()
        torch.cuda.synchronize(dev)
        self._chk(self._L.sf_render(self._h, C.byref(p), spec.n, spec.envs_ptr(), C.c_void_p(out.data_ptr())))
        if self.async_mode:
            self._blobs_in_flight.extend([out] + spec.device_tensors())
        return out

    def cell_layout(self):
        """1 = the resident launch's blocked cell plane is current, 0 = the row-major planes (what ``observe`` reads)."""
        v = C.c_int32()
        self._chk(self._L.sf_cell_layout(self._h, C.byref(v)))
        return int(v.value)

    # ---------------------------------------------------------------- per-update history
    def enable_history(self, capacity):
        """Record the fire map after every executed update (what ``_save_data`` appends to
        ``fire_map.npy``, simfire/sim/simulation.py:548-549) in GPU memory: a ring int8
        [n_envs, capacity, H, W] (update u in slot u mod capacity); 0 switches it off."""
        self._chk(self._L.sf_enable_history(self._h, int(capacity)))

    def history(self, env=0, first=0, count=None):
        """int8 [count, H, W]: maps after updates ``first .. first+count-1`` of ``env`` since its reset."""
        if count is None:
            st, _ = self.status()
            count = int(st[env, 1]) - int(first)
        out = np.empty((max(int(count), 0), self.H, self.W), dtype=np.int8)
        if out.shape[0]:
            self._chk(self._L.sf_get_history(self._h, int(env), int(first), int(count), _ptr(out)))
        return out

    # ---------------------------------------------------------------- arrival times
    def enable_arrival(self, on=True):
        """Record for every cell the update that created its first sprite (``sf_enable_arrival``): kept by a pass behind the step
        launches, a call of n updates then runs in pieces of at most ``max_fire_duration``.  Allowed at any time: cells that burned
        out earlier stay "never", sprites live now carry their true update.  ``on=False`` frees the plane."""
        self._chk(self._L.sf_enable_arrival(self._h, int(bool(on))))
        self.arrival_on = bool(on)

    def arrival(self, env=0):
        """int32 [H, W]: the update that ignited each cell of ``env`` - 0 the reset's ignition, -1 never (``sf_get_arrival``).
        An update index, not minutes."""
        out = np.empty((self.H, self.W), dtype=np.int32)
        self._chk(self._L.sf_get_arrival(self._h, int(env), _ptr(out)))
        return out

    def arrival_torch(self):
        """Zero-copy view of the raw plane as a torch int32 tensor [n_envs, H, W] on this GPU: update + 1, 0 = never
        (``sf_arrival_device``).  Read-only; the handle's stream is waited for first.  Valid until ``enable_arrival(False)``."""
        import torch
        p, pitch, stride = C.c_void_p(), C.c_int64(), C.c_int64()
        self._chk(self._L.sf_arrival_device(self._h, C.byref(p), C.byref(pitch), C.byref(stride)))
        self.sync()
        shape, strides = (self.n_envs, self.H, self.W), (int(stride.value), int(pitch.value), 4)

        class _Plane:
            __cuda_array_interface__ = {"shape": shape, "typestr": "<i4", "data": (p.value, False), "version": 2, "strides": strides}
        return torch.as_tensor(_Plane(), device=f"cuda:{self.params.device}")

    # ---------------------------------------------------------------- values at risk
    VALUE_MAX = 1 << 24

    def values_set(self, values, per_env=None):
        """A value plane (``sf_values_set``): while it is set the device keeps ``damage[e]``, the sum of the values of every cell the
        fire of environment ``e`` has reached in this episode (the cells with ``arrival(e) >= 0``).  ``values``: int32 ``[H, W]`` for
        every environment or ``[n_envs, H, W]``, |value| <= 2**24 - a NumPy array, or a contiguous int32 CUDA tensor on this GPU
        (torch's queued work on it is waited for first; the handle keeps a copy of its own).  ``per_env``: inferred from the number
        of dimensions when None.  ``None`` switches the feature off and frees its memory.  Needs ``enable_arrival``; allowed at any
        time (the damage is recounted under the new plane).  Shape, dtype and range errors of a NumPy plane are ``ValueError`` before
        any device call; the range of a tensor is checked on the device (``ValueError`` too, and the handle is as it was)."""
        if values is None:
            self._chk(self._L.sf_values_set(self._h, None, 0, 0))
            self.values_on = False
            return
        on_device = getattr(values, "is_cuda", None) is not None
        shape = tuple(values.shape)
        if per_env is None:
            per_env = len(shape) == 3
        want = (self.n_envs, self.H, self.W) if per_env else (self.H, self.W)
        if shape != want:
            raise ValueError(f"values_set: the plane must have shape {want}, got {shape}")
        if on_device:
            import torch
            if not values.is_cuda or values.device.index != self.params.device or values.dtype != torch.int32 or not values.is_contiguous():
                raise ValueError(f"values_set: a tensor must be a contiguous int32 CUDA tensor on device {self.params.device}")
            torch.cuda.synchronize(values.device)
            self._chk(self._L.sf_values_set(self._h, C.c_void_p(values.data_ptr()), int(bool(per_env)), 1))
        else:
            a = np.asarray(values)
            if a.dtype.kind not in "iu":
                raise ValueError(f"values_set: values must be integers, got {a.dtype}")
            if a.size and (int(a.max()) > self.VALUE_MAX or int(a.min()) < -self.VALUE_MAX):
                raise ValueError("values_set: a value is outside -2**24 .. 2**24")
            a = np.ascontiguousarray(a, dtype=np.int32)
            self._chk(self._L.sf_values_set(self._h, _ptr(a), int(bool(per_env)), 0))
        self.values_on = True

    def damage(self):
        """int64 [n_envs]: the value the fire of every environment has reached in its episode (``sf_values_get``).  Complete on return."""
        out = np.empty(self.n_envs, dtype=np.int64)
        self._chk(self._L.sf_values_get(self._h, _ptr(out)))
        return out

    def values_torch(self):
        """Zero-copy torch views ``(damage, tick_loss)``, int64 [n_envs] each, on this GPU (``sf_values_device``): the damage as
        ``damage()`` returns it, and what the last ``agents_step`` tick added to it (0 for an environment that was not running before
        the tick; after an auto-reset tick still the finished episode's last tick).  Read-only; the handle's stream is waited for
        first.  Valid until the next ``values_set``."""
        import torch
        d, stride, t = C.c_void_p(), C.c_int64(), C.c_void_p()
        self._chk(self._L.sf_values_device(self._h, C.byref(d), C.byref(stride), C.byref(t)))
        self.sync()
        shape, strides = (self.n_envs,), (int(stride.value),)

        class _Damage:
            __cuda_array_interface__ = {"shape": shape, "typestr": "<i8", "data": (d.value, False), "version": 2, "strides": strides}

        class _Loss:
            __cuda_array_interface__ = {"shape": shape, "typestr": "<i8", "data": (t.value, False), "version": 2, "strides": None}
        dev = f"cuda:{self.params.device}"
        return torch.as_tensor(_Damage(), device=dev), torch.as_tensor(_Loss(), device=dev)

    def set_values_dense(self, on=True):
        """Laboratory: the value pass always in its dense form (one thread per cell) instead of walking the vector bitmap."""
        self._chk(self._L.sf_set_values_dense(self._h, int(bool(on))))

    def value_passes(self):
        """Laboratory: (sparse, dense) value passes made since the handle was created; recounts are dense ones."""
        out = np.zeros(2, dtype=np.int64)
        self._chk(self._L.sf_get_value_passes(self._h, _ptr(out)))
        return int(out[0]), int(out[1])

    # ---------------------------------------------------------------- ensemble statistics
    ENS_MAX_HORIZONS = _lib.ENS_MAX_HORIZONS

    def _ensemble_request(self, members, horizons):
        """The checked arguments of ``ensemble_stats``: (int32 [G, K] contiguous, list of horizons).  ``ValueError`` on anything the
        library would refuse, before it is called."""
        if members is None:
            m = np.arange(self.n_envs, dtype=np.int32).reshape(1, -1)
        else:
            m = np.asarray(members)
            if m.ndim != 2 or m.dtype.kind not in "iu":
                raise ValueError(f"ensemble_stats: members must be a 2-D integer array [groups, members], got {m.dtype} {m.shape}")
        G, K = m.shape
        if G < 1 or not 1 <= K <= 65535 or G * K > 1 << 20:
            raise ValueError(f"ensemble_stats: {G} groups of {K} members (G >= 1, 1 <= K <= 65535, G * K <= 2**20)")
        if int(m.min()) < 0 or int(m.max()) >= self.n_envs:
            raise ValueError(f"ensemble_stats: members holds an environment outside 0..{self.n_envs - 1}")
        try:
            hz = [int(h) for h in np.asarray(horizons).reshape(-1).tolist()]
        except (TypeError, ValueError):
            raise ValueError(f"ensemble_stats: horizons must be integers, got {horizons!r}") from None
        if np.asarray(horizons).dtype.kind not in "iu" or not 1 <= len(hz) <= self.ENS_MAX_HORIZONS:
            raise ValueError(f"ensemble_stats: 1 to {self.ENS_MAX_HORIZONS} integer horizons, got {horizons!r}")
        for t, h in enumerate(hz):
            if h < -1 or h > 2 ** 31 - 1 or (h == -1 and t != len(hz) - 1):
                raise ValueError(f"ensemble_stats: horizon {h} (>= 0; -1, no limit, only as the last)")
            if t and h != -1 and h <= hz[t - 1]:
                raise ValueError(f"ensemble_stats: the horizons must be strictly ascending, got {hz}")
        return np.ascontiguousarray(m, dtype=np.int32), hz

    def ensemble_stats(self, members, horizons=(-1,), count=False, prob=True, first=False, mean=False, loss=False):
        """Per-cell statistics over groups of environments (``sf_ensemble_stats``), read off the arrival planes
        as they stand by one launch.  ``members``: [G, K] environment numbers (anything ``np.asarray`` makes a 2-D integer array of;
        an environment may stand in several groups and more than once in one, and counts as often as listed); ``None``: one group
        of every environment.  ``horizons``: 1 to 8 update indices, strictly ascending, the last may be -1 (no limit); a member has
        reached a cell by horizon h if its arrival there is an update <= h.  Returns a dict of torch tensors on this GPU with the
        outputs asked for: ``count`` int32 [G, T, H, W], ``prob`` float32 [G, T, H, W] = count / K, ``first`` int32 [G, H, W] (the
        earliest arrival by the last horizon, -1 none), ``mean`` float32 [G, H, W] (the mean arrival of the members that arrived,
        -1.0 none) and ``loss`` int64 [G, T] (the values of the cells each member reached, summed over the group; needs
        ``values_set``).  Needs ``enable_arrival``.  No state of the handle changes.  Torch's queued work is waited for first; in
        async mode the call only enqueues: the tensors are complete after ``sync()`` and kept alive until then."""
        m, hz = self._ensemble_request(members, horizons)
        want = [n for n, on in (("count", count), ("prob", prob), ("first", first), ("mean", mean), ("loss", loss)) if on]
        if not want:
            raise ValueError("ensemble_stats: no output asked for")
        call = self._L.sf_ensemble_stats
        import torch
        dev = torch.device(f"cuda:{self.params.device}")
        G, K, T = m.shape[0], m.shape[1], len(hz)
        shapes = {"count": ((G, T, self.H, self.W), torch.int32), "prob": ((G, T, self.H, self.W), torch.float32),
                  "first": ((G, self.H, self.W), torch.int32), "mean": ((G, self.H, self.W), torch.float32), "loss": ((G, T), torch.int64)}
        res = {n: torch.empty(shapes[n][0], dtype=shapes[n][1], device=dev) for n in want}
        p = _lib.SfEnsembleParams(n_groups=G, group_size=K, n_horizons=T)
        for t, h in enumerate(hz):
            p.horizons[t] = h
        o = _lib.SfEnsembleOut(**{n: res[n].data_ptr() for n in want})
        torch.cuda.current_stream(dev).synchronize()       # (torch may still be using the memory it has just handed out again)
        self._chk(call(self._h, C.byref(p), _ptr(m), C.byref(o)))
        if self.async_mode:
            self._blobs_in_flight.extend(res.values())
        return res

    def set_arrival_dense(self, on=True):
        """Laboratory: the arrival pass always in its dense form (one thread per cell) instead of walking the vector bitmap."""
        self._chk(self._L.sf_set_arrival_dense(self._h, int(bool(on))))

    def time_arrival_pass(self):
        """Laboratory: GPU milliseconds of one more arrival pass over the state as it stands (it changes nothing)."""
        ms = C.c_float(0.0)
        self._chk(self._L.sf_time_arrival_pass(self._h, C.byref(ms)))
        return float(ms.value)

    def arrival_passes(self):
        """Laboratory: (sparse, dense) arrival passes made since the handle was created."""
        out = np.zeros(2, dtype=np.int64)
        self._chk(self._L.sf_get_arrival_passes(self._h, _ptr(out)))
        return int(out[0]), int(out[1])

    def set_generic(self, on=True):
        """Per-cell kernel instead of the tiled SWAR kernels (always on for max_fire_duration > 5)."""
        self._chk(self._L.sf_set_generic(self._h, int(bool(on))))

    def set_dense(self, dense=True):
        """Visit every tile every step (cross-check of the tile activity map)."""
        self._chk(self._L.sf_set_dense(self._h, int(bool(dense))))

    def fire_map_device(self):
        """(device pointer, row pitch, env stride) of the uint8 status plane (BurnStatus values)."""
        p, pitch, stride = C.c_void_p(), C.c_int64(), C.c_int64()
        self._chk(self._L.sf_fire_map_device(self._h, C.byref(p), C.byref(pitch), C.byref(stride)))
        return p.value, int(pitch.value), int(stride.value)

    def fire_maps_torch(self):
        """Zero-copy view of all fire_maps as a torch uint8 tensor [n_envs, H, W] on this GPU (RL
        observations without a PCIe round trip).  The bytes are the BurnStatus values.  Read-only, and call it
        again after stepping: the plane is refreshed by this call (a snapshot while the resident launch keeps the
        cells in its blocked plane; same address every time)."""
        import torch
        ptr, pitch, stride = self.fire_map_device()
        self.sync()

        class _Plane:
            __cuda_array_interface__ = {"shape": (self.n_envs, self.H, self.W), "typestr": "|u1",
                                        "data": (ptr, False), "version": 2, "strides": (stride, pitch, 1)}
        return torch.as_tensor(_Plane(), device=f"cuda:{self.params.device}")

    def status_device_ptr(self):
        """Device address of the int32 [E, 8] result block (after ``update_status_device``)."""
        p = C.c_void_p()
        self._chk(self._L.sf_status_device(self._h, C.byref(p)))
        return p.value

    def copy_status_to(self, device_ptr):
        """Refresh the result block and copy it into device memory at ``device_ptr``
        (int32 [n_envs, 8]), e.g. ``tensor.data_ptr()`` of a torch tensor on the same GPU."""
        self._chk(self._L.sf_copy_status_to(self._h, C.c_void_p(int(device_ptr))))

    def rollout(self, n, device_ptr):
        """``step(n)`` without a wait of its own + ``copy_status_to(device_ptr)`` as one call: what a harness does
        between two policy evaluations."""
        self._chk(self._L.sf_rollout(self._h, int(n), C.c_void_p(int(device_ptr))))

    def set_result_sink(self, device_ptr):
        """Register device memory (int32 [n_envs, 8], e.g. ``tensor.data_ptr()``; ``None`` unregisters) that every
        refresh of the result block also writes - the resident launch of ``step(n >= 2)`` leaves the block there
        itself, so ``copy_status_to(same pointer)`` after a rollout is only the wait.  Keep the tensor alive."""
        self._chk(self._L.sf_set_result_sink(self._h, C.c_void_p(int(device_ptr) if device_ptr else None)))

    # ---- the one collective of the path, through the C ABI (hosts without torch.distributed)
    @staticmethod
    def comm_unique_id():
        """128 opaque bytes made by rank 0, to be handed to every rank's ``comm_init`` by the host's own means."""
        buf = C.create_string_buffer(128)
        _lib.check(_lib.load().sf_comm_unique_id(C.cast(buf, C.c_void_p)))
        return buf.raw

    def comm_init(self, rank, world_size, unique_id):
        """Collective: join the RCCL communicator of the result-block all-gather (one process per GPU, the same
        number of environments on every rank)."""
        if len(unique_id) != 128:
            raise ValueError("unique_id must be the 128 bytes of comm_unique_id()")
        buf = C.create_string_buffer(bytes(unique_id), 128)
        self._chk(self._L.sf_comm_init(self._h, int(rank), int(world_size), C.cast(buf, C.c_void_p)))

    def allgather_status(self, device_ptr):
        """Refresh this rank's result block and all-gather the blocks of all ranks over RCCL into device memory
        int32 [world_size * n_envs, 8] (rank-major), on the handle's stream; returns when it is there."""
        self._chk(self._L.sf_allgather_status(self._h, C.c_void_p(int(device_ptr))))

    def comm_destroy(self):
        self._chk(self._L.sf_comm_destroy(self._h))

    def enable_counters(self, on=True):
        """Statistics for the roofline accounting; off by default (they cost atomics)."""
        self._chk(self._L.sf_enable_counters(self._h, int(bool(on))))

    def counters(self, reset=False):
        """dict(active_cell_updates, ignitions, frontier_items) summed since the last reset."""
        out = np.zeros(16, dtype=np.int64)
        self._chk(self._L.sf_get_counters(self._h, _ptr(out), int(bool(reset))))
        return dict(active_cell_updates=int(out[0]), ignitions=int(out[1]), frontier_items=int(out[2]),
                    active_waves=int(out[3]), frontier_walks=int(out[4]), vectors=int(out[5]),
                    team_boundaries=int(out[6] & 0xFFFFFFFF), team_boundaries_one_l2=int(out[6] >> 32), team_boundary_clocks=int(out[7]),
                    window_updates=int(out[8]), window_waves_looking=int(out[9]))

    def update_status_device(self):
        self._chk(self._L.sf_update_status_device(self._h))


def compute_ros(arrays, device=0):
    """17 float32 vectors -> R float64 through ``sf_compute_ros``."""
    L = _lib.load()
    arrs = [np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1)) for a in arrays]
    if len(arrs) != 17:
        raise ValueError("compute_rate_of_spread takes 17 arrays")
    n = arrs[0].shape[0]
    for a in arrs:
        if a.shape[0] != n:
            raise ValueError("all inputs must have the same length")
    out = np.zeros(n, dtype=np.float64)
    _lib.check(L.sf_compute_ros(n, *[_ptr(a) for a in arrs], _ptr(out), int(device)))
    return out
