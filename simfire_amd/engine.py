"""``FireEngine``: object wrapper around one ``sf_sim`` handle of the C ABI.

This is the only module that touches the HIP library; the reference-shaped classes in
``fire.py`` / ``simulation.py`` are written on top of it.  Arrays cross the boundary as
NumPy host arrays (copied during the call) or as torch CUDA tensors, read and written in place; torch is imported only by the
methods that take or return one.  Layout (binding map): argument checks in ``_args.py``, one request class per feature
(``observe.py``, ``render.py``, ``distance.py``, ``reach.py``, ``walk.py``, ``escape.py``, ``travel.py``, ``behavior.py``, ``perimeter.py``, ``influence.py``, ``components.py``, ``ensemble.py``), and one frame, ``_device_call``, for every call
that hands the library a tensor.
"""
import ctypes as C
import os

import numpy as np

from . import _args, _lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _device_view(ptr, shape, typestr, strides, device):
    """Zero-copy torch view of device memory the library owns: ``ptr`` as a tensor of ``shape``, ``typestr`` ("<i4") and byte
    ``strides`` (None: contiguous) on ``device``.  Valid for as long as the library keeps the allocation."""
    import torch

    class _View:
        __cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2, "strides": strides}
    return torch.as_tensor(_View(), device=device)


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
        self._blobs_in_flight = []          # tensors an enqueued call may still touch (async mode: _device_call; released by sync)
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

    @property
    def torch_device(self):
        """The GPU of this handle as a ``torch.device``."""
        import torch
        return torch.device(f"cuda:{self.params.device}")

    def _device_call(self, fn, *args, tensors=(), wait="device"):
        """The frame of every call that hands the library torch tensors: ``fn(handle, *args)`` checked, around it what ``tensors``
        - every tensor the call reads or writes - need.  The handle works on its own stream, so torch's queued work (which may
        still write a tensor, or still use the memory a fresh one was given) is waited for first: ``wait="device"`` the whole
        device, ``wait="stream"`` torch's current stream only.  In async mode the call only enqueues, so the tensors are kept alive
        until ``sync`` (the caching allocator must not hand their memory out while the handle's stream may still touch it).
        Without tensors it is the plain checked call."""
        if len(tensors):
            import torch
            if wait == "device":
                torch.cuda.synchronize(tensors[0].device)
            else:
                torch.cuda.current_stream(tensors[0].device).synchronize()
        self._chk(fn(self._h, *args))
        if self.async_mode:
            self._blobs_in_flight.extend(tensors)

    def _outputs(self, who, spec, out=None, dtype=None):
        """The output of a checked request (``observe.ObsSpec`` and its kin) on this GPU: ``out`` or a new tensor of ``spec.shape``
        and ``dtype`` - or, where the request names several (``spec.outputs``: name -> (shape, dtype)), a dict of new ones - after
        checking that ``out`` and the tensors the request reads (``spec.device_tensors()``) live on this GPU too."""
        import torch
        dev = self.torch_device
        for t in spec.device_tensors() + ([out] if out is not None else []):
            if t.device != dev:
                raise ValueError(f"{who}: a tensor on {t.device}, the simulation runs on {dev}")

        def new(shape, dt):
            return torch.empty(shape, dtype=getattr(torch, dt) if isinstance(dt, str) else dt, device=dev)
        if dtype is None:
            return {name: new(*sd) for name, sd in spec.outputs.items()}
        return out if out is not None else new(spec.shape, dtype)

    def _get(self, fn, ctype, *args):
        """One scalar out-parameter of C type ``ctype``: ``fn(handle, *args, &v)`` checked, ``v`` as a Python number."""
        v = ctype()
        self._chk(fn(self._h, *args, C.byref(v)))
        return v.value

    def _switch(self, fn, on):
        """An on / off flag: ``fn(handle, 0 | 1)`` checked; returns the flag as a bool."""
        self._chk(fn(self._h, int(bool(on))))
        return bool(on)

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

    def reset_envs(self, envs, xy):
        """New episodes in ``envs`` (environment ``envs[i]`` ignites at ``xy[i]`` = (x, y)), one launch for all of them
        (``sf_reset_envs``).  An environment may repeat: its last ignition wins.  In async mode the call only enqueues."""
        e = _args.env_list(envs, who="reset_envs")
        a = _args.cells(xy, (e.shape[0], 2), self.H, self.W, "reset_envs", "ignition")
        _args.env_range(e, self.n_envs, "reset_envs", exc=IndexError)
        if e.size:
            self._chk(self._L.sf_reset_envs(self._h, int(e.shape[0]), _ptr(e), _ptr(a)))

    def reset_where(self, mask=None, xy=None):
        """New episodes in every environment that is not running (``mask=None``; decided on the device, nothing is read back) or that
        ``mask`` selects (a torch CUDA uint8 / bool tensor [n_envs] on this GPU); environment e ignites at ``xy[e]`` - a NumPy array
        or a torch CUDA int32 tensor [n_envs, 2] (``sf_reset_where``).  A device ignition off the grid leaves its environment
        untouched.  Torch's queued work on the tensors is waited for first; in async mode they are kept alive until ``sync``."""
        tensors = []
        if mask is not None:
            mask = _args.env_mask(mask, self.n_envs, "reset_where")
            tensors.append(mask)
        if xy is None:
            raise ValueError("reset_where: xy (the ignitions, [n_envs, 2]) is required")
        if getattr(xy, "is_cuda", False):
            xy = _args.cuda_tensor(xy, "reset_where: a device xy", ("int32",), [(self.n_envs, 2)]).contiguous()
            tensors.append(xy)
            xy_ptr, xy_dev = C.c_void_p(xy.data_ptr()), 1
        else:
            a = _args.cells(xy, (self.n_envs, 2), self.H, self.W, "reset_where", "ignition")
            xy_ptr, xy_dev = _ptr(a), 0
        mask_ptr = C.c_void_p(mask.data_ptr()) if mask is not None else None
        self._device_call(self._L.sf_reset_where, mask_ptr, xy_ptr, xy_dev, tensors=tensors)

    def time_resets(self, on=True):
        """Measurement only: record HIP events around the launches of every ``reset_envs`` / ``reset_where`` (``sf_time_resets``)."""
        self._switch(self._L.sf_time_resets, on)

    def reset_ms(self):
        """GPU milliseconds of the last timed batched reset's launches (``sf_get_reset_ms``; waits for them)."""
        return self._get(self._L.sf_get_reset_ms, C.c_float)

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
            ign = _args.cells(ignitions, (self.n_envs, 2), self.H, self.W, "agents_create", "ignition")
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
        a = _args.cells(xy, (e.shape[0], k, 2), self.H, self.W, "agents_place")
        _args.env_range(e, self.n_envs, "agents_place")
        if e.size:
            self._chk(self._L.sf_agents_place(self._h, int(e.shape[0]), _ptr(e), _ptr(a), int(bool(also_start))))

    def agents_step(self, actions, reward=None, done=None, terms=None, final_len=None, final_ret=None):
        """One tick for every environment from a device action tensor, nothing read back (``sf_agents_step``).  ``actions``: torch
        CUDA int32 [n_envs, n_agents], word = move + 5 * interact.  Outputs, each optional, torch CUDA tensors on this GPU:
        ``reward`` float32 [n_envs], ``done`` uint8 / bool [n_envs], ``terms`` int32 [n_envs, 4], ``final_len`` int32 [n_envs],
        ``final_ret`` float64 [n_envs].  Torch's queued work on the tensors is waited for first; in async mode the call only
        enqueues and the tensors are kept alive until ``sync``."""
        k = self.n_agents
        if not k:
            raise _lib.SimfireHipError("agents_step: call agents_create first")
        E, dev = self.n_envs, self.torch_device
        _args.cuda_tensor(actions, "agents_step: actions", ("int32",), [(E, k)], device=dev, contiguous=True)
        o, tensors = _lib.SfAgentOut(), [actions]
        for t, name, dtypes, shape in ((reward, "reward", ("float32",), (E,)), (done, "done", ("uint8", "bool"), (E,)),
                                       (terms, "terms", ("int32",), (E, 4)), (final_len, "final_len", ("int32",), (E,)),
                                       (final_ret, "final_ret", ("float64",), (E,))):
            if t is not None:
                setattr(o, name, _args.cuda_tensor(t, f"agents_step: {name}", dtypes, [shape], device=dev, contiguous=True).data_ptr())
                tensors.append(t)
        self._device_call(self._L.sf_agents_step, C.c_void_p(actions.data_ptr()), C.byref(o), tensors=tensors)

    def agents_device(self):
        """Zero-copy torch view int32 [n_envs, n_agents, 3] = (column, row, id) of the agent positions on this GPU: what ``observe``
        / ``render`` take as ``agents``.  Valid until the next ``agents_create``; read it after ``sync`` in async mode."""
        if not self.n_agents:
            raise _lib.SimfireHipError("agents_device: call agents_create first")
        p = self._get(self._L.sf_agents_device, C.c_void_p)
        return _device_view(p, (self.n_envs, self.n_agents, 3), "<i4", None, self.torch_device)

    # ------------------------------------------------------------------ drawn episodes
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
            p.ign_box[:] = _args.box(ignition_box, self.H, self.W, "episodes_set", "ignition_box")
        if agent_box is not None:
            flags |= _lib.SF_EP_AGENTS
            p.agent_box[:] = _args.box(agent_box, self.H, self.W, "episodes_set", "agent_box")
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
            tensors.append(_args.env_mask(mask, self.n_envs, "episodes_begin"))
        mask_ptr = C.c_void_p(tensors[0].data_ptr()) if tensors else None
        self._device_call(self._L.sf_episodes_begin, mask_ptr, int(bool(all)), tensors=tensors)

    def episodes_torch(self):
        """Zero-copy torch views of what the last draw of every environment made (``sf_episodes_device``): ``index`` int32 [n_envs]
        (the NEXT episode's index; the bits of a uint32), ``ignition`` int32 [n_envs, 2] = (x, y), ``wind`` float64 [n_envs, 2] =
        (U ft/min, U_dir degrees).  They report draws, not a later ``set_wind``, ``reset_envs`` or ``copy_envs``.  Read-only; the
        handle's stream is waited for first.  Valid until the next ``episodes_set``."""
        ptrs = [C.c_void_p(), C.c_void_p(), C.c_void_p()]
        self._chk(self._L.sf_episodes_device(self._h, *[C.byref(p) for p in ptrs]))
        self.sync()
        E, dev = self.n_envs, self.torch_device
        return dict(index=_device_view(ptrs[0].value, (E,), "<i4", None, dev), ignition=_device_view(ptrs[1].value, (E, 2), "<i4", None, dev),
                    wind=_device_view(ptrs[2].value, (E, 2), "<f8", None, dev))

    def apply_mitigation(self, pts):
        """pts: rows (env, x, y, type)."""
        q = np.ascontiguousarray(np.asarray(pts, dtype=np.int32).reshape(-1, 4))
        if len(q):
            self._chk(self._L.sf_apply_mitigation(self._h, _ptr(q), len(q)))

    def apply_mitigation_torch(self, pts):
        """The same scatter for a torch int32 tensor [n, 4] (env, x, y, type) that already lives on this
        GPU (e.g. the actions of a policy): no host round trip; rows with an out-of-range field are
        skipped.  The caller orders its own stream before this call (a device-wide wait or an
        event), the library then works on its own stream."""
        import torch
        if pts.dtype != torch.int32 or pts.dim() != 2 or pts.shape[1] != 4 or not pts.is_cuda:
            raise ValueError("expected a CUDA int32 tensor of shape [n, 4]")
        pts = pts.contiguous()
        if pts.shape[0]:
            self._chk(self._L.sf_apply_mitigation_device(self._h, C.c_void_p(pts.data_ptr()), int(pts.shape[0])))
            # one slot, replaced by the next call - not _device_call's list: a rollout makes these calls (and step_mitigated's)
            # many times in async mode without a sync(), and the list would grow with every one
            self._keep_alive = pts          # until the next call: the scatter may still be queued (async mode)

    def ignite(self, points):
        """New fire in running environments (``sf_ignite``): rows ``(env, x, y)`` - ``[n, 3]``, or ``[n, 4]``
        with a reserved 0 behind.  Every listed cell that is UNBURNED becomes BURNING with a sprite of age 0, as if the last update
        had ignited it; rows on other cells, or in environments that are not running, are skipped.  Argument errors are raised
        before any device call: ``IndexError`` for an environment out of range, ``ValueError`` otherwise.  In async mode the call
        only enqueues."""
        q = _args.ignite_rows(points, self.n_envs, self.H, self.W, "ignite")
        if len(q):
            self._chk(self._L.sf_ignite(self._h, _ptr(q), len(q)))

    def ignite_torch(self, points):
        """The same for a contiguous torch int32 tensor ``[n, 4]`` = (env, x, y, 0) that already lives on this GPU
        (``sf_ignite_device``): no host round trip; rows with an out-of-range field or a fourth field that is not 0 are skipped.
        The library works on a stream of its own and waits for nothing here: the caller orders its own stream before this call (a
        device-wide wait, a stream wait or an event), as for ``apply_mitigation_torch`` - which is why a tensor that is not
        contiguous is refused, not copied (the copy would run on torch's stream behind the caller's back).  The tensor is kept
        alive until the next call."""
        points = _args.cuda_tensor(points, "ignite_torch: points", ("int32",), [(None, 4)], contiguous=True)
        if points.device != self.torch_device:
            raise ValueError(f"ignite_torch: a tensor on {points.device}, the simulation runs on {self.torch_device}")
        if points.shape[0]:
            self._chk(self._L.sf_ignite_device(self._h, C.c_void_p(points.data_ptr()), int(points.shape[0])))
            self._keep_alive_ignite = points      # one slot, as apply_mitigation_torch keeps its own: the launch may still be queued (async mode)

    def time_ignites(self, on=True):
        """Measurement only: record HIP events around the scatter launch of every ``ignite`` / ``ignite_torch`` (``sf_time_ignites``)."""
        self._switch(self._L.sf_time_ignites, on)

    def ignite_ms(self):
        """GPU milliseconds of the last timed ignition's scatter launch (``sf_get_ignite_ms``; waits for it)."""
        return self._get(self._L.sf_get_ignite_ms, C.c_float)

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
        return self._get(self._L.sf_step_timed, C.c_float, int(n))

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
        """The legacy lenient list: a scalar is a list of one, anything that casts to int32 passes, the range is the library's."""
        return _args.env_list(envs, name=name, lenient=True)

    def copy_envs(self, src, dst, terrain=False):
        """Environment ``dst[i]`` becomes environment ``src[i]`` (one launch for all pairs; ``sf_copy_envs``).  ``terrain``: on a
        per-environment-terrain handle ``dst`` also takes ``src``'s layers and R table."""
        s, d = self._env_list(src, "src"), self._env_list(dst, "dst")
        if s.shape != d.shape:
            raise ValueError(f"src and dst differ in length ({s.shape[0]} != {d.shape[0]})")
        self._chk(self._L.sf_copy_envs(self._h, _ptr(s), _ptr(d), int(s.shape[0]), 1 if terrain else 0))

    def state_bytes(self):
        """Bytes of one environment's state blob (``sf_state_bytes``)."""
        return self._get(self._L.sf_state_bytes, C.c_int64)

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
        self._device_call(self._L.sf_save_state, int(e.shape[0]), _ptr(e), C.c_void_p(out.data_ptr()), 1, tensors=[out])
        return out

    def load_state(self, envs, blob):
        """Environment ``envs[i]`` takes the state of blob i (numpy uint8 [n, state_bytes()] or a contiguous CUDA tensor holding the
        blobs back to back; ``sf_load_state``).  A blob from another geometry or configuration raises ValueError and changes nothing."""
        e = self._env_list(envs, "envs")
        nb = self.state_bytes()
        if getattr(blob, "is_cuda", False):
            if not blob.is_contiguous() or blob.numel() * blob.element_size() < e.shape[0] * nb:
                raise ValueError(f"blob must be a contiguous CUDA tensor of at least {e.shape[0] * nb} bytes")
            self._device_call(self._L.sf_load_state, int(e.shape[0]), _ptr(e), C.c_void_p(blob.data_ptr()), 1, tensors=[blob])
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
        return self._get(self._L.sf_memory_bytes, C.c_int64)

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
        self.async_mode = self._switch(self._L.sf_set_async, on)

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
        return self._get(self._L.sf_loop_restarts, C.c_int32)

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
        return self._get(self._L.sf_get_last_launches, C.c_int32)

    def team_fallbacks(self):
        """Teams of a fixed size that found at their start that not all members were resident and whose environment was stepped by
        member 0 alone (same results; since the handle was created)."""
        return self._get(self._L.sf_get_team_fallbacks, C.c_int32)

    def get_tuning(self, name):
        return self._get(self._L.sf_get_tuning, C.c_int32, _lib.TUNE[name])

    def set_prune_after_quit(self, on=True):
        """Environments that QUIT on the runtime check keep pruning when stepped again (fire.py:631-643)."""
        self.prune_after_quit = self._switch(self._L.sf_set_prune_after_quit, on)

    def last_launch_kind(self):
        """0 k_select + k_step, 1 fused launch per step, 2 resident launch (k_run), 3 per-cell kernel, 4 the window kernel k_win in front of
        k_run (more environments than CUs, young fires), -1 none yet."""
        return self._get(self._L.sf_last_step_launch, C.c_int32)

    # neighbour order of the parent masks = adj_locs of simfire/utils/graph.py:125-134
    GRAPH_DX = (+1, +1, 0, -1, -1, -1, 0, +1)
    GRAPH_DY = (0, +1, +1, +1, 0, -1, -1, -1)

    def enable_spread_graph(self, on=True):
        """Record the fire-spread graph (FireSpreadGraph, simfire/utils/graph.py) as parent masks."""
        self.spread_graph_on = self._switch(self._L.sf_enable_spread_graph, on)
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
        tensors = []
        if on_device[0]:
            for t, name in ((speed, "speed"), (direction, "direction")):
                _args.cuda_tensor(t, f"set_wind: {name}", ("float64",), device=self.torch_device, contiguous=True)
            if tuple(speed.shape) != tuple(direction.shape) or tuple(speed.shape) not in shapes:
                raise ValueError(f"set_wind: speed {tuple(speed.shape)} / direction {tuple(direction.shape)}: scalars, [{n}], "
                                 f"[{self.H}, {self.W}] or [{n}, {self.H}, {self.W}]")
            flags = shapes[tuple(speed.shape)] | _lib.SF_WIND_DEVICE
            lead = (n,) if flags & _lib.SF_WIND_FIELD == 0 else (n, self.H, self.W)
            if tuple(speed.shape) != lead:              # one value / one field for every listed table
                speed, direction = speed.expand(lead).contiguous(), direction.expand(lead).contiguous()
            tensors = [speed, direction]
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
        self._device_call(self._L.sf_set_wind, n, None if e is None else _ptr(e), u, d, flags, tensors=tensors)

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
        return self._get(self._L.sf_get_wind_ms, C.c_float)

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
        keys = {"w_0": torch.float32, "sigma": torch.int32, "delta": torch.float32, "M_x": torch.float32, "elevation": torch.float64,
                "wind_speed": torch.float64, "wind_direction": torch.float64}
        out = {k: torch.empty((len(envs), self.H, self.W), dtype=dt, device=self.torch_device) for k, dt in keys.items()}
        for i, e in enumerate(envs):
            planes = [out[k][i] for k in keys]
            self._device_call(self._L.sf_get_attribute_data, e, *[C.c_void_p(t.data_ptr()) for t in planes], 1, tensors=planes)
        return out

    def observe(self, channels, envs=None, normalize=True, pool=1, pool_mode="mean", crop=None, centers=None, agents=None, pad=0.0,
                dtype=None, out=None):
        """The observation of ``envs`` (default: all, in order; repeats allowed) as a torch tensor [n, C, oh, ow] on this GPU, written by
        one launch (``sf_observe``) from whichever cell plane is current - nothing is converted, no state of the
        handle changes.  ``channels``: names of ``observe.CHANNELS``.  ``crop=(h, w)`` around ``centers`` [n, 2] = (column, row),
        ``pool`` f (mean or max, per channel with a dict), ``agents`` [n, k, 3] = (column, row, id); host arrays or CUDA int32 tensors.
        ``out``: a tensor to fill instead of a new one.  Torch's queued work is waited for before the handle's stream writes ``out``; in
        async mode the call only enqueues and the tensors are kept alive until ``sync()``."""
        from .observe import ObsSpec
        spec = ObsSpec(channels, self.n_envs, self.H, self.W, envs=envs, normalize=normalize, pool=pool, pool_mode=pool_mode, crop=crop,
                       centers=centers, agents=agents, pad=pad, dtype=dtype, out=out)
        out, p = self._outputs("observe", spec, out, spec.dtype), spec.params()
        self._device_call(self._L.sf_observe, C.byref(p), spec.n, _ptr(spec.envs), C.c_void_p(out.data_ptr()),
                          tensors=[out] + spec.device_tensors())
        return out

    # ---------------------------------------------------------------- distance fields
    DIST_FAR = _lib.SF_DIST_FAR
    DIST_MAX_POINTS = _lib.SF_DIST_MAX_POINTS

    @staticmethod
    def _status_mask(who, status, what="status"):
        return _args.status_mask(who, status, what)

    @staticmethod
    def _distance_request(status, max_dist=None, max_d2=None, dtype="float32", scale=1.0, scratch_bytes=0):
        from . import distance
        return distance.request(status, max_dist, max_d2, dtype, scale, scratch_bytes)

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
        from .distance import DistSpec
        spec = DistSpec(self.n_envs, self.H, self.W, status, envs=envs, max_dist=max_dist, points=points, dtype=dtype, scale=scale, out=out,
                        scratch_bytes=scratch_bytes, max_d2=max_d2)
        out = self._outputs("distance", spec, out, spec.dtype)
        if spec.n:
            p = spec.params()
            self._device_call(self._L.sf_distance, C.byref(p), spec.n, _ptr(spec.envs), C.c_void_p(out.data_ptr()),
                              tensors=[out] + spec.device_tensors())
        return out

    # ---------------------------------------------------------------- reach of the fire
    REACH_DEFAULT_SCRATCH = 256 << 20

    @staticmethod
    def _reach_request(source=("BURNING",), through=("UNBURNED",), connectivity=None, max_rounds=0, scratch_bytes=0):
        from . import reach
        return reach.request(source, through, connectivity, max_rounds, scratch_bytes)

    def reach_scratch_bytes(self):
        from . import reach
        return reach.scratch_need(self.H, self.W)

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
        from .reach import ReachSpec
        spec = ReachSpec(self.n_envs, self.H, self.W, getattr(self, "values_on", False), source=source, through=through, envs=envs,
                         connectivity=connectivity, passable=passable, points=points, count=count, value=value, mask=mask, seeds=seeds,
                         rounds=rounds, max_rounds=max_rounds, scratch_bytes=scratch_bytes)
        res = self._outputs("reach", spec)
        if spec.n:
            p, o = spec.params(), spec.out(res)
            self._device_call(self._L.sf_reach, C.byref(p), spec.n, _ptr(spec.envs), C.byref(o), tensors=list(res.values()) + spec.device_tensors())
        return res

    # ---------------------------------------------------------------- walking distance
    WALK_FAR, WALK_BLOCKED = _lib.SF_WALK_FAR, _lib.SF_WALK_BLOCKED

    def walk_scratch_bytes(self):
        from . import walk
        return walk.scratch_need(self.H, self.W)

    def walk(self, target=("BURNING",), through=("UNBURNED",), envs=None, connectivity=4, passable=None, targets=None, points=None,
             max_moves=None, plane=False, step=False, reached=False, levels=False, scratch_bytes=0):
        """How many moves a walker of ``envs`` (default: all, in order; any order, repeats allowed) needs to step onto a target cell
        when it enters only walkable cells, one cell per move (``sf_walk``).  Targets: the cells whose
        BurnStatus ``target`` selects, or - with ``targets``, a uint8 CUDA tensor [H, W] for all or [n_envs, H, W] indexed by
        environment number - the cells where that is not 0 (``target`` may then be ``None``).  Walkable: the cells ``through`` selects
        and, with ``passable`` (same forms), only where it is not 0.  ``target`` / ``through``: masks (bit s = BurnStatus s) or
        iterables of ``BurnStatus`` members, names or ints; they may overlap, a cell that is both is a target.  ``connectivity`` 4
        (the agents' moves) or 8.  Read from whichever cell plane is current; no state of the handle changes.
        Returns a dict of int32 torch tensors on this GPU, one per output asked for: with ``plane`` ``moves`` [n, H, W] (the number of
        moves; ``WALK_FAR`` on walkable cells no route leaves, ``WALK_BLOCKED`` = -1 on cells that are neither), with ``points`` -
        int32 CUDA [n, k, 3] = (column, row, id), k <= 256, e.g. ``agents_device()`` - ``point_moves`` [n, k] (0 on a target, else 1 +
        the least value of a target or walkable neighbour; the point itself need not be walkable; -1 for id <= 0 or off the grid) and
        with ``step`` ``point_step`` [n, k]: the move code 1..4 (row - 1, row + 1, column - 1, column + 1) of the lowest-numbered
        neighbour on a shortest route, 0 on a target or when no move gets there; ``reached`` [n]: walkable cells with a route;
        ``levels`` [n]: the largest number of moves found.  ``max_moves`` = M: values above M, ``WALK_FAR`` included, are reported as
        M, and ``point_step`` is 0 there.  ``scratch_bytes``: the most scratch the call may use (0: 256 MiB); less than
        ``walk_scratch_bytes()`` is a ``ValueError``.  Torch's queued work is waited for first; in async mode the call only enqueues:
        the tensors are complete after ``sync()`` and kept alive until then."""
        from .walk import WalkSpec
        spec = WalkSpec(self.n_envs, self.H, self.W, target=target, through=through, envs=envs, connectivity=connectivity,
                        passable=passable, targets=targets, points=points, max_moves=max_moves, plane=plane, step=step, reached=reached,
                        levels=levels, scratch_bytes=scratch_bytes)
        res = self._outputs("walk", spec)
        if spec.n:
            p, o = spec.params(), spec.out(res)
            self._device_call(self._L.sf_walk, C.byref(p), spec.n, _ptr(spec.envs), C.byref(o), tensors=list(res.values()) + spec.device_tensors())
        return res

    # ---------------------------------------------------------------- escape routes
    ESCAPE_SAFE, ESCAPE_LOST, ESCAPE_BLOCKED = _lib.SF_ESCAPE_SAFE, _lib.SF_ESCAPE_LOST, _lib.SF_ESCAPE_BLOCKED

    def escape_scratch_bytes(self):
        from . import escape
        return escape.scratch_need(self.H, self.W)

    def escape(self, minutes, target=(), targets=None, through=("UNBURNED",), passable=None, envs=None, connectivity=4,
               minutes_per_move=None, margin_minutes=0.0, horizon_minutes=None, unreached_safe=False, points=None, plane=False,
               step=False, summary=False, scratch_bytes=0):
        """The escape slack of ``envs`` (default: all, in order; any order, repeats allowed): how many more moves a walker may wait
        where it stands and still reach a target cell, one cell per move through walkable cells, never standing on a cell at or
        after the moment the fire closes it (``sf_escape``).  ``minutes``: a float32 CUDA tensor [n, H, W],
        row i for ``envs[i]``, the closing time of every cell in minutes from now - the ``minutes`` of ``travel`` as it is.  A cell
        with T = ``minutes`` < 0 or not < ``horizon_minutes`` never closes; else its deadline is ``ceil((T - margin_minutes) /
        minutes_per_move)`` moves (at least 0), and a walker may stand on it at move index m (now: 0) while m is below that.
        ``minutes_per_move=None``: the simulation's ``update_rate`` - one move per tick of ``agents_step``.  Targets and walkable
        cells: ``target`` / ``targets`` and ``through`` / ``passable`` as for ``walk`` (``target`` may be empty with a ``targets``
        plane); targets are safe.  ``unreached_safe``: every walkable cell that never closes is a target too.  ``connectivity`` 4
        (the agents' moves) or 8.  Read from whichever cell plane is current; no state of the handle changes.
        Returns a dict of int32 torch tensors on this GPU, one per output asked for: with ``plane`` ``slack`` [n, H, W]
        (``ESCAPE_SAFE`` on targets and where no deadline binds, ``ESCAPE_LOST`` = -1 on walkable cells without a feasible route,
        ``ESCAPE_BLOCKED`` = -2 on cells that are neither); with ``points`` - int32 CUDA [n, k, 3] = (column, row, id), k <= 256,
        e.g. ``agents_device()`` - ``point_slack`` [n, k] (the point need not be walkable; -2 for id <= 0 or off the grid) and with
        ``step`` ``point_step`` [n, k]: where 0 <= slack < ``ESCAPE_SAFE``, the move code 1..4 of the lowest-numbered neighbour
        with the largest slack - following it raises the slack by at least 1 per move; 0 on a target, when lost, when the slack is
        ``ESCAPE_SAFE`` (no hurry: ``walk`` routes) and with connectivity 8; with ``summary`` ``safe``, ``escapable``, ``lost``
        (walkable non-target cells by slack) and ``top`` (the largest finite deadline) [n].  The horizon may be at most 32768 moves
        away.  ``scratch_bytes``: the most scratch the call may use (0: 1280 MiB); less than ``escape_scratch_bytes()`` is a
        ``ValueError``.  Torch's queued work is waited for first; in async mode the call only enqueues: the tensors are complete
        after ``sync()`` and kept alive until then."""
        from .escape import EscapeSpec
        spec = EscapeSpec(self.n_envs, self.H, self.W, minutes, target=target, targets=targets, through=through, passable=passable,
                          envs=envs, connectivity=connectivity,
                          minutes_per_move=float(self.params.update_rate) if minutes_per_move is None else minutes_per_move,
                          margin_minutes=margin_minutes, horizon_minutes=horizon_minutes, unreached_safe=unreached_safe, points=points,
                          plane=plane, step=step, summary=summary, scratch_bytes=scratch_bytes)
        res = self._outputs("escape", spec)
        if spec.n:
            p, o = spec.params(), spec.out(res)
            self._device_call(self._L.sf_escape, C.byref(p), spec.n, _ptr(spec.envs), C.byref(o), tensors=list(res.values()) + spec.device_tensors())
        return res

    # ---------------------------------------------------------------- fire travel time
    TRAVEL_BLOCKED = _lib.SF_TRAVEL_BLOCKED

    def travel_scratch_bytes(self):
        from . import travel
        return travel.scratch_need(self.H, self.W)

    def travel(self, source=("BURNING",), through=("UNBURNED",), envs=None, connectivity=None, passable=None, sources=None, points=None,
               max_minutes=None, plane=True, pred=False, reached=False, last=False, scratch_bytes=0, activations=False):
        """WHEN the fire of ``envs`` (default: all, in order; any order, repeats allowed) gets to every cell: the minimum travel time
        in minutes from now over the rate-of-spread table the handle holds now (``sf_travel``).  A forecast in
        continuous time over the automaton's own graph - cell c is entered from its neighbour ``SRC_OFFSETS[k]`` after
        ``pixel_scale / rt[k][c]`` minutes -, NOT the automaton: no whole updates, no burn-out of sources.  Sources: the cells whose
        BurnStatus ``source`` selects, or - with ``sources``, a uint8 CUDA tensor [H, W] for all or [n_envs, H, W] indexed by
        environment number - the cells where that is not 0 (``source`` may then be ``None``).  Passable: the cells ``through`` selects
        and, with ``passable`` (same forms), only where it is not 0 - a candidate control line costs a plane, not a fork of the
        state.  ``source`` / ``through``: masks (bit s = BurnStatus s) or iterables of ``BurnStatus`` members, names or ints; they
        may overlap, a cell that is both is a source.  ``connectivity`` 4, 8 or None (the simulation's ``diagonal_spread``).  Read
        from whichever cell plane is current; no state of the handle changes.
        Returns a dict of torch tensors on this GPU, one per output asked for: with ``plane`` ``minutes`` float32 [n, H, W] (+inf
        where no route arrives, ``TRAVEL_BLOCKED`` = -1 on cells that are neither source nor passable); with ``pred`` ``pred`` int8
        [n, H, W], the index into ``SRC_OFFSETS`` of the neighbour the fastest route comes from (-1 on sources, unreached and blocked
        cells); with ``points`` - int32 CUDA [n, k, 3] = (column, row, id), k <= 256, e.g. ``agents_device()`` - ``point_minutes``
        float32 [n, k] (the plane's value; on a blocked cell the time at which it would be reached were it passable; -1 for id <= 0
        or off the grid); ``reached`` int32 [n]: passable cells with a route; ``last`` float32 [n]: the largest finite time;
        ``activations`` int32 [n]: tiles the search loaded (measurement).  ``max_minutes`` = M: the search stops at M, values above
        M, +inf included, are reported as M and ``pred`` is -1 there.  ``scratch_bytes``: the most scratch a call without ``plane``
        may use (0: 1 GiB); less than ``travel_scratch_bytes()`` is a ``ValueError``.  Torch's queued work is waited for first; in
        async mode the call only enqueues: the tensors are complete after ``sync()`` and kept alive until then."""
        from .travel import TravelSpec
        spec = TravelSpec(self.n_envs, self.H, self.W, source=source, through=through, envs=envs, connectivity=connectivity,
                          passable=passable, sources=sources, points=points, max_minutes=max_minutes, plane=plane, pred=pred,
                          reached=reached, last=last, activations=activations, scratch_bytes=scratch_bytes)
        res = self._outputs("travel", spec)
        if spec.n:
            p, o = spec.params(), spec.out(res)
            self._device_call(self._L.sf_travel, C.byref(p), spec.n, _ptr(spec.envs), C.byref(o), tensors=list(res.values()) + spec.device_tensors())
        return res

    # ---------------------------------------------------------------- fire behaviour
    def behavior(self, envs=None, status=None, summary=("BURNING",), flame_limit=None, edges=None, points=None,
                 planes=("flame_length",), workable=False, stats=False):
        """Fireline intensity and flame length per cell of ``envs`` (default: all, in order; any order, repeats allowed) from the R
        table the handle holds now (``sf_behavior``).  Units are the reference's: feet, minutes, pounds, BTU.
        Returns a dict of torch tensors on this GPU, one per output asked for.  ``planes``: any of ``hpa`` (heat per unit area,
        BTU/ft2), ``ros`` (the head rate of spread, ft/min), ``intensity`` (Byram's, BTU/ft/s), ``flame_length`` (ft), float32
        [n, H, W], and ``head`` int8 [n, H, W]: the index into ``SRC_OFFSETS`` of the neighbour the head fire arrives from, -1 where
        nothing spreads; with ``status`` (a mask, or BurnStatus members, names or ints) the cells it does not select show 0 / -1.
        ``workable`` (needs ``flame_limit``): uint8 [n, H, W], 1 where the flame-length plane is <= ``flame_limit`` - what ``walk``
        and ``reach`` take as ``passable``.  ``stats``: over the cells ``summary`` selects ``max_flame`` and ``max_intensity``
        float32 [n] and ``classes`` int32 [n, 5], the cells with a flame length in [0, e0) [e0, e1) [e1, e2) [e2, e3) [e3, inf) for
        ``edges`` (default 4, 8, 11, 1e30 ft).  ``points`` - int32 CUDA [n, k, 3] = (column, row, id), k <= 256, e.g.
        ``agents_device()`` - gives ``point_flame`` float32 [n, k]: the largest flame length among the cells of the 3 x 3 block
        around the point that ``summary`` selects (0: none; -1 for id <= 0 or off the grid).  No state of the handle changes.
        Torch's queued work is waited for first; in async mode the call only enqueues: the tensors are complete after ``sync()``
        and kept alive until then."""
        from .behavior import BehaviorSpec
        spec = BehaviorSpec(self.n_envs, self.H, self.W, envs=envs, status=status, summary=summary, flame_limit=flame_limit, edges=edges,
                            points=points, planes=planes, workable=workable, stats=stats)
        res = self._outputs("behavior", spec)
        if spec.n:
            p, o = spec.params(), spec.out(res)
            self._device_call(self._L.sf_behavior, C.byref(p), C.byref(o), _ptr(spec.envs), spec.n, tensors=list(res.values()) + spec.device_tensors())
        return res

    # ---------------------------------------------------------------- fire perimeters
    def perimeter_scratch_bytes(self, max_edges=None):
        from . import perimeter
        return perimeter.scratch_need(self.H, self.W, perimeter.default_capacities(self.H, self.W, max_edges)[0])

    def perimeter(self, status=None, envs=None, member=None, at_update=None, connectivity=None, simplify=True, counts=True, front=False,
                  trace=False, max_edges=None, max_vertices=None, max_loops=None, scratch_bytes=0):
        """WHERE the edge of the fire of ``envs`` (default: all, in order; any order, repeats allowed) runs (``sf_perimeter``; DESIGN.md
        section 27), in integers.  The set S is exactly one of: the cells whose BurnStatus ``status`` selects (a mask, or members, names
        or ints; default BURNING | BURNED), read from whichever cell plane is current; the cells where ``member`` - a uint8 CUDA tensor
        [H, W] for all or [n_envs, H, W] indexed by environment number - is not 0; the cells the fire had reached by update
        ``at_update`` (needs ``enable_arrival``).  Cell (x, y) is the square [x, x + 1] x [y, y + 1], y down; the edge runs along the
        cracks between a cell of S and a cell outside it (off the grid counts as outside).
        Returns a dict of torch tensors on this GPU.  ``counts``: ``edges`` int32 [n], the perimeter in cell edges, and ``cells``
        int32 [n], |S|.  ``front``: uint8 [n, H, W], 1 on the cells of S with a crack.  ``trace``: the edge as polygons in canonical
        order - ``loops``, ``holes``, ``n_vertices`` int32 [n]; ``vertices`` int32 [n, max_vertices, 2] = (x, y) lattice corners;
        ``loop_start`` int32 [n, max_loops + 1] (zeroed first); ``loop_area`` int32 [n, max_loops], signed: outer loops run clockwise
        on the screen and are positive, holes negative; ``loop_edges`` int32 [n, max_loops] (``perimeter.rings`` cuts one
        environment's lists into polygons).  ``connectivity`` 4 keeps diagonal neighbours apart, 8 joins them, None is the
        simulation's ``diagonal_spread``; ``simplify`` keeps corners only.  Capacities per environment: ``max_edges`` (default
        min(2 H W + 2, 2^18)), ``max_vertices`` (default ``max_edges``), ``max_loops`` (default ``max_edges // 4``); an environment
        with more edges reports -1 in the three counts, one whose vertices or loops do not fit reports the right counts, and either
        way its rows of the four lists are left as they were.  ``scratch_bytes``: the most scratch a traced call may use (0: 1 GiB);
        less than ``perimeter_scratch_bytes(max_edges)`` is a ``ValueError``.  No state of the handle changes.  Torch's queued work
        is waited for first; in async mode the call only enqueues: the tensors are complete after ``sync()`` and kept alive until
        then."""
        from .perimeter import PerimeterSpec
        spec = PerimeterSpec(self.n_envs, self.H, self.W, status=status, envs=envs, member=member, at_update=at_update,
                             connectivity=connectivity, simplify=simplify, counts=counts, front=front, trace=trace, max_edges=max_edges,
                             max_vertices=max_vertices, max_loops=max_loops, scratch_bytes=scratch_bytes,
                             arrival_on=bool(getattr(self, "arrival_on", False)))
        res = self._outputs("perimeter", spec)
        if "loop_start" in res:
            res["loop_start"].zero_()
        if spec.n:
            p, o = spec.params(), spec.out(res)
            self._device_call(self._L.sf_perimeter, C.byref(p), spec.n, _ptr(spec.envs), C.byref(o), tensors=list(res.values()) + spec.device_tensors())
        return res

    # ---------------------------------------------------------------- fire influence
    INFLUENCE_CYCLE = _lib.SF_INFLUENCE_CYCLE

    def influence_scratch_bytes(self, cells=True, weighted=False, value=False):
        from . import influence
        return influence.scratch_need(self.H, self.W, cells=cells, weighted=weighted, value=value)

    def influence(self, pred=None, history=False, envs=None, weights=None, include=None, inclusive=False, points=None, max_route=0,
                  cells=True, value=False, pred_out=False, counts=False, scratch_bytes=0):
        """WHICH cells matter in ``envs`` (default: all, in order; any order, repeats allowed): how much of the fire passes through
        each cell of a forest of parent pointers (``sf_influence``), in integers.  The parents come from exactly
        one source: ``pred``, an int8 CUDA tensor of codes into ``travel.SRC_OFFSETS`` - [H, W] for all or [n, H, W] with row i
        belonging to ``envs[i]``, which is what ``travel(pred=True)`` returns; any byte outside 0..7 and any code that points off the
        grid is "no parent" -, or ``history=True``: the ignition tree of the episode so far, the spread-graph parent masks narrowed to
        the newest neighbour that burned strictly earlier (needs ``enable_spread_graph`` and ``enable_arrival``).  D(c) is the set of
        cells whose parent chain reaches c.
        Returns a dict of torch tensors on this GPU.  ``cells``: int32 [n, H, W], the cells of D(c) - with ``include`` (uint8 CUDA
        [H, W] or [n_envs, H, W] by environment number) only those where it is not 0, with ``inclusive`` c itself too -,
        ``INFLUENCE_CYCLE`` = -2 on the cells of a cycle (a caller's plane only).  ``value``: int64 [n, H, W], the same sum weighted
        by ``weights`` - ``"values"`` (the plane of ``values_set``) or an int32 CUDA tensor [H, W] / [n_envs, H, W] -, 0 on a cycle.
        ``pred_out``: ``pred`` int8 [n, H, W], the sanitised codes used, -1 without a parent (with ``history`` the ignition tree).
        ``counts``: ``forest`` (cells with a parent), ``roots`` (without one, with children) and ``cyclic`` int32 [n].  With
        ``points`` - int32 CUDA [n, k, 3] = (column, row, id), k <= 256, e.g. ``agents_device()`` - ``point_cells`` int32 [n, k]
        and, with weights, ``point_value`` int64 [n, k]: the plane values at the point (-1 and 0 for id <= 0 or off the grid); with
        ``max_route`` = R > 0 also ``point_route`` int32 [n, k, R] - flat cell indices row * W + column from the point's cell up
        its parent chain, -1 beyond its end - and ``point_hops`` int32 [n, k]: the route's length - 1, -2 where R cut it short (a
        longer route or a cycle), -1 for an invalid point.  ``scratch_bytes``: the most scratch the call may use (0: 1 GiB); less
        than ``influence_scratch_bytes(...)`` is a ``ValueError``.  No state of the handle changes.  Torch's queued work is waited
        for first; in async mode the call only enqueues: the tensors are complete after ``sync()`` and kept alive until then."""
        from .influence import InfluenceSpec
        spec = InfluenceSpec(self.n_envs, self.H, self.W, pred=pred, history=history, envs=envs, weights=weights, include=include,
                             inclusive=inclusive, points=points, max_route=max_route, cells=cells, value=value, pred_out=pred_out,
                             counts=counts, scratch_bytes=scratch_bytes, graph_on=self.spread_graph_on, arrival_on=self.arrival_on,
                             values_on=self.values_on)                # (spread_graph_on: the switch, not "masks exist" - masks of a graph switched off are stale)
        res = self._outputs("influence", spec)
        if spec.n:
            p, o = spec.params(), spec.out(res)
            self._device_call(self._L.sf_influence, C.byref(p), spec.n, _ptr(spec.envs), C.byref(o), tensors=list(res.values()) + spec.device_tensors())
        return res

    # ---------------------------------------------------------------- connected components
    TOUCH_BORDER = 64

    def components_scratch_bytes(self, labels=False):
        from . import components
        return components.scratch_need(self.H, self.W, labels)

    def time_components(self, on=True):
        """Measurement only: record HIP events around the memsets and launches of every ``components`` call (``sf_time_components``)."""
        self._switch(self._L.sf_time_components, on)

    def components_ms(self):
        """GPU milliseconds of the last timed ``components`` call (``sf_get_components_ms``; waits for it)."""
        return self._get(self._L.sf_get_components_ms, C.c_float)

    def components(self, select=("BURNING",), envs=None, connectivity=None, member=None, points=None, max_components=64, count=True,
                   labels=False, cells=False, value=False, first=False, bbox=False, touch=False, largest=False, selected=False,
                   scratch_bytes=0):
        """The separate fires - or pockets - of ``envs`` (default: all, in order; any order, repeats allowed): the maximal connected
        sets of the cells whose BurnStatus ``select`` selects (a mask, or members, names or ints) and, with ``member`` (a uint8 CUDA
        tensor [H, W] for all or [n_envs, H, W] indexed by environment number), only where it is not 0, over the 8- or
        4-neighbourhood (``connectivity``; None: the simulation's ``diagonal_spread``) (``sf_components``).
        Components are numbered 1..C by the row-major index of their first cell, as ``scipy.ndimage.label`` numbers them.  Read from
        whichever cell plane is current; no state of the handle changes.
        Returns a dict of torch tensors on this GPU, one per output asked for: ``count`` int32 [n] (C, also beyond
        ``max_components``), ``selected`` int32 [n], ``labels`` int32 [n, H, W] (0: not selected), ``largest`` int32 [n, 2] = (number,
        cells) over all C, ties to the lower number; one row per component for the first ``max_components`` (1..4096): ``cells``
        int32 [n, cap], ``value`` int64 [n, cap] (the value plane of ``values_set`` summed over it), ``first`` int32 [n, cap]
        (y * W + x of its first cell, -1 past C), ``bbox`` int32 [n, cap, 4] = (x0, y0, x1, y1) inclusive (-1 past C), ``touch`` int32
        [n, cap]: bit s = some cell has an unselected neighbour of BurnStatus s, bit 6 (``TOUCH_BORDER``) = some cell lies on the
        grid's border; and with ``points`` - int32 CUDA [n, k, 3] = (column, row, id), k <= 256, e.g. ``agents_device()`` -
        ``point_label`` int32 [n, k]: the label under the point, 0 not selected, -1 for id <= 0 or off the grid.
        ``scratch_bytes``: the most scratch the call may use (0: 3 GiB); less than ``components_scratch_bytes(labels)`` is a
        ``ValueError``.  Torch's queued work is waited for first; in async mode the call only enqueues: the tensors are complete after
        ``sync()`` and kept alive until then."""
        from .components import ComponentsSpec
        spec = ComponentsSpec(self.n_envs, self.H, self.W, getattr(self, "values_on", False), select=select, envs=envs,
                              connectivity=connectivity, member=member, points=points, max_components=max_components, count=count,
                              labels=labels, cells=cells, value=value, first=first, bbox=bbox, touch=touch, largest=largest,
                              selected=selected, scratch_bytes=scratch_bytes)
        res = self._outputs("components", spec)
        if spec.n:
            p, o = spec.params(), spec.out(res)
            self._device_call(self._L.sf_components, C.byref(p), spec.n, _ptr(spec.envs), C.byref(o), tensors=list(res.values()) + spec.device_tensors())
        return res

    def behavior_builds(self):
        """Measurement / tests: how many tables' parts of the heat cache ``behavior`` has built so far (``sf_get_behavior_builds``)."""
        return self._get(self._L.sf_get_behavior_builds, C.c_int64)

    def render(self, envs=None, scale=1, mode=None, background="fuel", contours=True, terrain_rgb=None, agents=None, channels_last=True,
               history=None, out=None):
        """Frames of ``envs`` (default: all, in order; repeats allowed) as a uint8 torch tensor [n, oh, ow, 3] (or [n, 3, oh, ow]) on
        this GPU, written by one launch (``sf_render``) from whichever cell plane is current - or, with
        ``history=(first, count)``, from the history ring (count frames per environment, updates first .. first + count - 1).  No state
        of the handle changes.  ``agents`` [n, k, 3] = (column, row, id) as for ``observe``.  ``out``: a tensor to fill instead of a new
        one.  In async mode the call only enqueues and the tensors are kept alive until ``sync()``."""
        from .render import RenderSpec
        spec = RenderSpec(self.n_envs, self.H, self.W, envs=envs, scale=scale, mode=mode, background=background, contours=contours,
                          terrain_rgb=terrain_rgb, agents=agents, channels_last=channels_last, history=history, out=out)
        out, p = self._outputs("render", spec, out, "uint8"), spec.params()
        self._device_call(self._L.sf_render, C.byref(p), spec.n, _ptr(spec.envs), C.c_void_p(out.data_ptr()),
                          tensors=[out] + spec.device_tensors())
        return out

    def cell_layout(self):
        """1 = the resident launch's blocked cell plane is current, 0 = the row-major planes (what ``observe`` reads)."""
        return self._get(self._L.sf_cell_layout, C.c_int32)

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
        self.arrival_on = self._switch(self._L.sf_enable_arrival, on)

    def arrival(self, env=0):
        """int32 [H, W]: the update that ignited each cell of ``env`` - 0 the reset's ignition, -1 never (``sf_get_arrival``).
        An update index, not minutes."""
        out = np.empty((self.H, self.W), dtype=np.int32)
        self._chk(self._L.sf_get_arrival(self._h, int(env), _ptr(out)))
        return out

    def arrival_torch(self):
        """Zero-copy view of the raw plane as a torch int32 tensor [n_envs, H, W] on this GPU: update + 1, 0 = never
        (``sf_arrival_device``).  Read-only; the handle's stream is waited for first.  Valid until ``enable_arrival(False)``."""
        p, pitch, stride = C.c_void_p(), C.c_int64(), C.c_int64()
        self._chk(self._L.sf_arrival_device(self._h, C.byref(p), C.byref(pitch), C.byref(stride)))
        self.sync()
        return _device_view(p.value, (self.n_envs, self.H, self.W), "<i4", (int(stride.value), int(pitch.value), 4), self.torch_device)

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
            _args.cuda_tensor(values, "values_set: a tensor", ("int32",), device=self.torch_device, contiguous=True)
            self._device_call(self._L.sf_values_set, C.c_void_p(values.data_ptr()), int(bool(per_env)), 1, tensors=[values])
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
        d, stride, t = C.c_void_p(), C.c_int64(), C.c_void_p()
        self._chk(self._L.sf_values_device(self._h, C.byref(d), C.byref(stride), C.byref(t)))
        self.sync()
        dev = self.torch_device
        return (_device_view(d.value, (self.n_envs,), "<i8", (int(stride.value),), dev), _device_view(t.value, (self.n_envs,), "<i8", None, dev))

    def set_values_dense(self, on=True):
        """Laboratory: the value pass always in its dense form (one thread per cell) instead of walking the vector bitmap."""
        self._switch(self._L.sf_set_values_dense, on)

    def value_passes(self):
        """Laboratory: (sparse, dense) value passes made since the handle was created; recounts are dense ones."""
        out = np.zeros(2, dtype=np.int64)
        self._chk(self._L.sf_get_value_passes(self._h, _ptr(out)))
        return int(out[0]), int(out[1])

    # ---------------------------------------------------------------- ensemble statistics
    ENS_MAX_HORIZONS = _lib.ENS_MAX_HORIZONS

    def _ensemble_request(self, members, horizons):
        from . import ensemble
        return ensemble.request(self.n_envs, members, horizons)

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
        from .ensemble import EnsembleSpec
        spec = EnsembleSpec(self.n_envs, self.H, self.W, members, horizons, count=count, prob=prob, first=first, mean=mean, loss=loss)
        fn = self._L.sf_ensemble_stats
        res = self._outputs("ensemble_stats", spec)
        p, o = spec.params(), spec.out(res)
        # (the current-stream wait: torch may still be using the memory it has just handed out again)
        self._device_call(fn, C.byref(p), _ptr(spec.members), C.byref(o), tensors=list(res.values()), wait="stream")
        return res

    def set_arrival_dense(self, on=True):
        """Laboratory: the arrival pass always in its dense form (one thread per cell) instead of walking the vector bitmap."""
        self._switch(self._L.sf_set_arrival_dense, on)

    def time_arrival_pass(self):
        """Laboratory: GPU milliseconds of one more arrival pass over the state as it stands (it changes nothing)."""
        return self._get(self._L.sf_time_arrival_pass, C.c_float)

    def arrival_passes(self):
        """Laboratory: (sparse, dense) arrival passes made since the handle was created."""
        out = np.zeros(2, dtype=np.int64)
        self._chk(self._L.sf_get_arrival_passes(self._h, _ptr(out)))
        return int(out[0]), int(out[1])

    def set_generic(self, on=True):
        """Per-cell kernel instead of the tiled SWAR kernels (always on for max_fire_duration > 5)."""
        self._switch(self._L.sf_set_generic, on)

    def set_dense(self, dense=True):
        """Visit every tile every step (cross-check of the tile activity map)."""
        self._switch(self._L.sf_set_dense, dense)

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
        ptr, pitch, stride = self.fire_map_device()
        self.sync()
        return _device_view(ptr, (self.n_envs, self.H, self.W), "|u1", (stride, pitch, 1), self.torch_device)

    def status_device_ptr(self):
        """Device address of the int32 [E, 8] result block (after ``update_status_device``)."""
        return self._get(self._L.sf_status_device, C.c_void_p)

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
        self._switch(self._L.sf_enable_counters, on)

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
