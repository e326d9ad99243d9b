"""ctypes binding of the C ABI declared in ``include/simfire_hip.h``.

The HIP library is built in-tree (``simfire_amd/csrc/libsimfire_hip.so``) by
``__graft_entry__.build()`` / ``python -m simfire_amd.build``.  There is no CPU fallback:
if the library is missing, importing the product path fails loudly.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SIMFIRE_HIP_LIB: another build of the same library (e.g. the phase-clock build of profiles/phase_profile.sh)
LIB_PATH = os.environ.get("SIMFIRE_HIP_LIB") or os.path.join(_HERE, "csrc", "libsimfire_hip.so")

SF_OK, SF_EINVAL, SF_ESHAPE, SF_EHIP, SF_ENOTSUP, SF_ESTATE, SF_ERCCL = 0, -1, -2, -3, -4, -5, -6


class SimfireHipError(RuntimeError):
    pass


class SfParams(C.Structure):
    _fields_ = [("n_envs", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("max_fire_duration", C.c_int32), ("diagonal_spread", C.c_int32),
                ("attenuate_line_ros", C.c_int32), ("has_max_time", C.c_int32), ("device", C.c_int32),
                ("pixel_scale", C.c_double), ("update_rate", C.c_double), ("max_time", C.c_double),
                ("h", C.c_double), ("S_T", C.c_double), ("S_e", C.c_double), ("p_p", C.c_double),
                ("M_f", C.c_double), ("per_env_terrain", C.c_int32)]


class SfCfdParams(C.Structure):
    _fields_ = [("n", C.c_int32), ("n_envs", C.c_int32), ("result_accuracy", C.c_int32), ("direction", C.c_int32),
                ("timestep_dt", C.c_double), ("viscosity", C.c_double), ("speed", C.c_double)]


OBS_MAX_CHANNELS = 32


class SfObsParams(C.Structure):
    """``sf_obs_params`` (include/simfire_hip.h)."""
    _fields_ = [("n_channels", C.c_int32), ("channels", C.c_int32 * OBS_MAX_CHANNELS), ("pool_mode", C.c_int32 * OBS_MAX_CHANNELS),
                ("normalize", C.c_int32), ("pool", C.c_int32), ("crop_h", C.c_int32), ("crop_w", C.c_int32), ("dtype", C.c_int32),
                ("centers_device", C.c_int32), ("agents_k", C.c_int32), ("agents_device", C.c_int32), ("pad", C.c_double),
                ("centers", C.c_void_p), ("agents", C.c_void_p)]


SF_GEN_NONE, SF_GEN_CONSTANT, SF_GEN_SIMPLEX = 0, 1, 2


class SfNoise(C.Structure):
    """``sf_noise`` (include/simfire_hip.h)."""
    _fields_ = [("kind", C.c_int32), ("octaves", C.c_int32), ("seed", C.c_int64), ("scale", C.c_double), ("persistence", C.c_double),
                ("lacunarity", C.c_double), ("lo", C.c_double), ("hi", C.c_double)]


class SfLayerGen(C.Structure):
    """``sf_layer_gen`` (include/simfire_hip.h): one environment's planes for ``sf_generate_layers``."""
    _fields_ = [("elevation", SfNoise), ("fuel", C.c_int32), ("reserved", C.c_int32), ("fuel_values", C.c_double * 4),
                ("wind_speed", SfNoise), ("wind_direction", SfNoise)]


SF_WIND_UNIFORM, SF_WIND_FIELD, SF_WIND_DEVICE, SF_WIND_MAX_SEGS = 0, 1, 2, 16


class SfWindSeg(C.Structure):
    """``sf_wind_seg`` (include/simfire_hip.h): from update ``first_update`` on the wind is (U ft/min, U_dir degrees)."""
    _fields_ = [("first_update", C.c_int32), ("reserved", C.c_int32), ("U", C.c_double), ("U_dir", C.c_double)]


class SfRenderParams(C.Structure):
    """``sf_render_params`` (include/simfire_hip.h)."""
    _fields_ = [("source", C.c_int32), ("first", C.c_int32), ("count", C.c_int32), ("scale", C.c_int32), ("mode", C.c_int32),
                ("background", C.c_int32), ("contours", C.c_int32), ("terrain_rgb", C.c_int32 * 3), ("channels_last", C.c_int32),
                ("agents_k", C.c_int32), ("agents_device", C.c_int32), ("agents", C.c_void_p)]


class SfAgentParams(C.Structure):
    """``sf_agent_params`` (include/simfire_hip.h)."""
    _fields_ = [("k", C.c_int32), ("n_updates", C.c_int32), ("only_unburned", C.c_int32), ("done_on_burn", C.c_int32),
                ("max_ticks", C.c_int32), ("auto_reset", C.c_int32), ("w", C.c_float * 4)]


SF_EP_IGNITION, SF_EP_LIVE_CELL, SF_EP_WIND, SF_EP_AGENTS = 1, 2, 4, 8


class SfEpisodeParams(C.Structure):
    """``sf_episode_params`` (include/simfire_hip.h): what a new episode draws on the device."""
    _fields_ = [("seed", C.c_uint64), ("flags", C.c_int32), ("reserved", C.c_int32), ("ign_box", C.c_int32 * 4),
                ("agent_box", C.c_int32 * 4), ("U", C.c_double * 2), ("U_dir", C.c_double * 2)]


class SfAgentOut(C.Structure):
    """``sf_agent_out`` (include/simfire_hip.h): device pointers, any may be null."""
    _fields_ = [("reward", C.c_void_p), ("done", C.c_void_p), ("terms", C.c_void_p), ("final_len", C.c_void_p),
                ("final_ret", C.c_void_p)]


ENS_MAX_HORIZONS = 8


class SfEnsembleParams(C.Structure):
    """``sf_ensemble_params`` (include/simfire_hip.h)."""
    _fields_ = [("n_groups", C.c_int32), ("group_size", C.c_int32), ("n_horizons", C.c_int32),
                ("horizons", C.c_int32 * ENS_MAX_HORIZONS), ("reserved", C.c_int32)]


class SfEnsembleOut(C.Structure):
    """``sf_ensemble_out`` (include/simfire_hip.h): device pointers, any may be null, not all."""
    _fields_ = [("count", C.c_void_p), ("prob", C.c_void_p), ("first", C.c_void_p), ("mean", C.c_void_p), ("loss", C.c_void_p)]


SF_DIST_FAR, SF_DIST_I32, SF_DIST_F32, SF_DIST_MAX_POINTS = 2 ** 31 - 1, 0, 1, 256


class SfDistParams(C.Structure):
    """``sf_dist_params`` (include/simfire_hip.h)."""
    _fields_ = [("status_mask", C.c_int32), ("max_d2", C.c_int32), ("dtype", C.c_int32), ("k", C.c_int32), ("scale", C.c_double),
                ("points", C.c_void_p), ("scratch_bytes", C.c_int64), ("reserved", C.c_int32 * 2)]


class SfReachParams(C.Structure):
    """``sf_reach_params`` (include/simfire_hip.h)."""
    _fields_ = [("source_mask", C.c_int32), ("through_mask", C.c_int32), ("connectivity", C.c_int32), ("k", C.c_int32),
                ("max_rounds", C.c_int32), ("passable_per_env", C.c_int32), ("passable", C.c_void_p), ("points", C.c_void_p),
                ("scratch_bytes", C.c_int64), ("reserved", C.c_int32 * 2)]


class SfReachOut(C.Structure):
    """``sf_reach_out`` (include/simfire_hip.h): device pointers, any may be null, not all."""
    _fields_ = [("count", C.c_void_p), ("value", C.c_void_p), ("mask", C.c_void_p), ("seeds", C.c_void_p), ("point_in", C.c_void_p),
                ("rounds", C.c_void_p)]


SF_WALK_FAR, SF_WALK_BLOCKED = 2 ** 31 - 1, -1


class SfWalkParams(C.Structure):
    """``sf_walk_params`` (include/simfire_hip.h)."""
    _fields_ = [("target_mask", C.c_int32), ("through_mask", C.c_int32), ("connectivity", C.c_int32), ("k", C.c_int32),
                ("max_moves", C.c_int32), ("passable_per_env", C.c_int32), ("targets_per_env", C.c_int32), ("passable", C.c_void_p),
                ("targets", C.c_void_p), ("points", C.c_void_p), ("scratch_bytes", C.c_int64), ("reserved", C.c_int32 * 2)]


class SfWalkOut(C.Structure):
    """``sf_walk_out`` (include/simfire_hip.h): device pointers, any may be null, not all."""
    _fields_ = [("moves", C.c_void_p), ("point_moves", C.c_void_p), ("point_step", C.c_void_p), ("reached", C.c_void_p),
                ("levels", C.c_void_p)]


SF_ESCAPE_SAFE, SF_ESCAPE_LOST, SF_ESCAPE_BLOCKED, SF_ESCAPE_MAX_MOVES, SF_ESCAPE_UNREACHED_SAFE = 2 ** 31 - 1, -1, -2, 32768, 1


class SfEscapeParams(C.Structure):
    """``sf_escape_params`` (include/simfire_hip.h)."""
    _fields_ = [("target_mask", C.c_int32), ("through_mask", C.c_int32), ("connectivity", C.c_int32), ("k", C.c_int32),
                ("flags", C.c_int32), ("passable_per_env", C.c_int32), ("targets_per_env", C.c_int32), ("passable", C.c_void_p),
                ("targets", C.c_void_p), ("points", C.c_void_p), ("minutes", C.c_void_p), ("minutes_per_move", C.c_double),
                ("margin_minutes", C.c_double), ("horizon_minutes", C.c_double), ("scratch_bytes", C.c_int64),
                ("reserved", C.c_int32 * 2)]


class SfEscapeOut(C.Structure):
    """``sf_escape_out`` (include/simfire_hip.h): device pointers, any may be null, not all."""
    _fields_ = [("slack", C.c_void_p), ("point_slack", C.c_void_p), ("point_step", C.c_void_p), ("safe", C.c_void_p),
                ("escapable", C.c_void_p), ("lost", C.c_void_p), ("top", C.c_void_p)]


SF_TRAVEL_BLOCKED = -1.0


class SfTravelParams(C.Structure):
    """``sf_travel_params`` (include/simfire_hip.h)."""
    _fields_ = [("source_mask", C.c_int32), ("through_mask", C.c_int32), ("connectivity", C.c_int32), ("k", C.c_int32),
                ("max_minutes", C.c_float), ("passable_per_env", C.c_int32), ("sources_per_env", C.c_int32), ("passable", C.c_void_p),
                ("sources", C.c_void_p), ("points", C.c_void_p), ("scratch_bytes", C.c_int64), ("reserved", C.c_int32 * 2)]


class SfTravelOut(C.Structure):
    """``sf_travel_out`` (include/simfire_hip.h): device pointers, any may be null, not all."""
    _fields_ = [("minutes", C.c_void_p), ("pred", C.c_void_p), ("point_minutes", C.c_void_p), ("reached", C.c_void_p),
                ("last", C.c_void_p), ("activations", C.c_void_p)]


class SfBehaviorParams(C.Structure):
    """``sf_behavior_params`` (include/simfire_hip.h)."""
    _fields_ = [("status_mask", C.c_int32), ("summary_mask", C.c_int32), ("k", C.c_int32), ("reserved", C.c_int32),
                ("flame_limit", C.c_float), ("edges", C.c_float * 4), ("points", C.c_void_p)]


class SfBehaviorOut(C.Structure):
    """``sf_behavior_out`` (include/simfire_hip.h): device pointers, any may be null, not all."""
    _fields_ = [("hpa", C.c_void_p), ("ros", C.c_void_p), ("intensity", C.c_void_p), ("flame_length", C.c_void_p), ("head", C.c_void_p),
                ("workable", C.c_void_p), ("max_flame", C.c_void_p), ("max_intensity", C.c_void_p), ("classes", C.c_void_p),
                ("point_flame", C.c_void_p)]


class SfPerimeterParams(C.Structure):
    """``sf_perimeter_params`` (include/simfire_hip.h)."""
    _fields_ = [("status_mask", C.c_int32), ("at_update", C.c_int32), ("connectivity", C.c_int32), ("simplify", C.c_int32),
                ("member_per_env", C.c_int32), ("max_edges", C.c_int32), ("max_vertices", C.c_int32), ("max_loops", C.c_int32),
                ("member", C.c_void_p), ("scratch_bytes", C.c_int64), ("reserved", C.c_int32 * 2)]


class SfPerimeterOut(C.Structure):
    """``sf_perimeter_out`` (include/simfire_hip.h): device pointers, any may be null, not all."""
    _fields_ = [("edges", C.c_void_p), ("cells", C.c_void_p), ("front", C.c_void_p), ("loops", C.c_void_p), ("holes", C.c_void_p),
                ("n_vertices", C.c_void_p), ("vertices", C.c_void_p), ("loop_start", C.c_void_p), ("loop_area", C.c_void_p),
                ("loop_edges", C.c_void_p)]


SF_INFLUENCE_PRED_PLANE, SF_INFLUENCE_PRED_HISTORY = 0, 1
SF_INFLUENCE_WEIGHT_NONE, SF_INFLUENCE_WEIGHT_VALUES, SF_INFLUENCE_WEIGHT_PLANE = 0, 1, 2
SF_INFLUENCE_CYCLE = -2


class SfInfluenceParams(C.Structure):
    """``sf_influence_params`` (include/simfire_hip.h)."""
    _fields_ = [("pred_source", C.c_int32), ("pred_per_env", C.c_int32), ("weight_mode", C.c_int32), ("weights_per_env", C.c_int32),
                ("include_per_env", C.c_int32), ("inclusive", C.c_int32), ("k", C.c_int32), ("max_route", C.c_int32),
                ("pred", C.c_void_p), ("weights", C.c_void_p), ("include", C.c_void_p), ("points", C.c_void_p),
                ("scratch_bytes", C.c_int64), ("reserved", C.c_int32 * 2)]


class SfInfluenceOut(C.Structure):
    """``sf_influence_out`` (include/simfire_hip.h): device pointers, any may be null, not all."""
    _fields_ = [("cells", C.c_void_p), ("value", C.c_void_p), ("pred", C.c_void_p), ("forest", C.c_void_p), ("roots", C.c_void_p),
                ("cyclic", C.c_void_p), ("point_cells", C.c_void_p), ("point_value", C.c_void_p), ("point_route", C.c_void_p),
                ("point_hops", C.c_void_p)]


SF_COMPONENTS_MAX = 4096


class SfComponentsParams(C.Structure):
    """``sf_components_params`` (include/simfire_hip.h)."""
    _fields_ = [("select_mask", C.c_int32), ("connectivity", C.c_int32), ("k", C.c_int32), ("max_components", C.c_int32),
                ("member_per_env", C.c_int32), ("reserved0", C.c_int32), ("member", C.c_void_p), ("points", C.c_void_p),
                ("scratch_bytes", C.c_int64), ("reserved", C.c_int32 * 2)]


class SfComponentsOut(C.Structure):
    """``sf_components_out`` (include/simfire_hip.h): device pointers, any may be null, not all."""
    _fields_ = [("count", C.c_void_p), ("selected", C.c_void_p), ("labels", C.c_void_p), ("cells", C.c_void_p), ("value", C.c_void_p),
                ("first", C.c_void_p), ("bbox", C.c_void_p), ("touch", C.c_void_p), ("largest", C.c_void_p), ("point_label", C.c_void_p)]


# name -> argtypes; every function returns int except the two string getters
_VP, _I32, _I64 = C.c_void_p, C.c_int32, C.c_int64
SIGNATURES = {
    "sf_create": [C.POINTER(SfParams), C.POINTER(_VP)],
    "sf_destroy": [_VP],
    "sf_set_layers": [_VP] + [_VP] * 7,
    "sf_set_rtable": [_VP, _VP],
    "sf_get_rtable": [_VP, _VP],
    "sf_get_slopes": [_VP, _VP, _VP],
    "sf_set_layers_env": [_VP, _I32] + [_VP] * 7,
    "sf_set_rtable_env": [_VP, _I32, _VP],
    "sf_get_rtable_env": [_VP, _I32, _VP],
    "sf_set_layers_fbfm": [_VP, _I32, _VP, _I32, _VP, _VP, _VP, _VP, _VP],
    "sf_get_attribute_data": [_VP, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I32],
    "sf_generate_layers": [_VP, _I32, _VP, _VP],
    "sf_set_wind": [_VP, _I32, _VP, _VP, _VP, _I32],
    "sf_set_wind_schedule": [_VP, _I32, _VP, _I32, _VP],
    "sf_set_wind_lab": [_VP, _I32, _I32],
    "sf_get_wind_ms": [_VP, C.POINTER(C.c_float)],
    "sf_enable_history": [_VP, _I32],
    "sf_get_history": [_VP, _I32, _I32, _I32, _VP],
    "sf_history_device": [_VP, _VP, _VP],
    "sf_enable_arrival": [_VP, _I32],
    "sf_get_arrival": [_VP, _I32, _VP],
    "sf_arrival_device": [_VP, C.POINTER(_VP), C.POINTER(_I64), C.POINTER(_I64)],
    "sf_set_arrival_dense": [_VP, _I32],
    "sf_get_arrival_passes": [_VP, _VP],
    "sf_time_arrival_pass": [_VP, C.POINTER(C.c_float)],
    "sf_values_set": [_VP, _VP, _I32, _I32],
    "sf_values_get": [_VP, _VP],
    "sf_values_device": [_VP, C.POINTER(_VP), C.POINTER(_I64), C.POINTER(_VP)],
    "sf_values_set_weight": [_VP, C.c_float, _I32],
    "sf_set_values_dense": [_VP, _I32],
    "sf_get_value_passes": [_VP, _VP],
    "sf_ensemble_stats": [_VP, C.POINTER(SfEnsembleParams), _VP, C.POINTER(SfEnsembleOut)],
    "sf_reset": [_VP, _VP],
    "sf_reset_env": [_VP, _I32, _I32, _I32],
    "sf_reset_envs": [_VP, _I32, _VP, _VP],
    "sf_reset_where": [_VP, _VP, _VP, _I32],
    "sf_agents_create": [_VP, C.POINTER(SfAgentParams), _VP],
    "sf_agents_place": [_VP, _I32, _VP, _VP, _I32],
    "sf_agents_step": [_VP, _VP, C.POINTER(SfAgentOut)],
    "sf_agents_device": [_VP, C.POINTER(_VP)],
    "sf_episodes_set": [_VP, C.POINTER(SfEpisodeParams)],
    "sf_episodes_begin": [_VP, _VP, _I32],
    "sf_episodes_device": [_VP, C.POINTER(_VP), C.POINTER(_VP), C.POINTER(_VP)],
    "sf_time_resets": [_VP, _I32],
    "sf_get_reset_ms": [_VP, C.POINTER(C.c_float)],
    "sf_apply_mitigation": [_VP, _VP, _I32],
    "sf_apply_mitigation_device": [_VP, _VP, _I32],
    "sf_ignite": [_VP, _VP, _I32],
    "sf_ignite_device": [_VP, _VP, _I32],
    "sf_time_ignites": [_VP, _I32],
    "sf_get_ignite_ms": [_VP, C.POINTER(C.c_float)],
    "sf_time_components": [_VP, _I32],
    "sf_get_components_ms": [_VP, C.POINTER(C.c_float)],
    "sf_load_fire_map": [_VP, _I32, _VP],
    "sf_step": [_VP, _I32],
    "sf_step_timed": [_VP, _I32, C.POINTER(C.c_float)],
    "sf_step_mitigated": [_VP, _I32, _VP, _I32, _I32, C.POINTER(C.c_float)],
    "sf_get_fire_map": [_VP, _I32, _VP],
    "sf_get_fire_maps": [_VP, _VP],
    "sf_get_fire_map_delta": [_VP, _I32, _VP, _I32, C.POINTER(_I32)],
    "sf_run_delta": [_VP, _I32, _I32, _VP, _VP, _VP, _I32, C.POINTER(_I32)],
    "sf_get_burn": [_VP, _I32, _VP],
    "sf_set_burn": [_VP, _I32, _VP],
    "sf_copy_envs": [_VP, _VP, _VP, _I32, _I32],
    "sf_state_bytes": [_VP, C.POINTER(_I64)],
    "sf_save_state": [_VP, _I32, _VP, _VP, _I32],
    "sf_load_state": [_VP, _I32, _VP, _VP, _I32],
    "sf_get_status": [_VP, _VP, _VP],
    "sf_fire_map_device": [_VP, C.POINTER(_VP), C.POINTER(_I64), C.POINTER(_I64)],
    "sf_observe": [_VP, C.POINTER(SfObsParams), _I32, _VP, _VP],
    "sf_distance": [_VP, C.POINTER(SfDistParams), _I32, _VP, _VP],
    "sf_reach": [_VP, C.POINTER(SfReachParams), _I32, _VP, C.POINTER(SfReachOut)],
    "sf_walk": [_VP, C.POINTER(SfWalkParams), _I32, _VP, C.POINTER(SfWalkOut)],
    "sf_escape": [_VP, C.POINTER(SfEscapeParams), _I32, _VP, C.POINTER(SfEscapeOut)],
    "sf_travel": [_VP, C.POINTER(SfTravelParams), _I32, _VP, C.POINTER(SfTravelOut)],
    "sf_behavior": [_VP, C.POINTER(SfBehaviorParams), C.POINTER(SfBehaviorOut), _VP, _I32],
    "sf_get_behavior_builds": [_VP, C.POINTER(_I64)],
    "sf_perimeter": [_VP, C.POINTER(SfPerimeterParams), _I32, _VP, C.POINTER(SfPerimeterOut)],
    "sf_influence": [_VP, C.POINTER(SfInfluenceParams), _I32, _VP, C.POINTER(SfInfluenceOut)],
    "sf_components": [_VP, C.POINTER(SfComponentsParams), _I32, _VP, C.POINTER(SfComponentsOut)],
    "sf_cell_layout": [_VP, C.POINTER(_I32)],
    "sf_render": [_VP, C.POINTER(SfRenderParams), _I32, _VP, _VP],
    "sf_status_device": [_VP, C.POINTER(_VP)],
    "sf_update_status_device": [_VP],
    "sf_copy_status_to": [_VP, _VP],
    "sf_rollout": [_VP, _I32, _VP],
    "sf_set_result_sink": [_VP, _VP],
    "sf_comm_unique_id": [_VP],
    "sf_comm_init": [_VP, _I32, _I32, _VP],
    "sf_allgather_status": [_VP, _VP],
    "sf_comm_destroy": [_VP],
    "sf_get_counters": [_VP, _VP, _I32],
    "sf_enable_counters": [_VP, _I32],
    "sf_compute_ros": [_I64] + [_VP] * 18 + [_I32],
    "sf_memory_bytes": [_VP, C.POINTER(_I64)],
    "sf_get_geometry": [_VP, _VP],
    "sf_set_rows_per_band": [_VP, _I32],
    "sf_set_dense": [_VP, _I32],
    "sf_enable_spread_graph": [_VP, _I32],
    "sf_get_spread_parents": [_VP, _I32, _VP],
    "sf_set_generic": [_VP, _I32],
    "sf_set_fused": [_VP, _I32],
    "sf_set_tuning": [_VP, _I32, _I32],
    "sf_get_tuning": [_VP, _I32, C.POINTER(_I32)],
    "sf_get_run_cost": [_VP, _VP],
    "sf_loop_start": [_VP, _I32],
    "sf_loop_step": [_VP, _VP, _VP, _VP],
    "sf_loop_stop": [_VP],
    "sf_loop_restarts": [_VP, C.POINTER(_I32)],
    "sf_get_team_sizes": [_VP, _VP],
    "sf_get_join_log": [_VP, _VP, C.c_int32, _VP],
    "sf_get_last_launches": [_VP, _VP],
    "sf_get_team_fallbacks": [_VP, _VP],
    "sf_last_step_launch": [_VP, C.POINTER(_I32)],
    "sf_set_prune_after_quit": [_VP, _I32],
    "sf_set_async": [_VP, _I32],
    "sf_sync": [_VP],
    "sf_set_threshold": [_VP, C.c_double],
    "sf_cfd_create": [C.POINTER(SfCfdParams), C.POINTER(_VP)],
    "sf_cfd_destroy": [_VP],
    "sf_cfd_set_terrain": [_VP, _I32, _VP],
    "sf_cfd_step": [_VP, _I32, _I32],
    "sf_cfd_step_timed": [_VP, _I32, _I32, C.POINTER(C.c_float)],
    "sf_cfd_get_velocity": [_VP, _I32, _VP, _VP],
}
STRING_GETTERS = ("sf_last_error", "sf_version")

# Other builds of the same sources, loaded only by tests (python -m simfire_amd.build --all):
#   "sow"  -DSF_STORE_ORDER_WAIT: k_run with an explicit wait between a vector's 16-byte store and its ignition byte stores
VARIANTS = {"sow": "libsimfire_hip_sow.so"}


def variant_path(variant):
    return os.environ.get("SIMFIRE_HIP_LIB_" + variant.upper()) or os.path.join(_HERE, "csrc", VARIANTS[variant])


TUNE = {name: i for i, name in enumerate((
    "waves_per_cu", "run_waves", "run_min_envs", "run_vcap", "run_compact", "run_batch", "run_result", "run_segment",
    "run_team", "team_placement", "team_recut", "run_window", "team_timeout_ms", "run_join", "loop_light"))}

_libs = {}


def load(variant=None):
    """Load the HIP library (once).  Raises ``SimfireHipError`` if it has not been built."""
    path = variant_path(variant) if variant else LIB_PATH
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise SimfireHipError(
            f"{path} is missing: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()' or python -m simfire_amd.build"
            f"{' --all' if variant else ''}). simfire_amd has no CPU fallback.")
    lib = C.CDLL(path)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = C.c_int
    for name in STRING_GETTERS:
        getattr(lib, name).restype = C.c_char_p
        getattr(lib, name).argtypes = []
    _libs[path] = lib
    return lib


def check(rc, lib=None):
    """Map a C return code onto the exception type the reference raises for that failure."""
    if rc == SF_OK:
        return
    msg = (lib or load()).sf_last_error().decode("utf-8", "replace")
    if rc in (SF_EINVAL, SF_ESHAPE):
        raise ValueError(msg)
    if rc == SF_ENOTSUP:
        raise NotImplementedError(msg)
    raise SimfireHipError(msg)
