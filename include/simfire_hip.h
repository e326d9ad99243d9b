/*
 * simfire_hip.h - C ABI of the MI355X (gfx950) Rothermel fire-spread stepper.
 *
 * This library is a drop-in for ONE path of mitrefireline/simfire (v2.0.1):
 *
 *   RothermelFireManager.__init__ / update      simfire/game/managers/fire.py:293-380, 616-719
 *   compute_rate_of_spread                      simfire/world/rothermel.py:4-136
 *   ControlLineManager.update (line scatter)    simfire/game/managers/mitigation.py:60-80
 *   FireSimulation.update_mitigation            simfire/sim/simulation.py:449-478
 *   FireSimulation.load_mitigation              simfire/sim/simulation.py:425-447
 *
 * batched over a leading environment axis (n_envs independent simulations that share the
 * terrain / wind layers).  Plain C types only: host pointers in, host pointers out, an
 * opaque handle in between.  Every function returns 0 (SF_OK) or a negative code;
 * sf_last_error() gives the message for the calling thread.  No exception crosses the ABI.
 *
 * Ownership: the library owns all device memory.  Host arrays are caller-owned, read or
 * written during the call only; nothing but the handle outlives a call.
 * Threading: calls on one handle are not re-entrant; different handles may be driven from
 * different threads.  One HIP stream per handle; every call returns after its work is done
 * unless stated otherwise.
 *
 * Grid convention (same as the reference): arrays are [H][W] row-major, "x" is the column,
 * "y" the row, positions are given as (x, y) like fire_initial_position
 * (simulation.py:565-566) and mitigation points (column, row, type) (simulation.py:462).
 */
#ifndef SIMFIRE_HIP_H
#define SIMFIRE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SF_OK 0
#define SF_EINVAL (-1)   /* bad argument value                         -> ValueError      */
#define SF_ESHAPE (-2)   /* array shape mismatch (fire.py:406-428)     -> ValueError      */
#define SF_EHIP (-3)     /* HIP runtime error                          -> RuntimeError    */
#define SF_ENOTSUP (-4)  /* outside the supported envelope             -> NotImplementedError */
#define SF_ESTATE (-5)   /* call sequence error (e.g. step before layers) -> RuntimeError */
#define SF_ERCCL (-6)    /* RCCL error (library missing, communicator, collective) -> RuntimeError */

/* BurnStatus (simfire/enums.py:52-69) - the values stored in fire_map */
#define SF_UNBURNED 0
#define SF_BURNING 1
#define SF_BURNED 2
#define SF_FIRELINE 3
#define SF_SCRATCHLINE 4
#define SF_WETLINE 5

/* Index k of the 8 travel directions of the R table: source cell = destination + SF_SRC_DX/DY[k].
 * The order is the reference's tie-break priority (last sprite in list order wins the scatter at
 * fire.py:705; the sprite list is sorted by ignition step, then y, then x, fire.py:566-579). */
#define SF_NDIR 8
static const int SF_SRC_DX[SF_NDIR] = {+1, 0, -1, +1, -1, +1, 0, -1};
static const int SF_SRC_DY[SF_NDIR] = {+1, +1, +1, 0, 0, -1, -1, -1};

/* Constructor arguments of RothermelFireManager (fire.py:293-307) + FuelParticle
 * (world/parameters.py:7-27) + Environment.M_f (parameters.py:52-76) + batch size. */
typedef struct sf_params {
    int32_t n_envs;             /* independent simulations batched on this GPU (>= 1)          */
    int32_t height, width;      /* terrain.screen_size = (H, W)                                */
    int32_t max_fire_duration;  /* fire.py:60; 1..28 (1..5: tiled SWAR kernels; above: generic kernel) */
    int32_t diagonal_spread;    /* fire.py:306   0 = 4-connected, 1 = 8-connected              */
    int32_t attenuate_line_ros; /* fire.py:304                                                 */
    int32_t has_max_time;       /* 0 <=> max_time is None (fire.py:303)                        */
    int32_t device;             /* HIP device ordinal                                          */
    double pixel_scale;         /* fire.py:298 (ft per pixel)                                  */
    double update_rate;         /* fire.py:299 (minutes per step)                              */
    double max_time;            /* fire.py:303 (minutes)                                       */
    double h, S_T, S_e, p_p;    /* FuelParticle; rounded to float32 like fire.py:537,546        */
    double M_f;                 /* Environment.M_f                                              */
    int32_t per_env_terrain;    /* 0 = all environments share terrain and wind (one R table);    */
                                /* 1 = every environment has its own layers (sf_set_layers_env)  */
} sf_params;

typedef struct sf_sim sf_sim; /* opaque */

/* (Launch-geometry knobs, launch-structure forcing, statistics counters, timing and cost introspection - what bench.py, the
 * tests and the scripts under profiles/ use and a SimFire maintainer never binds - are declared in simfire_hip_lab.h; same library.) */
const char *sf_last_error(void);
const char *sf_version(void);

/* replaces RothermelFireManager.__init__ (fire.py:293-380) - allocation only */
int sf_create(const sf_params *params, sf_sim **out);
int sf_destroy(sf_sim *sim);

/* Layers read once at construction (fire.py:354-380): fuel of every cell (terrain.fuels ->
 * Fuel.w_0/delta/M_x/sigma, parameters.py:30-49), terrain.elevations, Environment.U / U_dir
 * already broadcast to [H][W] (fire.py:382-434).  All arrays float64 [H*W]; the library rounds
 * to float32 where the reference does.  Computes the slopes (fire.py:436-449, np.gradient) and
 * the R table R8[k][y][x] on the device. */
int sf_set_layers(sf_sim *sim, const double *w_0, const double *delta, const double *M_x,
                  const double *sigma, const double *elevation, const double *U,
                  const double *U_dir);

/* Logic-parity mode: supply / read back the rate-of-spread table R8[SF_NDIR][H][W] (ft/min,
 * not yet multiplied by update_rate). */
int sf_set_rtable(sf_sim *sim, const double *R8);
int sf_get_rtable(sf_sim *sim, double *R8_out);
int sf_get_slopes(sf_sim *sim, double *slope_mag_out, double *slope_dir_out);
/* Per-environment terrain (handles created with per_env_terrain = 1): independent FireSimulation
 * instances with different fuel / topography / wind in one batch.  sf_set_layers / sf_set_rtable
 * then address every environment at once; sf_get_rtable returns environment 0. */
int sf_set_layers_env(sf_sim *sim, int32_t env, const double *w_0, const double *delta, const double *M_x,
                      const double *sigma, const double *elevation, const double *U, const double *U_dir);
int sf_set_rtable_env(sf_sim *sim, int32_t env, const double *R8);
int sf_get_rtable_env(sf_sim *sim, int32_t env, double *R8_out);

/* Layers from an FBFM13 fuel-model raster, expanded on the device: FuelLayer._get_data
 * (simfire/utils/layers.py:670-676) with the caller's FuelModelToFuel table (simfire/enums.py:176-198):
 * lut_codes int32 [n_lut], lut_fuel float64 [n_lut][4] = (w_0, delta, M_x, sigma).  codes int32 [H*W];
 * env = -1 addresses every environment.  A code missing from the table is SF_EINVAL (KeyError there). */
int sf_set_layers_fbfm(sf_sim *sim, int32_t env, const int32_t *codes, int32_t n_lut, const int32_t *lut_codes,
                       const double *lut_fuel, const double *elevation, const double *U, const double *U_dir);
/* FireSimulation.get_attribute_data (simfire/sim/simulation.py:376-403) from the layers held in HBM:
 * w_0, delta, M_x as float32, sigma as uint32, elevation / wind as supplied (float64), each [H*W];
 * null pointers are skipped.  device_pointers != 0: the outputs are device buffers. */
int sf_get_attribute_data(sf_sim *sim, int32_t env, float *w_0, uint32_t *sigma, float *delta, float *M_x,
                          double *elevation, double *wind_speed, double *wind_direction, int32_t device_pointers);

/* Seeded worlds drawn on the device: what FireSimulation.set_seeds + reset rebuild
 * (simfire/sim/simulation.py:713-759, 202-214) for a list of environments of a per_env_terrain handle, in a bounded
 * number of launches and one wait - nothing but the descriptors crosses PCIe.  The generators are pure functions of
 * (seed, cell), evaluated in float64 in the order of the host oracles in simfire_amd/workloads.py:
 *   elevation  SF_GEN_SIMPLEX: perlin topography, elevation_functions.py:75-122 (workloads.perlin_elevation: the
 *              fractal value rounded to float32, then ((z + 1) / 2) * (hi - lo) + lo in float64); SF_GEN_CONSTANT: lo
 *              everywhere (flat, elevation_functions.py:9-30)
 *   fuel       SF_GEN_CONSTANT: w_0, delta, M_x, sigma everywhere - chaparral(seed), terrain.py:29-114, whose four
 *              legacy-MT19937 draws the host makes (config.chaparral_fuel)
 *   wind_speed / wind_direction  SF_GEN_SIMPLEX: perlin wind, perlin_wind.py:69-98 with config.py:892-944's float32
 *              map (workloads.simplex_field, widened to float64; speed in ft/min); SF_GEN_CONSTANT: lo everywhere
 * The simplex generator is this build's own, not the `noise` wheel's: same parameters, other values.  Seeds s and
 * s + 256 give the same field.  SF_GEN_NONE leaves a plane as it is.  Then the slopes and R tables of exactly these
 * environments are rebuilt, bit-identical to what sf_set_layers_env builds from the same planes (sf_get_slopes keeps
 * reporting the last sf_set_layers* call).  Every descriptor is checked before any device work: a shared-terrain
 * handle is SF_ESTATE; environments out of range or repeated, scale <= 0, octaves outside 1..16, lo >= hi (simplex)
 * or an unknown kind are SF_EINVAL.  Ends a running closed loop first.  n == 0 does nothing. */
#define SF_GEN_NONE 0
#define SF_GEN_CONSTANT 1
#define SF_GEN_SIMPLEX 2
typedef struct sf_noise {
    int32_t kind;                 /* SF_GEN_*                                                                     */
    int32_t octaves;              /* simplex: 1..16                                                               */
    int64_t seed;                 /* simplex: offsets the permutation indices ((i + seed) & 255, 64-bit)          */
    double scale;                 /* simplex: cells per noise unit (> 0; perlin topography: 1)                    */
    double persistence, lacunarity;
    double lo, hi;                /* simplex: range_min < range_max; constant: the value is lo                    */
} sf_noise;
typedef struct sf_layer_gen {
    sf_noise elevation;
    int32_t fuel;                 /* SF_GEN_NONE or SF_GEN_CONSTANT                                               */
    int32_t reserved;             /* 0                                                                            */
    double fuel_values[4];        /* w_0, delta, M_x, sigma                                                       */
    sf_noise wind_speed, wind_direction;
} sf_layer_gen;
int sf_generate_layers(sf_sim *sim, int32_t n, const int32_t *envs, const sf_layer_gen *gen);

/* A wind change during an episode.  RothermelFireManager reads self.U / self.U_dir at every update()
 * (simfire/game/managers/fire.py:365, 490-494): a caller who assigns new arrays between two update() calls gets a wind shift.
 * sf_set_wind is that assignment for the tables of a list of environments: every later update uses the table sf_set_layers_env
 * would build from the unchanged fuel and elevation planes and the new U (ft/min), U_dir (degrees) - bit for bit -; cells, ages,
 * burn_amounts (the lazy line attenuation included), elapsed_time, result rows, history, arrival plane and spread graph stay
 * as they are.  Layer planes 5 and 6 take the new wind (sf_get_attribute_data, sf_observe).  envs == NULL addresses every
 * table in order: n == 1 on a shared-terrain handle, n == n_envs otherwise; a list on a shared-terrain handle is SF_ESTATE.
 * Environments out of range or repeated, null pointers, unknown flag bits: SF_EINVAL before any device work; a listed table that
 * has no layers (only sf_set_rtable): SF_ESTATE; n == 0 does nothing.  Ends a running closed loop first.  Under sf_set_async the
 * call only enqueues (a host U / U_dir is consumed before it returns; device memory must stay as it is until the handle's stream
 * has passed the call); otherwise it waits once at its end.  Clears the schedule of a listed environment. */
#define SF_WIND_UNIFORM 0   /* U, U_dir: float64 [n] */
#define SF_WIND_FIELD   1   /* U, U_dir: float64 [n][H*W] */
#define SF_WIND_DEVICE  2   /* or-ed in: the two pointers are device memory */
int sf_set_wind(sf_sim *sim, int32_t n, const int32_t *envs, const double *U, const double *U_dir, int32_t flags);

/* A wind that depends on the episode's time, decided on the device (fire.py:365, 490-494 with the assignment made by a timetable;
 * an environment restarted inside sf_agents_step has an update count the host does not know).  Environment envs[i] gets K
 * segments segs[i][0 .. K): from update first_update on (0-based count of update() calls since the environment's reset) its
 * uniform wind is (U, U_dir).  segs[.][0].first_update == 0, strictly increasing, 1 <= K <= SF_WIND_MAX_SEGS, reserved == 0, else
 * SF_EINVAL; K == 0 clears.  Needs a per_env_terrain handle (SF_ESTATE) whose listed tables have layers (SF_ESTATE).  envs == NULL:
 * every environment in order (n == n_envs).
 * THE CALL-BOUNDARY RULE: the wind changes where a stepping call begins, not inside it.  In front of the updates of every stepping
 * call (sf_step, sf_step_mitigated, sf_rollout, sf_run_delta, each of the stepping pieces of sf_agents_step) the segment of every
 * scheduled environment's update count is compared with the one its table stands for, on the device, and the tables that are due
 * are rebuilt; the call then runs entirely under those tables.  A restart inside sf_agents_step is picked up by the next call.
 * sf_loop_start with a schedule set is SF_ENOTSUP.  sf_copy_envs with SF_COPY_TERRAIN copies the schedule with the table, without
 * it leaves it alone; sf_load_state makes the loaded environments' segment unknown (their next stepping call rebuilds the table). */
#define SF_WIND_MAX_SEGS 16
typedef struct sf_wind_seg { int32_t first_update, reserved; double U, U_dir; } sf_wind_seg;
int sf_set_wind_schedule(sf_sim *sim, int32_t n, const int32_t *envs, int32_t K, const sf_wind_seg *segs /* [n][K] host */);

/* History of FireSimulation._save_data (simulation.py:548-549, 887-959): the fire map after every
 * executed update, a ring int8 [n_envs][capacity][H][W] in HBM: update number u (0-based, counted from
 * the last reset of that environment = elapsed_steps before it) lands in slot u mod capacity.
 * sf_get_history copies updates first .. first+count-1 (count <= capacity; the caller fetches before
 * the ring wraps over them).  capacity 0 frees it. */
int sf_enable_history(sf_sim *sim, int32_t capacity);
int sf_get_history(sf_sim *sim, int32_t env, int32_t first, int32_t count, int8_t *out);
int sf_history_device(sf_sim *sim, void **ptr, int32_t *capacity);

/* Arrival times: for every cell the update() call that created its FIRST sprite - the sprite creation of
 * _update_with_new_locs (fire.py:571-587), which the reference forgets once the sprite is pruned and its users rebuild from
 * fire_map.npy after the run.  Numbered as sf_get_history numbers updates: the reset's ignition cell is 0, a cell ignited by the
 * first update() call is 1.  The value is an update INDEX, not minutes: elapsed_time does not advance on an update without a
 * candidate (fire.py:651-652), so a conversion is the caller's business (sf_get_status per update, or update_rate where every
 * update ran to the end).  The definition counts SPRITES: a cell that sf_load_fire_map paints BURNING has no sprite and no arrival; a
 * control line drawn over a burned cell does not erase its arrival; a cell that ignites again (a line drawn on a burning cell makes
 * it eligible, fire.py:192-205) keeps its first.  A new episode (every form of reset) clears the environment's plane.
 * The plane is kept by a pass BEHIND the step launches, not by them: while recording is on, a call of n updates runs as pieces of at
 * most max_fire_duration updates, each followed by the pass - the launch structure of every piece is chosen as for a call of that
 * length, results do not change, a long call pays one launch boundary per piece.  Recording off costs nothing.
 * sf_enable_arrival: allowed at any time; ends a running closed loop first.  on != 0 allocates and zeroes the plane (uint32 per cell
 * and environment; counted by sf_memory_bytes): cells that burned out before that moment stay "never", sprites that are live at that
 * moment are picked up with their true update by the first pass (made here if the handle has been reset).  on == 0 frees it.
 * While it is on: sf_loop_start is SF_ENOTSUP (a closed loop has no launch boundary to hang the pass on); sf_copy_envs carries the
 * plane; a state blob carries it, and blobs of a handle with recording and one without do not match (SF_EINVAL).
 * sf_get_arrival: int32 [H*W] of one environment - the update that ignited the cell, 0 = the reset's ignition, -1 = never.
 * SF_ESTATE before sf_enable_arrival.
 * sf_arrival_device: the raw plane for zero-copy consumers - uint32, update + 1, 0 = never; pointer to environment 0, row pitch and
 * environment stride in bytes.  Complete once the handle's stream has reached the end of the last stepping (or reset) call. */
int sf_enable_arrival(sf_sim *sim, int32_t on);
int sf_get_arrival(sf_sim *sim, int32_t env, int32_t *out /* [H*W] */);
int sf_arrival_device(sf_sim *sim, void **ptr, int64_t *row_pitch, int64_t *env_stride);

/* Values at risk.  The reference keeps no asset values; the entries stand for what a harness of the reference
 * computes after a run from fire_map.npy (simulation.py:548-549) and a value raster of its own: the worth of every cell that ever
 * showed BURNING, i.e. whose first sprite was created (fire.py:571-587), and per agent step the part of it that was new.  While a value
 * plane is set the handle keeps, for every environment,
 *     damage[e] == the sum of value[e][y][x] over the cells whose arrival is not "never" (sf_get_arrival(e) >= 0), in integers,
 * complete wherever the arrival plane is complete: behind every stepping call, every form of reset, sf_copy_envs and sf_load_state.
 * What follows: a cell counts once per episode, when its first sprite is created - the reset's ignition cell included; a cell
 * that sf_load_fire_map paints BURNING has no sprite and does not count; a control line drawn later gives nothing back; a line
 * drawn on a burning cell does not count it twice; cells that burned out before sf_enable_arrival do not count.  A new episode
 * (every form of reset) starts from value[ignition].  The sum is kept by a pass behind the arrival pass, O(fire front), not by the
 * step kernels; with no plane set every call enqueues what it enqueues without the feature.
 * sf_values_set: int32 [H*W] for every environment (per_env == 0) or [n_envs][H*W] (per_env != 0), host memory or device memory on
 * this GPU (device_pointer != 0); the handle keeps a copy of its own (counted by sf_memory_bytes), the caller's memory is free when
 * the call returns.  |value| <= 2^24, else SF_EINVAL and the handle is as it was: host input is checked before any device work,
 * device input by a kernel whose verdict the call waits for.  Needs sf_enable_arrival (SF_ESTATE), and while a plane is set
 * sf_enable_arrival(sim, 0) is SF_ESTATE.  Allowed at any time; ends a running closed loop first (sf_loop_start stays SF_ENOTSUP
 * as under sf_enable_arrival); damage is recounted from the arrival plane as it stands, under the new plane.  values == NULL switches
 * the feature off and frees its buffers (and the fifth reward weight with them).
 * sf_values_get: damage of every environment, complete on return.  SF_ESTATE without a plane.
 * sf_values_device: for zero-copy consumers - damage (int64 per environment, stride in bytes between environments) and the loss of the
 * last sf_agents_step tick (int64 [n_envs], contiguous): damage after the tick's updates minus damage before them, 0 for an
 * environment that was not running before the tick; after an auto-reset tick it still reports the finished episode's last tick
 * while damage is already the new episode's.  Complete once the handle's stream has reached the end of the last call.
 * sf_values_set_weight (an entry of this family, not of sf_agents_*: it is refused without a plane): on != 0 adds a fifth product to the reward of sf_agents_step, evaluated like the four (in double, left
 * to right, rounded to float once): ... + w_value * (double)tick_loss[e]; on == 0 leaves the reward exactly what it is without the
 * feature.  sf_agent_params.w and sf_agent_out.terms stay four wide.  SF_ESTATE without agents or without a value plane;
 * sf_agents_create and sf_values_set(NULL) switch the weight off.  State blobs do not carry damage (a restore recounts it), a
 * fork carries it but not the tick's base. */
int sf_values_set(sf_sim *sim, const int32_t *values, int32_t per_env, int32_t device_pointer);
int sf_values_get(sf_sim *sim, int64_t *damage_out /* [n_envs] host */);
int sf_values_device(sf_sim *sim, void **damage, int64_t *damage_stride, void **tick_loss);
int sf_values_set_weight(sf_sim *sim, float w_value, int32_t on);

/* Ensemble statistics: per-cell statistics ACROSS environments.  The reference keeps no ensemble; the entries
 * stand for what a harness of the reference computes after many runs from their fire_map.npy files (simulation.py:548-549): the
 * burn-probability map, the earliest and the mean arrival, the expected loss by horizon.  A group is a list of K environments of
 * this handle (forked, under different winds or control lines: the members of an ensemble); an environment may stand in several
 * groups and more than once in one - it counts as often as it is listed.  With a1 the raw arrival word of a cell (update + 1,
 * 0 = never; sf_arrival_device), a member has REACHED the cell by horizon h iff a1 != 0 && (h < 0 || a1 <= h + 1).  Horizons are
 * update indices as sf_get_arrival numbers them, strictly ascending, the last may be -1: no limit.  Per group g and horizon t:
 *   count [G][T][H][W] int32    members that reached the cell by horizons[t]
 *   prob  [G][T][H][W] float32  (float)count / (float)K, correctly rounded
 *   first [G][H][W]    int32    the smallest update index over the members that reached the cell by the LAST horizon, -1 if none
 *   mean  [G][H][W]    float32  over the same n members: (float)((double)sum / (double)n), sum their update indices (uint64); -1 if none
 *   loss  [G][T]       int64    the sum over the members as listed of the values (sf_values_set; the member's own plane under
 *                               per_env) of the cells that member reached by horizons[t]
 * All device memory, contiguous, aligned to their element; any may be NULL, not all.  The arrival plane is taken as it stands: a member
 * that has made fewer updates than a horizon contributes what it has recorded, a frozen member is frozen, a member whose recording was
 * enabled late carries the limits of sf_enable_arrival.  One launch reads every listed member's plane once, for all horizons and
 * outputs; no state of the handle changes (no plane is converted, the reference point of sf_get_fire_map_delta and the result block
 * stay).  Everything is checked before any device work: a NULL argument, no output, G < 1, K outside 1..65535, G * K > 2^20, T outside
 * 1..SF_ENS_MAX_HORIZONS, horizons not strictly ascending or below -1 or a -1 that is not last, reserved != 0, a member outside
 * 0..n_envs-1, a misaligned output: SF_EINVAL; before sf_enable_arrival, or loss without a value plane: SF_ESTATE.  In async mode the
 * call only enqueues: the outputs are complete once the handle's stream has passed it (sf_sync). */
#define SF_ENS_MAX_HORIZONS 8
typedef struct sf_ensemble_params {
    int32_t n_groups, group_size;               /* G, K */
    int32_t n_horizons;                         /* T */
    int32_t horizons[SF_ENS_MAX_HORIZONS];
    int32_t reserved;                           /* 0 */
} sf_ensemble_params;
typedef struct sf_ensemble_out {                /* device memory, any may be NULL, not all */
    int32_t *count; float *prob; int32_t *first; float *mean; int64_t *loss;
} sf_ensemble_out;
int sf_ensemble_stats(sf_sim *sim, const sf_ensemble_params *params,
                      const int32_t *members /* [G][K] host */, const sf_ensemble_out *out);

/* FireSimulation.reset for every environment (simulation.py:202-214, 555-566): fire_map all
 * UNBURNED except the ignition cell, burn_amounts 0, one sprite of duration 0, elapsed_time 0.
 * init_xy = int32 [n_envs][2] = (x, y). */
int sf_reset(sf_sim *sim, const int32_t *init_xy);
int sf_reset_env(sf_sim *sim, int32_t env, int32_t x, int32_t y);
/* New episodes in many environments, one call: every environment taken is left exactly as sf_reset_env leaves
 * it, the others are not touched.  Both calls end a running closed loop first, need sf_reset to have run once (SF_ESTATE) and refuse a
 * handle whose last team launch failed; in async mode (sf_set_async) they only enqueue, otherwise they wait once at their end.
 * sf_reset_envs: environments envs[0 .. n) with ignitions xy[i] = (x, y), host arrays.  An environment may repeat (its last ignition
 * wins); n == 0 does nothing; an environment out of range or an ignition off the grid is SF_EINVAL before anything is enqueued.
 * sf_reset_where: environment e is taken iff device_mask[e] != 0 (uint8 [n_envs] in device memory) - or, with a null mask, iff it
 * is not running (what its result row shows: QUIT, still pruning or not; its state on the device: nothing is read back) - and
 * ignites at xy[e] (int32 [n_envs][2], a host array, or a device array when xy_device_pointer != 0).  An environment whose ignition lies off the grid is left untouched.  The host cannot
 * know which environments were taken, so the next sf_get_fire_map_delta of every environment returns -1 once. */
int sf_reset_envs(sf_sim *sim, int32_t n, const int32_t *envs, const int32_t *xy /* [n][2] host */);
int sf_reset_where(sf_sim *sim, const uint8_t *device_mask /* [n_envs] or NULL: not running */,
                   const int32_t *xy /* [n_envs][2] */, int32_t xy_device_pointer);

/* FireSimulation.update_mitigation (simulation.py:449-478) for any number of environments:
 * pts = int32 [n][4] rows (env, x, y, type); type in {3,4,5}, other types are skipped with the
 * reference's semantics (simulation.py:469-473).  Within one call all FIRELINE writes land
 * first, then SCRATCHLINE, then WETLINE (simulation.py:476-478); each write is unconditional
 * (mitigation.py:75-78).  Out-of-range rows -> SF_EINVAL (the reference would raise IndexError). */
int sf_apply_mitigation(sf_sim *sim, const int32_t *pts, int32_t n);
/* The same scatter for a point list that already lives in GPU memory (e.g. the action tensor of a
 * policy): rows (env, column, row, type) int32; rows with an out-of-range field are skipped. */
int sf_apply_mitigation_device(sf_sim *sim, const int32_t *device_pts, int32_t n);

/* New fire during an episode: burn-out and backfire operations, spot fires, a second start.  The reference has
 * no such call; the definition follows its sprite list: fire_manager.sprites / durations are parallel lists (fire.py:102-103) that
 * every update() leaves ordered by age, oldest first, and inside one age by (y, x) ascending (np.unique, fire.py:566-587).  For every
 * row whose cell is UNBURNED a Fire sprite of duration 0 is inserted at the place that keeps this order - among the duration-0 sprites,
 * by (y, x) - and fire_map[y, x] = BURNING: the cell cannot be told from one the last update() ignited.  burn_amounts, elapsed_time and
 * the update counts are untouched; the cell is a root of the spread graph; with arrival recording on its arrival is the number of
 * update() calls its episode has made (0 right after a reset) and damage counts its value once, both complete when the call is.
 * rows = int32 [n][4] = (env, column, row, reserved = 0), the row shape of sf_apply_mitigation.  A row is skipped silently when its
 * cell is not UNBURNED (a control line, BURNING, BURNED) or its environment is not running (finished, or QUIT and still pruning); a
 * cell without fuel is lit like any other and burns out without spreading; a cell listed several times is lit once; an environment
 * whose last sprite is about to be pruned goes on with the new ones.
 * sf_ignite: host rows; an environment, column or row out of range or reserved != 0 is SF_EINVAL naming the row, before any device
 * work.  sf_ignite_device: rows in device memory, 16-byte aligned (else SF_EINVAL), e.g. a policy's tensor - nothing is read back,
 * such rows are skipped by the kernel.  Both: a null handle, n < 0 or a null list with n > 0 is SF_EINVAL; n == 0 does nothing; before
 * the first sf_reset SF_ESTATE; a running closed loop is ended first and a handle whose last team launch failed is refused; in async
 * mode (sf_set_async) they only enqueue, otherwise they wait once at their end.  Not part of sf_loop_step, sf_rollout or
 * sf_step_mitigated: between such calls only. */
int sf_ignite(sf_sim *sim, const int32_t *pts, int32_t n);
int sf_ignite_device(sf_sim *sim, const int32_t *device_pts, int32_t n);

/* FireSimulation.load_mitigation (simulation.py:425-447): fire_map of one environment is
 * replaced wholesale (uint8 [H*W], values 0..5 else SF_EINVAL); burning sprites persist. */
int sf_load_fire_map(sf_sim *sim, int32_t env, const uint8_t *fire_map);

/* n_steps calls of RothermelFireManager.update (fire.py:616-719) on every environment that
 * is still RUNNING - the loop of FireSimulation.run (simulation.py:533-544). */
int sf_step(sf_sim *sim, int32_t n_steps);

/* Outputs.  fire_map: uint8 [H*W] BurnStatus values; burn: RothermelFireManager.burn_amounts
 * float64 [H*W]. */
int sf_get_fire_map(sf_sim *sim, int32_t env, uint8_t *out);
int sf_get_fire_maps(sf_sim *sim, uint8_t *out /* [n_envs][H*W] */);
/* The reference mutates ONE host array in place - fire_map is written where a sprite is pruned, a cell ignites or a line is drawn
 * (fire.py:140, 587; mitigation.py:75-78) and handed back by FireSimulation.run (simulation.py:546-553).  A host that keeps its own copy of
 * the map gets the same effect from the cells that CHANGED since it last asked: cells_out[i] = (y * W + x) << 3 | BurnStatus for every cell
 * of environment env that differs from the REFERENCE POINT - the map as it was when this function was last called for the environment, or the
 * all-UNBURNED map of sf_reset (the ignition cell is reported); *n_out of them, in no particular order.  *n_out = -1: no reference point yet
 * (first call; sf_load_fire_map in between) or more than cap cells changed - fetch the whole map with sf_get_fire_map before anything steps.
 * Either way the current map is the reference point from now on; sf_get_fire_map(s) never moves it.  (One dense device-side compare, 2 bytes per cell; what crosses PCIe is the list: a run(1) costs the host O(changed cells).) */
int sf_get_fire_map_delta(sf_sim *sim, int32_t env, uint32_t *cells_out /* [cap] */, int32_t cap, int32_t *n_out);
/* FireSimulation.run(n) as ONE call and ONE wait (simulation.py:501-553: the loop of update() calls, then what the caller reads - fire_map,
 * elapsed_steps, elapsed_time, active): sf_step(n_steps), environment env's row of the result block (as sf_get_status) and its elapsed_time, and
 * the cells of its fire_map that changed (as sf_get_fire_map_delta; *n_out = -1: fetch the whole map) - enqueued behind each other, waited for once. */
int sf_run_delta(sf_sim *sim, int32_t n_steps, int32_t env, int32_t *status_row /* [8] */, double *elapsed_time /* [1] or NULL */,
                 uint32_t *cells_out /* [cap] */, int32_t cap, int32_t *n_out);
int sf_get_burn(sf_sim *sim, int32_t env, double *out);
int sf_set_burn(sf_sim *sim, int32_t env, const double *burn);

/* Environment state: fork, snapshot, restore.  Every call ends a running closed loop (sf_loop_start) first,
 * needs sf_reset to have run once (SF_ESTATE) and refuses a handle whose last team launch failed.
 * sf_copy_envs: environment dst[i] becomes environment src[i] in every respect - cells, sprite ages, burn_amounts, the attenuation
 * books, spread-graph parents, arrival times, update() calls made, elapsed_time, running, the result row - in ONE launch for all n pairs.  A src may
 * repeat (one to many); the dst are distinct and none of them is a src of the same call; n == 0 does nothing; anything else is
 * SF_EINVAL.  With SF_COPY_TERRAIN on a handle created with per_env_terrain, dst also takes src's layers and R table (without
 * it, and on a shared-terrain handle, dst keeps its own terrain).  In async mode (sf_set_async) the copy is only enqueued. */
#define SF_COPY_TERRAIN 1
int sf_copy_envs(sf_sim *sim, const int32_t *src, const int32_t *dst, int32_t n, int32_t flags);
/* Bytes of one environment's state blob (a versioned header, then the planes; the same whatever the handle's internal layout). */
int sf_state_bytes(sf_sim *sim, int64_t *bytes_out);
/* The state of environments envs[0 .. n) into out (n blobs of sf_state_bytes each, back to back - a multiple of 16 bytes; a host
 * pointer, or device memory when device_pointer != 0, which must then be 16-byte aligned, else SF_EINVAL).  Every byte of a blob is
 * written: two saves of the same state are equal.  A device-pointer save in async mode is only enqueued (the blobs are there when the
 * handle's stream has got there: sf_sync); the caller orders its own work on the buffer before the call. */
int sf_save_state(sf_sim *sim, int32_t n, const int32_t *envs, void *out, int32_t device_pointer);
/* The reverse: environment envs[i] takes the state of blob i.  A blob whose header does not match this handle (version, grid,
 * max_fire_duration, diagonal spread, attenuation, max_time, update_rate, pixel_scale threshold, prune_after_quit, spread graph, arrival
 * recording) is
 * SF_EINVAL and nothing is changed.  A device buffer must be 16-byte aligned (SF_EINVAL).  A device-pointer load waits for the stream
 * once to read the headers; the restore itself is only enqueued in async mode (the caller keeps the buffer until sf_sync). */
int sf_load_state(sf_sim *sim, int32_t n, const int32_t *envs, const void *in, int32_t device_pointer);

/* Per-environment result block, the quantities an RL harness turns into episode returns:
 * status[e] = { running (1 = GameStatus.RUNNING), update() calls made (elapsed_steps),
 *               count of cells in each BurnStatus 0..5 };   elapsed_time[e] minutes (may be NULL) */
int sf_get_status(sf_sim *sim, int32_t *status /* [n_envs][8] */, double *elapsed_time);

/* Device-side views for zero-copy consumers (RL observation tensors): pointer to the uint8
 * status plane of environment 0, row pitch and environment stride in bytes; the bytes are the
 * BurnStatus values 0..5.  Call it again after stepping: while the resident launch (sf_step with
 * n >= 2 on grids up to 1024 cells wide) keeps the cells in its blocked plane, the row-major plane
 * returned here is refreshed by this call (one device-side sweep, no host copy) and is a read-only
 * snapshot until the next one; the address does not change. */
int sf_fire_map_device(sf_sim *sim, void **ptr, int64_t *row_pitch, int64_t *env_stride);
/* Observation tensors for a policy: what FireSimulation.fire_map, get_attribute_data() normalised by
 * get_attribute_bounds() and agent_positions show (simfire/sim/simulation.py:317-403, 480-499), for a list of environments, written
 * by ONE launch into caller-owned device memory as a contiguous float32 or bfloat16 tensor out[n][C][oh][ow].  The status bytes are
 * read from whichever plane is current (the resident launch's blocked plane or the row-major plane); nothing is converted, and no
 * state of the handle changes (the current plane, the tile books, the reference point of sf_get_fire_map_delta, the result block). */
#define SF_OBS_MAX_CHANNELS 32
#define SF_OBS_MAX_AGENTS 256
#define SF_OBS_MAX_POOL 128
/* channel codes */
#define SF_OBS_FIRE_MAP 0          /* FireSimulation.fire_map (simulation.py:546-553): the BurnStatus value 0..5          */
#define SF_OBS_BURN_STATUS 1       /* + s (s = 0..5, enums.py:52-69): 1 where the cell's BurnStatus is s, else 0          */
#define SF_OBS_W_0 7               /* get_attribute_data()["w_0"] (simulation.py:397): float32                             */
#define SF_OBS_SIGMA 8             /* ["sigma"] (simulation.py:398): uint32                                                 */
#define SF_OBS_DELTA 9             /* ["delta"] (simulation.py:399): float32                                                */
#define SF_OBS_M_X 10              /* ["M_x"] (simulation.py:400): float32                                                  */
#define SF_OBS_ELEVATION 11        /* ["elevation"] (simulation.py:401): terrain.elevations, float64                       */
#define SF_OBS_WIND_SPEED 12       /* ["wind_speed"] (simulation.py:402): config.wind.speed as supplied, float64            */
#define SF_OBS_WIND_DIRECTION 13   /* ["wind_direction"] (simulation.py:403): float64                                       */
#define SF_OBS_AGENTS 14           /* agent_positions (simulation.py:480-499): the agent id at the cell, else 0           */
typedef struct sf_obs_params {
    int32_t n_channels;                        /* C, 1..SF_OBS_MAX_CHANNELS; a code may repeat                             */
    int32_t channels[SF_OBS_MAX_CHANNELS];     /* SF_OBS_* codes, in output order                                           */
    int32_t pool_mode[SF_OBS_MAX_CHANNELS];    /* per channel: 0 = mean (f64 sum in row-major order / f^2), 1 = max        */
    int32_t normalize;                         /* 1: attribute channels become (v - min) / (max - min) in f64 with the      */
                                               /* bounds of get_attribute_bounds() (simulation.py:334-374); no clamping     */
    int32_t pool;                              /* f, 1..SF_OBS_MAX_POOL; the (cropped) extent must be divisible by it       */
    int32_t crop_h, crop_w;                    /* 0, 0: the whole grid; else a window of crop_h x crop_w cells whose top-left */
                                               /* cell is (row - crop_h / 2, column - crop_w / 2) of the environment's center */
    int32_t dtype;                             /* 0 = float32, 1 = bfloat16 (the float32 value rounded to nearest even)      */
    int32_t centers_device;                    /* centers is a device pointer                                               */
    int32_t agents_k;                          /* entries per environment of agents, 0..SF_OBS_MAX_AGENTS                    */
    int32_t agents_device;                     /* agents is a device pointer                                                */
    double pad;                                /* final value of window cells off the grid (crop), in every channel          */
    const int32_t *centers;                    /* int32 [n][2] = (column, row) per listed environment (crop only)           */
    const int32_t *agents;                     /* int32 [n][agents_k][3] = (column, row, id) as update_agent_positions takes  */
                                               /* them (simulation.py:480-499) on a fresh map: a later entry wins a shared   */
                                               /* cell, an id moved later leaves its earlier cell; id <= 0 or off the grid =  */
                                               /* padding.  Null: the channel is 0                                            */
} sf_obs_params;
/* Environment envs[i] (a host array; repeats allowed) lands in out[i].  oh = extent_h / pool, ow = extent_w / pool.  Anything
 * invalid is SF_EINVAL before a launch; attribute channels before layers are SF_ESTATE.  In async mode the call only enqueues
 * (the tensor is complete when the handle's stream has got there); the caller orders its own work on device_out before the call. */
int sf_observe(sf_sim *sim, const sf_obs_params *params, int32_t n, const int32_t *envs, void *device_out);

/* Distance fields: how far every cell - or every one of a list of points - is from the nearest burning cell,
 * control line or unburned cell.  The reference has no counterpart; the semantics are this library's own, exact and in integers.
 * For a listed environment, the source set S is every cell (y, x), x < width, whose status byte & 7 is selected by status_mask (bit s
 * selects BurnStatus s, enums.py:52-69), read from whichever cell plane is current.
 *   d2[y][x] = min over S of (y - y')^2 + (x - x')^2 as int32; an empty S gives SF_DIST_FAR.  With max_d2 > 0 every value is
 *   min(d2, max_d2) (an empty S then gives max_d2 everywhere); max_d2 = 0: no cap.
 *   SF_DIST_I32: that value.  SF_DIST_F32: (float)(sqrt((double)value) / scale) - sqrt and divide in IEEE double, one rounding to
 *   float32 - bit for bit (np.sqrt(v.astype(np.float64)) / scale).astype(np.float32).
 *   Plane form (k = 0): out[n][height][width], dense.  Point form (1 <= k <= SF_DIST_MAX_POINTS): points is device int32 [n][k][3] =
 *   (column, row, id) - the layout of sf_agents_device, which can be passed as it is when envs is every environment in order - and
 *   the result is out[n][k]; an entry with id <= 0 or a cell off the grid gives -1 (-1.0f).
 * Ties and nearest-cell indices are not reported: distances only. */
#define SF_DIST_FAR 2147483647
#define SF_DIST_I32 0
#define SF_DIST_F32 1
#define SF_DIST_MAX_POINTS 256
typedef struct sf_dist_params {
    int32_t status_mask;           /* 1..63: bit s selects BurnStatus s                                                       */
    int32_t max_d2;                /* >= 0: the cap on the squared distance, 0 = none                                         */
    int32_t dtype;                 /* SF_DIST_I32 / SF_DIST_F32                                                                */
    int32_t k;                     /* 0: plane form; 1..SF_DIST_MAX_POINTS: points per listed environment                      */
    double scale;                  /* SF_DIST_F32: the divisor (cells per unit), finite and > 0                                */
    const int32_t *points;         /* device int32 [n][k][3], or NULL with k == 0                                              */
    int64_t scratch_bytes;         /* the most scratch the call may use; 0: the default budget of 128 MiB                      */
    int32_t reserved[2];           /* 0                                                                                        */
} sf_dist_params;
/* Environment envs[i] (a host array; any order, repeats allowed) lands in out[i].  Anything invalid is SF_EINVAL before anything is
 * enqueued (a mask outside 1..63, max_d2 < 0, an unknown dtype, k outside 0..256, k > 0 without points, a scale that is not finite
 * or <= 0, reserved != 0, an output that is not 4-byte aligned, an environment out of range, a positive scratch_bytes smaller than
 * one environment's scratch plane of height * pitch * 2 bytes); a handle without layers or reset is SF_ESTATE; a grid with
 * (height - 1)^2 + (width - 1)^2 >= SF_DIST_FAR or wider than 8192 cells is SF_ENOTSUP.  The call reads the state and writes
 * nothing but device_out and the library's scratch plane - not the current plane, the tile books, the reference point of
 * sf_get_fire_map_delta, the result block, any ring, the arrival or value planes.  The scratch plane belongs to the handle: allocated
 * at the first call, grown (never shrunk) when a later call needs more, freed by sf_destroy - a growth is a hipMalloc and waits for
 * the device; the list is worked through in chunks so that scratch never exceeds the budget, which changes no bit of the result.
 * In async mode the call only enqueues (the tensor is complete when the handle's stream has got there); the caller orders its own
 * work on points and device_out before the call. */
int sf_distance(sf_sim *sim, const sf_dist_params *params, int32_t n, const int32_t *envs /* [n] host */, void *device_out);

/* Reach of the fire: the cells the fire can still get to - the flood fill of the seed cells through the open
 * cells - its size, its worth under the value plane, its mask, and whether given points lie in it.  The reference has
 * no counterpart; the semantics are this library's own.
 * For a listed environment, s(y, x) is the status byte & 7 of cell (y, x), x < width, read from whichever cell plane is current.
 *   seed(y, x) = bit s of source_mask.  open(y, x) = bit s of through_mask and, with a passable plane, passable[y][x] != 0 (device u8,
 *   dense [height * width], one plane for all or - passable_per_env - one per environment, indexed by the environment's number).
 *   The two masks are disjoint.  The neighbourhood N is the 8-neighbourhood (connectivity 8) or the 4-neighbourhood (4);
 *   connectivity 0 takes the handle's own diagonal_spread.
 *   R is the smallest set with: c in R  iff  open(c) and some n in N(c) is a seed or is in R.
 *   The pitch padding (x >= width) is never open and never a seed.
 * The spread rule (fire.py:163-234, 550-589) ignites a cell only next to a BURNING cell, and only an UNBURNED cell or a control
 * line.  So with source_mask = BURNING, through_mask = UNBURNED | FIRELINE | SCRATCHLINE | WETLINE and connectivity 0, R holds every
 * cell that becomes BURNING in any later update, for as long as nothing but stepping changes the map: an upper bound, not a forecast.
 * With through_mask = UNBURNED the same holds as long as no control-line cell ignites (lines ignite only under attenuate_line_ros).
 * Points: device int32 [n][k][3] = (column, row, id), sf_agents_device's layout, as sf_distance takes them. */
typedef struct sf_reach_params {
    int32_t source_mask, through_mask;   /* 1..63, disjoint */
    int32_t connectivity;                /* 0 (the handle's diagonal_spread), 4, 8 */
    int32_t k;                           /* 0, or 1..SF_DIST_MAX_POINTS points per listed environment */
    int32_t max_rounds;                  /* 0: to the fixed point; > 0: stop after that many rounds */
    int32_t passable_per_env;            /* passable is [n_envs][H*W] (indexed by environment number), else [H*W] */
    const uint8_t *passable;             /* device, or NULL */
    const int32_t *points;               /* device int32 [n][k][3] = (column, row, id), sf_agents_device's layout; NULL with k == 0 */
    int64_t scratch_bytes;               /* 0: the default budget */
    int32_t reserved[2];                 /* 0 */
} sf_reach_params;
typedef struct sf_reach_out {            /* device pointers, any may be NULL, at least one not */
    int32_t *count;      /* [n]        |R| */
    int64_t *value;      /* [n]        sum of the value plane over R (sf_values_set; the environment's own plane under per_env) */
    uint8_t *mask;       /* [n][H][W]  1 in R, else 0; dense */
    int32_t *seeds;      /* [n]        number of seed cells (0: nothing burning - the reach is empty because there is no fire) */
    int32_t *point_in;   /* [n][k]     1 / 0; -1 for id <= 0 or a cell off the grid */
    int32_t *rounds;     /* [n]        rounds taken; negated when max_rounds stopped the fill before the fixed point */
} sf_reach_out;
/* Environment envs[i] (a host array; any order, repeats allowed) lands in row i of every output.  Anything invalid is SF_EINVAL before
 * anything is enqueued (overlapping masks or a mask outside 1..63, an unknown connectivity, k outside 0..256, k > 0 without points,
 * point_in without k, max_rounds < 0, reserved != 0, every output null, an output that is not aligned to its element - 4 bytes, 8 for
 * value -, an environment out of range, a positive scratch_bytes below one environment's need); value without a value plane, or a
 * handle without layers or reset, is SF_ESTATE; a grid wider than 8192 cells is SF_ENOTSUP.
 * One workgroup fills one environment in rounds until nothing changes; max_rounds > 0 stops after that many: mask, count, value and
 * point_in then describe the cells reached so far, a subset of R, and rounds is negative.
 * The call reads the state and writes nothing but its outputs and its own scratch - not the current plane, the tile books, the
 * reference point of sf_get_fire_map_delta, the result block, any ring, the arrival or value planes.  The scratch belongs to the
 * handle: per listed environment of a chunk two bit planes and a halo, 16 * ceil(height / 16) * ceil(pitch / 64) * 16 bytes + 20 per
 * band of 16 rows x 64 cells, rounded up to 256; allocated at the first call, grown (never shrunk) when a later call needs more,
 * freed by sf_destroy, counted by sf_memory_bytes - a growth is a hipMalloc and waits for the device.  The default budget is 256 MiB;
 * the list is worked through in chunks so that scratch never exceeds the budget, which changes no bit of the result.
 * In async mode the call only enqueues (the outputs are complete when the handle's stream has got there); the caller orders its own
 * work on passable, points and the outputs before the call. */
int sf_reach(sf_sim *sim, const sf_reach_params *params, int32_t n, const int32_t *envs /* [n] host */, const sf_reach_out *out);

/* Walking distance: how many moves a walker needs to step onto a target cell when it enters only walkable
 * cells - one cell per move, as the agents of sf_agents_step walk -, and which move comes first.  The reference has no counterpart;
 * the semantics are this library's own.
 * For a listed environment, s(y, x) is the status byte & 7 of cell (y, x), x < width, read from whichever cell plane is current.
 *   target(c) = bit s(c) of target_mask, or targets[c] != 0 when a targets plane is given (device u8, dense [height * width], one
 *   plane for all or - targets_per_env - one per environment, indexed by the environment's number).  target_mask may be 0 only with
 *   a targets plane.
 *   walk(c) = bit s(c) of through_mask and, with a passable plane (same forms, passable_per_env), passable[c] != 0.
 *   The masks may overlap; a cell that is both is a target.  The pitch padding (x >= width) is never a target and never walkable.
 *   The neighbourhood N is the 4-neighbourhood (connectivity 4, and 0: the agents' moves) or the 8-neighbourhood (8).
 *   d is the least solution of: d(c) = 0 on targets; d(c) = 1 + min over n in N(c) with target(n) or walk(n) of d(n) on walkable
 *   cells - the number of moves of a walker that enters only walkable cells until it steps onto a target.
 * Plane form, moves int32 [n][height][width]: d(c) on target and walkable cells, SF_WALK_FAR on walkable cells no route leaves,
 * SF_WALK_BLOCKED on cells that are neither.
 * Point form, points device int32 [n][k][3] = (column, row, id), sf_agents_device's layout: the walker may stand anywhere, also on a
 * cell that is not walkable (an agent on the line it has just drawn).  point_moves[i][j] = 0 on a target, else 1 + min d(n) over the
 * target or walkable neighbours n, SF_WALK_FAR if none has a finite d.  point_step[i][j] (connectivity 4 only) is the move code of the
 * action word of section 16 - 1: row - 1, 2: row + 1, 3: column - 1, 4: column + 1 - of the LOWEST-numbered neighbour that attains
 * the minimum; 0 on a target and 0 when no move gets there.  id <= 0 or a cell off the grid gives -1 in both.  On a walkable point
 * point_moves equals the plane value.
 * max_moves = M > 0 runs only M levels: every plane and point value that would exceed M, SF_WALK_FAR included, is reported as M (the
 * convention of sf_distance's max_d2), and point_step is 0 where the true value exceeds M.  M = 0: no cap.
 * reached [n]: the number of walkable non-target cells with a finite value within the cap.  levels [n]: the number of levels that
 * added a cell - the largest finite d, or M where the cap ended the search. */
#define SF_WALK_FAR 2147483647
#define SF_WALK_BLOCKED (-1)
typedef struct sf_walk_params {
    int32_t target_mask, through_mask;   /* 0..63 (0 only with targets) / 1..63 */
    int32_t connectivity;                /* 0 or 4 (the agents' moves), 8 */
    int32_t k;                           /* 0, or 1..SF_DIST_MAX_POINTS points per listed environment */
    int32_t max_moves;                   /* 0: no cap; > 0: that many levels */
    int32_t passable_per_env;            /* passable is [n_envs][H*W] (indexed by environment number), else [H*W] */
    int32_t targets_per_env;             /* the same for targets */
    const uint8_t *passable;             /* device, or NULL */
    const uint8_t *targets;              /* device, or NULL */
    const int32_t *points;               /* device int32 [n][k][3] = (column, row, id); NULL with k == 0 */
    int64_t scratch_bytes;               /* 0: the default budget */
    int32_t reserved[2];                 /* 0 */
} sf_walk_params;
typedef struct sf_walk_out {             /* device pointers, any may be NULL, at least one not */
    int32_t *moves;        /* [n][H][W]  dense */
    int32_t *point_moves;  /* [n][k] */
    int32_t *point_step;   /* [n][k]     connectivity 4 only */
    int32_t *reached;      /* [n] */
    int32_t *levels;       /* [n] */
} sf_walk_out;
/* Environment envs[i] (a host array; any order, repeats allowed) lands in row i of every output.  Anything invalid is SF_EINVAL before
 * anything is enqueued (target_mask outside 0..63 or through_mask outside 1..63, target_mask 0 without a targets plane, an unknown
 * connectivity, k outside 0..256, k > 0 without points or points with k == 0, point_moves or point_step without k, point_step with
 * connectivity 8, max_moves < 0, reserved != 0, every output null, an output that is not aligned to 4 bytes, an environment out of
 * range, a positive scratch_bytes below one environment's need); a handle without layers or reset is SF_ESTATE; a grid wider than
 * 8192 cells is SF_ENOTSUP.
 * One workgroup searches one environment, level by level, until a level adds nothing or max_moves levels have run.
 * The call reads the state and writes nothing but its outputs and its own scratch - not the current plane, the tile books, the
 * reference point of sf_get_fire_map_delta, the result block, any ring, the arrival or value planes.  The scratch belongs to the
 * handle: per listed environment of a chunk three bit planes and two halos, 16 * ceil(height / 16) * ceil(pitch / 64) * 24 bytes + 40
 * per band of 16 rows x 64 cells, rounded up to 256; allocated at the first call, grown (never shrunk) when a later call needs more,
 * freed by sf_destroy, counted by sf_memory_bytes - a growth is a hipMalloc and waits for the device.  The default budget is 256 MiB;
 * the list is worked through in chunks so that scratch never exceeds the budget, which changes no bit of the result.
 * In async mode the call only enqueues (the outputs are complete when the handle's stream has got there); the caller orders its own
 * work on passable, targets, points and the outputs before the call. */
int sf_walk(sf_sim *sim, const sf_walk_params *params, int32_t n, const int32_t *envs /* [n] host */, const sf_walk_out *out);

/* Fire travel time: WHEN the fire gets to a cell - the minimum time, in minutes from now, over the R table the
 * handle holds NOW (it follows sf_set_wind, and a schedule segment once a stepping call has applied it).  This is Finney's minimum
 * travel time on the automaton's own graph, a FORECAST in continuous time and NOT the automaton: the automaton accumulates burn from
 * the newest burning neighbour in whole updates and its sources burn out; here the fastest neighbour counts, time is continuous and a
 * source burns for ever.  The reference has no counterpart; the semantics are this library's own.
 * For a listed environment e, its table rt and s(c) the status byte & 7 of cell c, read from whichever cell plane is current:
 *   source(c) = bit s(c) of source_mask, or sources[c] != 0 when a sources plane is given (device u8, dense [height * width], one
 *   plane for all or - sources_per_env - one per environment, indexed by the environment's number).  source_mask may be 0 only with
 *   a sources plane.
 *   pass(c) = bit s(c) of through_mask and, with a passable plane (same forms, passable_per_env), passable[c] != 0.  The masks may
 *   overlap; a cell that is both is a source.  The pitch padding (x >= width) is neither.
 *   w_k(c) = float32(pixel_scale / rt[k][c]): the division in float64, rounded once; +inf where rt[k][c] is not > 0.  rt[k][c] is the
 *   rate at which fire enters c from its neighbour n_k = c + the k-th source offset, and a cell takes pixel_scale feet of burn.  A
 *   diagonal costs pixel_scale like the automaton's.  connectivity 8: all eight k; 4: the k whose offset has a zero component; 0: the
 *   handle's diagonal_spread.
 *   T (float32) is the greatest solution of: T(c) = 0 on sources; T(c) = min_k float32(T(n_k) + w_k(c)) on passable cells over the
 *   on-grid neighbours that are source or passable, +inf when none is.  Every sum is one float32 addition; the solution is unique
 *   (float32 addition is monotone, the weights are >= 0) - what a float32 Dijkstra settles -, so no bit depends on scheduling.
 * minutes float32 [n][height][width]: T on source and passable cells (+inf where no route arrives), SF_TRAVEL_BLOCKED on cells that
 * are neither.  pred int8 [n][height][width]: on passable non-source cells with a finite T the LOWEST k with float32(T(n_k) + w_k(c))
 * == T(c) - following it leads to a source along a fastest route -, -1 elsewhere.
 * Point form, points device int32 [n][k][3] = (column, row, id), sf_agents_device's layout, point_minutes float32 [n][k]: T(c) on a
 * source or passable cell; on any other cell (an agent on the line it has just drawn) min_k float32(T(n_k) + w_k(c)) over its source
 * or passable neighbours - when it would be reached were it passable -, +inf if there is none; -1 for id <= 0 or a cell off the grid.
 * reached int32 [n]: the passable non-source cells with a finite T; last float32 [n]: the largest such T, 0 if there is none.
 * activations int32 [n]: how many times the search loaded a tile (a measure of its work, not of the fire).
 * max_minutes = M > 0 caps the search: a candidate above M is dropped, so every value <= M stays exact, and every value that would
 * exceed M, +inf included, is reported as M (the convention of sf_distance's max_d2); pred is -1 there and reached / last do not
 * count it.  M = 0: no cap.
 * A control line is a wall unless through_mask names it; it is then crossed at the plain rate - attenuate_line_ros is not modelled. */
#define SF_TRAVEL_BLOCKED (-1.0f)
typedef struct sf_travel_params {
    int32_t source_mask, through_mask;   /* 0..63 (0 only with sources) / 1..63 */
    int32_t connectivity;                /* 0 (the handle's diagonal_spread), 4, 8 */
    int32_t k;                           /* 0, or 1..SF_DIST_MAX_POINTS points per listed environment */
    float max_minutes;                   /* 0: no cap; > 0: the cap */
    int32_t passable_per_env;            /* passable is [n_envs][H*W] (indexed by environment number), else [H*W] */
    int32_t sources_per_env;             /* the same for sources */
    const uint8_t *passable;             /* device, or NULL */
    const uint8_t *sources;              /* device, or NULL */
    const int32_t *points;               /* device int32 [n][k][3] = (column, row, id); NULL with k == 0 */
    int64_t scratch_bytes;               /* 0: the default budget */
    int32_t reserved[2];                 /* 0 */
} sf_travel_params;
typedef struct sf_travel_out {           /* device pointers, any may be NULL, at least one not */
    float *minutes;        /* [n][H][W]  dense */
    int8_t *pred;          /* [n][H][W] */
    float *point_minutes;  /* [n][k] */
    int32_t *reached;      /* [n] */
    float *last;           /* [n] */
    int32_t *activations;  /* [n] */
} sf_travel_out;
/* Environment envs[i] (a host array; any order, repeats allowed) lands in row i of every output.  Anything invalid is SF_EINVAL before
 * anything is enqueued (source_mask outside 0..63 or through_mask outside 1..63, source_mask 0 without a sources plane, an unknown
 * connectivity, k outside 0..256, k > 0 without points or points with k == 0, point_minutes without k or k without point_minutes, a
 * negative or NaN max_minutes, reserved != 0, every output null, a float32 or int32 output or points not aligned to 4 bytes, an
 * environment out of range, a positive scratch_bytes below one environment's need); a handle without an R table (sf_set_layers* or
 * sf_set_rtable* - layers are not needed) or without a reset is SF_ESTATE; a grid wider than 8192 cells or of more than 131072 tiles
 * is SF_ENOTSUP.
 * One workgroup searches one environment: tiles of 32 x 32 cells are relaxed in LDS and wake their neighbours until no tile is active.
 * The call reads the state and writes nothing but its outputs and its own scratch - not the current plane, the tile books, the
 * reference point of sf_get_fire_map_delta, the result block, any ring, the arrival or value planes.  The working array of a listed
 * environment is its row of minutes where that is asked for; else it lies in a scratch that belongs to the handle, 4 * height * width
 * bytes rounded up to 256 per listed environment of a chunk: allocated at the first such call, grown (never shrunk) when a later
 * call needs more, freed by sf_destroy, counted by sf_memory_bytes - a growth is a hipMalloc and waits for the device.  The default
 * budget is 1 GiB; the list is worked through in chunks so that scratch never exceeds the budget, which changes no bit of the result.
 * In async mode the call only enqueues (the outputs are complete when the handle's stream has got there); the caller orders its own
 * work on passable, sources, points and the outputs before the call. */
int sf_travel(sf_sim *sim, const sf_travel_params *params, int32_t n, const int32_t *envs /* [n] host */, const sf_travel_out *out);

/* Escape routes: how many more moves a walker may wait where it stands and still reach a target cell without
 * ever standing on a cell at or after the moment the fire closes it - the ESCAPE SLACK.  It joins sf_travel (when a cell closes) and
 * sf_walk (one cell per move).  The reference has no counterpart; the semantics are this library's own.
 * For a listed environment, s(c) is the status byte & 7 of cell c, read from whichever cell plane is current.
 *   target(c) and walk(c): as sf_walk's (target_mask or a targets plane; through_mask and a passable plane; a cell that is both is a
 *   target; the pitch padding is neither).  The neighbourhood is the 4-neighbourhood (connectivity 4, and 0) or the 8-neighbourhood.
 *   minutes float32 [n][height][width], row i for envs[i]: the time in minutes from now at which the fire closes a cell - the layout
 *   and conventions of sf_travel's minutes output, which can be handed over as it is; any plane of closing times will do.
 *   Deadline D(c), with T = minutes[c]: NEVER if T < 0 or not T < horizon_minutes (+inf, NaN, sf_travel's cap and SF_TRAVEL_BLOCKED);
 *   else q = ((double)T - margin_minutes) / minutes_per_move in float64 and D(c) = q > 0 ? (int)ceil(q) : 0.  A walker may stand on c
 *   at move index m (now is m = 0) exactly when m < D(c).  ceil((horizon_minutes - margin_minutes) / minutes_per_move) must not exceed
 *   SF_ESCAPE_MAX_MOVES, so every finite D is at most that.
 *   SF_ESCAPE_UNREACHED_SAFE in flags makes every walkable cell with D = NEVER a target too.
 *   A route from c is p_0 = c, p_1 ... p_L, L >= 0, consecutive cells neighbours, p_L a target, p_0 .. p_(L-1) walkable non-targets;
 *   targets are safe and have no deadline.  Started after waiting w >= 0 moves it is feasible when w + j < D(p_j) for every j < L.
 *   slack(c) = SF_ESCAPE_SAFE on targets and where w is unbounded (a route over NEVER cells only); SF_ESCAPE_LOST on a walkable cell
 *   with no feasible route even for w = 0; SF_ESCAPE_BLOCKED on cells that are neither target nor walkable; else the largest feasible
 *   w.  Equivalently the unique solution of S(c) = min(D(c) - 1, max over the target-or-walkable neighbours n of S(n) - 1), with
 *   SAFE - 1 = SAFE, NEVER - 1 = SAFE and the maximum over nothing LOST: a bottleneck shortest path, not a level count.
 * slack int32 [n][height][width]: that plane.
 * Point form, points device int32 [n][k][3] = (column, row, id), sf_agents_device's layout.  point_slack [n][k]: SAFE on a target,
 * S(c) on a walkable cell; on a blocked cell (an agent on the line it has just drawn) min(D(c) - 1, max_n S(n) - 1) with its own D(c)
 * formed from minutes[c]; -2 for id <= 0 or a cell off the grid.  point_step [n][k]: where 0 <= point_slack < SAFE and the
 * connectivity is 4, the sf_walk move code (1: row - 1, 2: row + 1, 3: column - 1, 4: column + 1) of the LOWEST-numbered neighbour
 * that attains max_n S(n); 0 on a target, when lost, when the slack is SAFE (no hurry: sf_walk routes) and with connectivity 8; -1
 * where point_slack is -2.  Following it raises S by at least 1 per move, so it never cycles.
 * Summaries int32 [n]: safe - walkable non-target cells with SAFE; escapable - with 0 <= S < SAFE; lost - with S = -1; top - the
 * largest finite D among walkable non-target cells, 0 if none. */
#define SF_ESCAPE_SAFE 2147483647
#define SF_ESCAPE_LOST (-1)
#define SF_ESCAPE_BLOCKED (-2)
#define SF_ESCAPE_MAX_MOVES 32768
#define SF_ESCAPE_UNREACHED_SAFE 1
typedef struct sf_escape_params {
    int32_t target_mask, through_mask;   /* 0..63 (0 only with targets) / 1..63 */
    int32_t connectivity;                /* 0 or 4 (the agents' moves), 8 */
    int32_t k;                           /* 0, or 1..SF_DIST_MAX_POINTS points per listed environment */
    int32_t flags;                       /* 0 or SF_ESCAPE_UNREACHED_SAFE */
    int32_t passable_per_env;            /* passable is [n_envs][H*W] (indexed by environment number), else [H*W] */
    int32_t targets_per_env;             /* the same for targets */
    const uint8_t *passable;             /* device, or NULL */
    const uint8_t *targets;              /* device, or NULL */
    const int32_t *points;               /* device int32 [n][k][3] = (column, row, id); NULL with k == 0 */
    const float *minutes;                /* device float32 [n][H][W] dense, row i for envs[i] */
    double minutes_per_move;             /* finite, > 0 */
    double margin_minutes;               /* finite, >= 0 */
    double horizon_minutes;              /* finite, > 0 */
    int64_t scratch_bytes;               /* 0: the default budget */
    int32_t reserved[2];                 /* 0 */
} sf_escape_params;
typedef struct sf_escape_out {           /* device pointers, any may be NULL, at least one not */
    int32_t *slack;        /* [n][H][W]  dense */
    int32_t *point_slack;  /* [n][k] */
    int32_t *point_step;   /* [n][k] */
    int32_t *safe;         /* [n] */
    int32_t *escapable;    /* [n] */
    int32_t *lost;         /* [n] */
    int32_t *top;          /* [n] */
} sf_escape_out;
/* Environment envs[i] (a host array; any order, repeats allowed) lands in row i of every output.  Anything invalid is SF_EINVAL before
 * anything is enqueued, in this order: target_mask outside 0..63 or through_mask outside 1..63, target_mask 0 without a targets plane,
 * an unknown connectivity or flag, k outside 0..256, k > 0 without points or points with k == 0, point_slack or point_step without k;
 * every output null; an output, points or minutes not aligned to 4 bytes; a time parameter that is not finite, minutes_per_move or
 * horizon_minutes not > 0, margin_minutes < 0; a move bound above SF_ESCAPE_MAX_MOVES; minutes null; reserved != 0; a positive
 * scratch_bytes below one environment's need; an environment out of range.  A grid wider than 8192 cells or of 2^31 cells or more is
 * SF_ENOTSUP; a handle without layers or reset is SF_ESTATE.
 * One workgroup searches one environment: the cells with a finite deadline are sorted by it, the safe set is flooded from the targets
 * over the NEVER cells, then the move indices run from the largest deadline down to 0 - a level opens the cells of its deadline and
 * grows the set by one ring.
 * The call reads the state and writes nothing but its outputs and its own scratch.  The scratch belongs to the handle: per listed
 * environment of a chunk three bit planes and two halos (as sf_walk), 4 * height * width bytes for the sorted cells and 262400 bytes
 * for the bounds of the deadlines' buckets, each rounded up to 256; allocated at the first call, grown (never shrunk) when a later
 * call needs more, freed by sf_destroy, counted by sf_memory_bytes.  The default budget is 1280 MiB (256 environments of 1024 x 1024
 * are one chunk); the list is worked through in chunks so that scratch never exceeds the budget, which changes no bit of the result.
 * In async mode the call only enqueues; the caller orders its own work on minutes, passable, targets, points and the outputs before
 * the call. */
int sf_escape(sf_sim *sim, const sf_escape_params *params, int32_t n, const int32_t *envs /* [n] host */, const sf_escape_out *out);

/* Fire behaviour per cell: heat per unit area, head rate of spread, Byram's fireline intensity and flame
 * length - the quantities of the fire characteristics chart - from the R table the handle holds NOW (it follows sf_set_wind, and a
 * schedule segment once a stepping call has applied it).  The reference computes I_R on its way to R (rothermel.py:74-92) and keeps
 * none of this; units are its own: feet, minutes, pounds, BTU.
 * For a listed environment e, its terrain table and cell c, with the handle's particle parameters:
 *   I_R(c): the float32 value of rothermel.py:92 as the R tables' chain rounds it (0 where w_0 <= 0);
 *   HPA(c) = I_R * (384 / sigma) BTU/ft2 (Anderson's residence time), in float64 from the float32 I_R and sigma, rounded once;
 *   R_head(c) = max_k rt[k][c]; head(c) = the lowest k that attains it, in the order of the table's planes (the fire travels from
 *   c + that plane's source offset into c), -1 where all eight entries are 0;
 *   I_B(c) = HPA * R_head / 60 BTU/ft/s; L(c) = 0.45 * I_B ** 0.46 ft (Byram 1959) - both in float64, rounded once, 0 where I_B == 0
 *   (and where rounding made it negative: eta_M at M_f >= M_x).
 * s(c) is the status byte & 7, read from whichever cell plane is current.
 * Planes, dense [n][height][width]: hpa, ros (R_head), intensity (I_B), flame_length (L) float32, head int8.  With status_mask != 0
 * (bit s = BurnStatus s) a cell whose status the mask does not select shows 0 (head: -1).  workable uint8: 1 where the flame_length
 * plane's value (asked for or not; 0 on a cell status_mask hides) is <= flame_limit, else 0 - the form sf_walk and sf_reach take as
 * passable.
 * Summary over the cells summary_mask selects: max_flame, max_intensity float32 [n] (0 when none is selected) and classes int32 [n][5]:
 * the selected cells with L in [0, e0) [e0, e1) [e1, e2) [e2, e3) [e3, inf), compared as float32.
 * Point form, points device int32 [n][k][3] = (column, row, id), sf_agents_device's layout: point_flame[i][j] is the largest L over the
 * cells of the 3 x 3 block around the point that are on the grid and selected by summary_mask, 0 if there are none; id <= 0 or a
 * cell off the grid gives -1. */
typedef struct sf_behavior_params {
    int32_t status_mask;                 /* 0: every cell, or 1..63 */
    int32_t summary_mask;                /* 1..63 */
    int32_t k;                           /* 0, or 1..SF_DIST_MAX_POINTS points per listed environment */
    int32_t reserved;                    /* 0 */
    float flame_limit;                   /* >= 0 (workable) */
    float edges[4];                      /* e0 < e1 < e2 < e3 (classes) */
    const int32_t *points;               /* device int32 [n][k][3]; NULL with k == 0 */
} sf_behavior_params;
typedef struct sf_behavior_out {         /* device pointers, any may be NULL, at least one not */
    float *hpa, *ros, *intensity, *flame_length;      /* [n][H][W] dense */
    int8_t *head;                        /* [n][H][W] */
    uint8_t *workable;                   /* [n][H][W] */
    float *max_flame, *max_intensity;    /* [n] */
    int32_t *classes;                    /* [n][5] */
    float *point_flame;                  /* [n][k] */
} sf_behavior_out;
/* Environment envs[i] (a host array; any order, repeats allowed) lands in row i of every output.  Anything invalid is SF_EINVAL before
 * anything is enqueued (a null argument, every output null, status_mask outside 0..63 or summary_mask outside 1..63, reserved != 0,
 * edges that do not increase or are NaN, flame_limit < 0 or NaN, k outside 0..256, k > 0 without points or points with k == 0,
 * point_flame without k or k without point_flame, a float32 or int32 output that is not aligned to 4 bytes, an environment out of
 * range); a handle without layers or reset is SF_ESTATE, and so is a listed environment whose table came from sf_set_rtable* and has
 * no layers to take I_R from.
 * HPA does not depend on the wind or the fire, so it is kept in a cache, float32 [tables][height * width]: allocated at the first call
 * (4 bytes per cell and table, counted by sf_memory_bytes, freed by sf_destroy), built by k_behavior_hpa - the only transcendentals of
 * the feature - for the listed tables that are stale: every table at first, then whatever sf_set_layers*, sf_generate_layers,
 * sf_set_rtable* or sf_copy_envs with SF_COPY_TERRAIN (the destination) has touched since; not sf_set_wind.  Then ONE launch of
 * k_behavior for the whole list.  The call reads the state and writes nothing but its outputs and its cache - not the current plane,
 * the tile books, the reference point of sf_get_fire_map_delta, the result block, any ring, the arrival or value planes.
 * In async mode the call only enqueues (the outputs are complete when the handle's stream has got there); the caller orders its own
 * work on points and the outputs before the call. */
int sf_behavior(sf_sim *sim, const sf_behavior_params *params, const sf_behavior_out *out, const int32_t *envs /* [n] host */, int32_t n);

/* Perimeters of the fire: WHERE the edge of a set S of cells runs - its length, the cells of S that lie on it,
 * and the edge itself as ordered polygons.  All integers; the reference has no counterpart, the semantics are this library's own.
 * S, for a listed environment, comes from exactly one of three sources:
 *   status_mask in 1..63: the cells whose status byte & 7, read from whichever cell plane is current, the mask selects;
 *   member: a device u8 plane, dense [height * width], one for all or - member_per_env - one per environment, indexed by the
 *   environment's number: the cells where it is not 0;
 *   at_update >= 0: the cells whose arrival is not "never" and is <= at_update (the raw plane of sf_arrival_device: uint32 update + 1,
 *   0 = never; needs sf_enable_arrival).
 * Cells off the grid are not in S.
 * Lattice: cell (x = column, y = row) is the square [x, x + 1] x [y, y + 1], y pointing down; vertices (vx, vy), 0 <= vx <= width,
 * 0 <= vy <= height.  A directed crack edge leaves its tail vertex in direction d (0: +x, 1: +y, 2: -x, 3: -y) and exists iff its
 * right cell is in S and its left cell is not; relative to the tail the (right, left) cells are d = 0: (0, 0), (0, -1); 1: (-1, 0),
 * (0, 0); 2: (-1, -1), (-1, 0); 3: (0, -1), (-1, -1).  Outer loops therefore run E, S, W, N and the shoelace sum
 * 1/2 sum (x_i * y_i+1 - x_i+1 * y_i) is positive for them and negative for holes.
 * Successor: at an edge's head, AR and AL are the right and the left cell of an edge leaving the head in direction d (the cells
 * ahead).  connectivity 4 (diagonal neighbours are separate): AR not in S: d + 1; else AL not in S: d; else d + 3.  connectivity 8
 * (diagonal neighbours are joined): AL in S: d + 3; else AR in S: d; else d + 1.  0: the handle's diagonal_spread.
 * Canonical order: an edge's id is (vy * (width + 1) + vx) * 4 + d of its tail; a loop starts at its smallest-id edge, loops are
 * listed by that id, a loop's vertices are the tails of its edges in order - with simplify only the tails where the direction
 * changes (the start vertex always is one).
 * Cheap outputs (no tracing): edges int32 [n], the perimeter in cell edges; cells int32 [n], |S|; front uint8 [n][height][width], 1
 * where a cell of S has at least one crack edge, else 0.
 * Traced outputs: loops, holes int32 [n] (holes: the loops of negative area); n_vertices int32 [n], the vertex count of the full
 * answer, also when it exceeds the capacity; vertices int32 [n][max_vertices][2] = (x, y); loop_start int32 [n][max_loops + 1], loop
 * l's vertices are [loop_start[l], loop_start[l + 1]); loop_area int32 [n][max_loops], signed, in cells; loop_edges int32
 * [n][max_loops].  The signed areas of an environment add up to |S|.
 * Overflow is decided per environment, never by a failure of the call: more than max_edges edges give -1 in loops, holes and
 * n_vertices and leave that environment's rows of the four lists untouched; n_vertices > max_vertices or loops > max_loops alone
 * leave the counts right and the four lists untouched; the entries of a list beyond the answer's are never written.  edges, cells and
 * front are always right. */
typedef struct sf_perimeter_params {
    int32_t status_mask;                 /* 1..63, or 0 with member or at_update */
    int32_t at_update;                   /* -1: off */
    int32_t connectivity;                /* 0 (the handle's diagonal_spread), 4, 8 */
    int32_t simplify;                    /* != 0: corners only */
    int32_t member_per_env;              /* member is [n_envs][H*W] (indexed by environment number), else [H*W] */
    int32_t max_edges, max_vertices, max_loops;      /* capacities per listed environment, >= 0 */
    const uint8_t *member;               /* device, or NULL */
    int64_t scratch_bytes;               /* 0: the default budget */
    int32_t reserved[2];                 /* 0 */
} sf_perimeter_params;
typedef struct sf_perimeter_out {        /* device pointers, any may be NULL, at least one not */
    int32_t *edges, *cells;              /* [n] */
    uint8_t *front;                      /* [n][H][W] dense */
    int32_t *loops, *holes, *n_vertices; /* [n] */
    int32_t *vertices;                   /* [n][max_vertices][2] */
    int32_t *loop_start;                 /* [n][max_loops + 1] */
    int32_t *loop_area, *loop_edges;     /* [n][max_loops] */
} sf_perimeter_out;
/* Environment envs[i] (a host array; any order, repeats allowed) lands in row i of every output.  Anything invalid is SF_EINVAL before
 * anything is enqueued (a null argument, a bad environment list, none or more than one of the three sources, status_mask outside
 * 0..63, at_update < -1, an unknown connectivity, a negative capacity, vertices with max_vertices == 0 or a loop list with max_loops
 * == 0, every output null, an int32 output not aligned to 4 bytes, a positive scratch_bytes below one environment's need, reserved
 * != 0, an environment out of range); a grid wider than 8192 cells, or of 2^25 or more edge words ((height + 1) * ceil((width + 1) /
 * 16)), is SF_ENOTSUP; a handle without a reset is SF_ESTATE, and so is at_update without arrival recording.
 * Without a traced output ONE streaming launch (k_perim_summary) serves the whole list and no scratch is used.  With one, one
 * workgroup traces one environment (k_perim_trace): the edges are ranked in id order, every loop is found by pointer doubling over
 * the successor permutation, positions, vertex numbers and areas come from scans - no result depends on scheduling.  Its scratch
 * belongs to the handle: per listed environment of a chunk 8 * height * ceil(width / 64) + 12 * (height + 1) * ceil((width + 1) / 16)
 * + 32 * max_edges bytes rounded up to 256 - allocated at the first such call, grown (never shrunk) when a later call needs more,
 * freed by sf_destroy, counted by sf_memory_bytes; a growth is a hipMalloc and waits for the device.  The default budget is 1 GiB; the
 * list is worked through in chunks so that scratch never exceeds the budget, which changes no bit of the result.
 * The call reads the state and writes nothing but its outputs and its own scratch - not the current plane, the tile books, the
 * reference point of sf_get_fire_map_delta, the result block, any ring, the arrival or value planes.  In async mode the call only
 * enqueues (the outputs are complete when the handle's stream has got there); the caller orders its own work on member and the
 * outputs before the call. */
int sf_perimeter(sf_sim *sim, const sf_perimeter_params *params, int32_t n, const int32_t *envs /* [n] host */, const sf_perimeter_out *out);

/* Influence of a cell on the fire: WHICH cells matter - how much of the fire passes, or passed, through each
 * cell of a forest of parent pointers, and the route from a point up to its root.  The reference has the idea as
 * FireSpreadGraph.get_descendant_heatmap (simfire/utils/graph.py:53-82), an all-pairs networkx.descendants loop; minimum-travel-time
 * tools ship it as the influence grid and the major paths.  All results are integers and no bit depends on scheduling.
 * Parent codes: a code is an index into the source offsets of the R table's planes, (dx, dy) = (+1,+1) (0,+1) (-1,+1) (+1,0) (-1,0)
 * (+1,-1) (0,-1) (-1,-1): the convention of sf_travel's pred.  For a listed environment and a cell c, par(c) is c + offset[code] when
 * 0 <= code <= 7 and that neighbour is on the grid; any other byte, or a code that points off the grid (a dense plane has no pitch
 * padding: column `width` is off the grid), is "no parent", not an error.  A cell with a parent is a FOREST cell; a cell without a
 * parent and with at least one child is a ROOT; C is the set of cells on a cycle of par (possible only with a caller's plane); D(c) is
 * the set of cells d != c whose parent chain reaches c - for c outside C it is finite and holds no cell of C.
 * pred_source says where the codes come from:
 *   SF_INFLUENCE_PRED_PLANE: pred, a device int8 plane, dense: [n][height * width] with row i belonging to envs[i] (pred_per_env != 0;
 *   what sf_travel writes) or one [height * width] for all;
 *   SF_INFLUENCE_PRED_HISTORY: the ignition tree of the episode so far; needs sf_enable_spread_graph and sf_enable_arrival.  With a(c)
 *   the value sf_get_arrival returns: a cell with a(c) < 0 has no parent; else the candidates are the neighbours n_j for which bit j is
 *   set in c's parent mask (sf_get_spread_parents, graph.py:125-134's order), n_j is on the grid, a(n_j) >= 0 and a(n_j) < a(c); the
 *   parent is the candidate of the greatest arrival (the newest, as the automaton's winner rule), ties go to the lowest code, no
 *   candidate is a root.  The strict inequality makes the result acyclic although a line drawn on a burning cell ORs later parents
 *   into its mask and cells painted by sf_load_fire_map have no arrival.
 * Weights: w1(c) = 1, or include[c] != 0 with an include plane (device u8, one [height * width] for all or - include_per_env -
 * [n_envs][height * width] indexed by environment number: the forms of sf_travel's passable).  wv(c) = w1(c) ? weight[c] : 0 where
 * weight is the handle's value plane (weight_mode SF_INFLUENCE_WEIGHT_VALUES; needs sf_values_set) or the caller's weights, device
 * int32, the same two forms (SF_INFLUENCE_WEIGHT_PLANE); with SF_INFLUENCE_WEIGHT_NONE value may not be asked for.  A cell with
 * w1 = 0 still links its children to its ancestors.
 * Plane outputs, dense [n][height][width]: cells int32 = sum of w1(d) over D(c), plus w1(c) with inclusive != 0; SF_INFLUENCE_CYCLE on
 * C.  value int64 = the same sum with wv; 0 on C.  pred int8 = the sanitised codes actually used, -1 where there is no parent - with
 * the history source the ignition tree itself.  forest, roots, cyclic int32 [n]: the three counts.
 * With inclusive = 0, a history in which every ignition had exactly one BURNING neighbour makes cells equal the reference's
 * len(nx.descendants(...)) before its uint8 cast; in general it is a lower bound: the tree keeps one parent where the graph keeps all.
 * Point form, points device int32 [n][k][3] = (column, row, id), sf_agents_device's layout, k <= SF_DIST_MAX_POINTS: point_cells int32
 * [n][k] and point_value int64 [n][k] are the plane values at the point's cell, -1 and 0 for id <= 0 or a point off the grid.
 * max_route = R > 0 (R <= 2^20) enables point_route int32 [n][k][R] and point_hops int32 [n][k]: a route holds flat cell indices
 * row * width + column - the point's cell, its parent, that cell's parent ...; the walk stops at a cell without a parent or after R
 * cells; unwritten entries are -1.  point_hops is cells written - 1 when the walk ended at a parentless cell, -2 when R cut it short
 * (a longer route, or a cycle), -1 for an invalid point. */
#define SF_INFLUENCE_PRED_PLANE 0
#define SF_INFLUENCE_PRED_HISTORY 1
#define SF_INFLUENCE_WEIGHT_NONE 0
#define SF_INFLUENCE_WEIGHT_VALUES 1
#define SF_INFLUENCE_WEIGHT_PLANE 2
#define SF_INFLUENCE_CYCLE (-2)
typedef struct sf_influence_params {
    int32_t pred_source;                 /* SF_INFLUENCE_PRED_PLANE, SF_INFLUENCE_PRED_HISTORY */
    int32_t pred_per_env;                /* pred is [n][H*W] (row i: envs[i]), else [H*W] */
    int32_t weight_mode;                 /* SF_INFLUENCE_WEIGHT_NONE, _VALUES, _PLANE */
    int32_t weights_per_env;             /* weights is [n_envs][H*W] (indexed by environment number), else [H*W] */
    int32_t include_per_env;             /* the same for include */
    int32_t inclusive;                   /* != 0: a cell counts itself */
    int32_t k;                           /* 0, or 1..SF_DIST_MAX_POINTS points per listed environment */
    int32_t max_route;                   /* 0: no routes, or 1..2^20 cells per route */
    const int8_t *pred;                  /* device; NULL with the history source */
    const int32_t *weights;              /* device; NULL unless weight_mode is SF_INFLUENCE_WEIGHT_PLANE */
    const uint8_t *include;              /* device, or NULL */
    const int32_t *points;               /* device int32 [n][k][3]; NULL with k == 0 */
    int64_t scratch_bytes;               /* 0: the default budget */
    int32_t reserved[2];                 /* 0 */
} sf_influence_params;
typedef struct sf_influence_out {        /* device pointers, any may be NULL, at least one not */
    int32_t *cells;                      /* [n][H][W] dense */
    int64_t *value;                      /* [n][H][W] */
    int8_t *pred;                        /* [n][H][W] */
    int32_t *forest, *roots, *cyclic;    /* [n] */
    int32_t *point_cells;                /* [n][k] */
    int64_t *point_value;                /* [n][k] */
    int32_t *point_route;                /* [n][k][max_route] */
    int32_t *point_hops;                 /* [n][k] */
} sf_influence_out;
/* Environment envs[i] (a host array; any order, repeats allowed) lands in row i of every output.  Anything invalid is SF_EINVAL before
 * anything is enqueued (a null argument, a bad environment list, an unknown pred_source or weight_mode, the plane source without pred
 * or the history source with one, weight_mode 2 without weights or weights without it, value or point_value without weights, k outside
 * 0..256, k > 0 without points or points with k == 0, a point output without k or k without one, max_route outside 0..2^20, max_route
 * > 0 without point_route and point_hops or either of them with max_route == 0, an int32 output, points or weights not aligned to 4
 * bytes or an int64 output not aligned to 8, a positive scratch_bytes below one environment's need, reserved != 0, every output null,
 * an environment out of range); a grid wider than 8192 cells is SF_ENOTSUP; a handle without a reset is SF_ESTATE, and so are the
 * history source while the spread graph is switched off (its masks would miss every ignition since) or without arrival recording, and
 * weight_mode 1 without a value plane.
 * Per chunk of listed environments four launches, a thread per cell: k_infl_stage derives (history) and sanitises the codes and counts
 * every cell's children; k_infl_walk starts a walker on every childless forest cell, which adds its finished sums to its parent's
 * accumulators and carries on upward only if it was the last child to arrive - agent-scope atomics only, no waiting, so the pass
 * cannot hang on any input, and on a cycle no walker ever finishes a cycle cell; k_infl_finish marks C, applies inclusive and counts;
 * k_infl_points answers the points, a lane each, with a walk of at most R cells.
 * The scratch belongs to the handle: per listed environment of a chunk, with N = height * width and every term rounded up to 256,
 * N + 4 * N bytes (codes, counters) + 4 * N where cells is not asked for + 8 * N where there are weights and value is not asked for
 * (an accumulator that is no output lives in scratch) - allocated at the first call, grown (never shrunk) when a later call needs
 * more, freed by sf_destroy, counted by sf_memory_bytes; a growth is a hipMalloc and waits for the device.  The default budget is
 * 1 GiB; the list is worked through in chunks so that scratch never exceeds the budget, which changes no bit of the result.
 * The call reads the state and writes nothing but its outputs and its own scratch - not the current plane, the tile books, the
 * reference point of sf_get_fire_map_delta, the result block, any ring, the parent masks, the arrival or value planes.  In async mode
 * the call only enqueues (the outputs are complete when the handle's stream has got there); the caller orders its own work on pred,
 * weights, include, points and the outputs before the call. */
int sf_influence(sf_sim *sim, const sf_influence_params *params, int32_t n, const int32_t *envs /* [n] host */, const sf_influence_out *out);

/* Connected components: the selected cells of an environment as separate fires or separate unburned pockets -
 * how many there are, which one a cell or a point belongs to, and what each is worth.  The reference has no counterpart; the
 * semantics are this library's own.
 * For a listed environment, s(c) is the status byte & 7 of cell c = (y, x), x < width, read from whichever cell plane is current.
 *   sel(c) = bit s(c) of select_mask and, with a member plane, member[c] != 0 (device u8, dense [height * width], one plane for all or
 *   - member_per_env - one per environment, indexed by the environment's number).  The pitch padding is never selected.
 *   The neighbourhood N is the 8-neighbourhood (connectivity 8) or the 4-neighbourhood (4); connectivity 0 takes the handle's own
 *   diagonal_spread.
 *   A component is a maximal N-connected set of selected cells.  Components are numbered 1..C by the row-major index y * width + x of
 *   their first cell, ascending (the numbering of scipy.ndimage.label), so every output is a pure function of the map: the same bits
 *   on every run and whatever the launch geometry.
 * cap = max_components.  Components beyond cap keep their numbers in labels and point_label and count in count, selected and largest;
 * they have no row in cells, value, first, bbox and touch.
 * touch: bit s (0..5) is set iff some cell of the component has an N-neighbour on the grid that is not selected and has status s; bit
 * 6 iff some cell of the component lies on the grid's border.
 * Points: device int32 [n][k][3] = (column, row, id), sf_agents_device's layout, as sf_distance takes them. */
#define SF_COMPONENTS_MAX 4096
typedef struct sf_components_params {
    int32_t select_mask;                 /* 1..63 */
    int32_t connectivity;                /* 0 (the handle's diagonal_spread), 4, 8 */
    int32_t k;                           /* 0, or 1..SF_DIST_MAX_POINTS points per listed environment */
    int32_t max_components;              /* cap: 1..SF_COMPONENTS_MAX rows of cells, value, first, bbox, touch */
    int32_t member_per_env;              /* member is [n_envs][H*W] (indexed by environment number), else [H*W] */
    int32_t reserved0;                   /* 0 (counts as reserved) */
    const uint8_t *member;               /* device, or NULL */
    const int32_t *points;               /* device int32 [n][k][3] = (column, row, id); NULL with k == 0 */
    int64_t scratch_bytes;               /* 0: the default budget */
    int32_t reserved[2];                 /* 0 */
} sf_components_params;
typedef struct sf_components_out {       /* device pointers, any may be NULL, at least one not */
    int32_t *count;        /* [n]             C, the true number, also when it exceeds cap */
    int32_t *selected;     /* [n]             number of selected cells */
    int32_t *labels;       /* [n][H][W]       dense: 0 where not selected, else the component's number (not capped) */
    int32_t *cells;        /* [n][cap]        size of component j + 1; rows j >= C are 0 */
    int64_t *value;        /* [n][cap]        the value plane (sf_values_set; the environment's own under per_env) summed over it */
    int32_t *first;        /* [n][cap]        y * width + x of its first cell; -1 for j >= C */
    int32_t *bbox;         /* [n][cap][4]     (x0, y0, x1, y1) inclusive; (-1, -1, -1, -1) for j >= C */
    int32_t *touch;        /* [n][cap]        see above; 0 for j >= C */
    int32_t *largest;      /* [n][2]          (number, cells) of the largest component over ALL C; ties to the lower number; (0, 0) if C == 0 */
    int32_t *point_label;  /* [n][k]          the label under each point; 0: not selected; -1 for id <= 0 or a cell off the grid */
} sf_components_out;
/* Environment envs[i] (a host array; any order, repeats allowed) lands in row i of every output.  Every refusal is SF_EINVAL before
 * anything is enqueued:
 *   | refused                                                              |
 *   | select_mask outside 1..63                                            |
 *   | connectivity not 0, 4 or 8                                           |
 *   | k outside 0..256                                                     |
 *   | k > 0 without points, points with k == 0                             |
 *   | max_components outside 1..4096                                       |
 *   | point_label with k == 0, k > 0 without point_label                   |
 *   | reserved != 0 (reserved0 included)                                   |
 *   | every output null                                                    |
 *   | an output or points not aligned to its element (4 bytes, 8 for value)|
 *   | a positive scratch_bytes below one environment's need                |
 *   | an environment out of range                                          |
 *   | value without a value plane (sf_values_set)                          |
 * A grid wider than 8192 cells or of 2^31 cells or more is SF_ENOTSUP; a handle without a reset is SF_ESTATE.  A running closed loop is
 * ended first, as by every query.
 * The work is a union-find over a label plane of one int32 per cell - the labels output where that is asked for, else scratch - in
 * separate launches per chunk of listed environments: stage and initialise (a cell's first parent is the first cell of its
 * horizontal run), merge (a lock-free union wherever a contact with the row above begins; agent-scope atomics only), flatten, rank
 * the roots in row-major order, relabel and gather the statistics with integer atomics.  No workgroup waits for another.
 * The call reads the state and writes nothing but its outputs and its own scratch.  The scratch belongs to the handle: per listed
 * environment of a chunk, every term rounded up to 256, 256 bytes + height * ceil(width / 64) * 8 (the selected bits) + 4 * (height +
 * 1) + 4 * height * width (ranks, then sizes) + 4 * height * width where labels is not asked for (the label plane); allocated at the
 * first call, grown (never shrunk) when a later call needs more, freed by sf_destroy, counted by sf_memory_bytes.  The default budget
 * is 3 GiB (256 environments of 1024 x 1024 are one chunk); the list is worked through in chunks so that scratch never exceeds the
 * budget, which changes no bit of the result.
 * In async mode the call only enqueues (the outputs are complete when the handle's stream has got there); the caller orders its own
 * work on member, points and the outputs before the call. */
int sf_components(sf_sim *sim, const sf_components_params *params, int32_t n, const int32_t *envs /* [n] host */, const sf_components_out *out);

/* Agents on the device: K agents per environment that walk the grid and draw control lines where they stand,
 * stepped from a policy's action tensor without a host read.  The reference records agent positions only (simulation.py:480-499) and
 * leaves the loop to the harness (the run docstring, 505-509); the semantics are this library's own.
 * Action word a = move + 5 * interact (int32): move 0 stay, 1 row - 1, 2 row + 1, 3 column - 1, 4 column + 1; interact 0 none,
 * 1 FIRELINE, 2 SCRATCHLINE, 3 WETLINE; any value outside 0..19 is (stay, none).
 * One sf_agents_step for environment e, r0 its result row (sf_get_status) before the tick:
 *   r0[0] != 1: the agents make no move and emit no point, terms = 0, done = 1, reward = 0, and steps a - d do not touch the episode
 *         statistics.  Being done, the environment still goes through e and f: final_len / final_ret report the statistics as they
 *         stand (without auto_reset the same stale values on every tick until the caller resets it and places its agents anew), and
 *         with auto_reset it is reset, its agents go back to their start cells and its statistics are cleared in this same tick.
 *   else  a. each agent moves; a move that would leave the grid does not happen and counts in terms[3]; agents may share a cell
 *         b. an agent with interact != 0 emits (column, row, type) at its NEW cell - with only_unburned only if that cell is UNBURNED
 *            before this tick's points; emitted points count in terms[1]; precedence on one cell is sf_apply_mitigation's
 *         c. update_mitigation(points of e); run(n_updates)          (sf_step_mitigated for the first update, sf_step for the rest)
 *         d. r1 the row afterwards: terms[0] = (r1[3] + r1[4]) - (r0[3] + r0[4]); terms[2] = agents whose cell is BURNING now;
 *            reward = (float)(w[0] * terms[0] + w[1] * terms[1] + w[2] * terms[2] + w[3] * terms[3]) evaluated in double, left to right;
 *            episode length += 1, episode return += (double)reward;
 *            done = r1[0] != 1 || (done_on_burn && terms[2] > 0) || (max_ticks > 0 && episode length >= max_ticks)
 *   e. outputs: reward, done, terms, and for done environments final_len / final_ret (the episode's length and return; else 0)
 *   f. with auto_reset every done environment is reset as by sf_reset_where(done, the ignitions given to sf_agents_create), its
 *      agents go back to their start cells and its episode statistics are cleared; without it nothing is reset.  While
 *      sf_episodes_set is in force (below) the new episode's ignition, wind and start cells are drawn on the device first.
 * Nothing is read back: in async mode the call only enqueues, otherwise it waits once at its end.  The agent buffers belong to
 * the handle, not to an environment's state: sf_copy_envs and sf_save_state / sf_load_state do not carry them.  With
 * sf_set_prune_after_quit an environment that QUIT on the runtime check is still pruned by the updates of step c. */
typedef struct sf_agent_params {
    int32_t k;                  /* agents per environment, 1..64 (the bound of sf_loop_start); 0 frees the agent buffers      */
    int32_t n_updates;          /* update() calls per tick, >= 1                                                             */
    int32_t only_unburned;      /* 1: a line is drawn on UNBURNED cells only; 0: always (also on a BURNING cell)             */
    int32_t done_on_burn;       /* 1: an agent standing in the fire ends the episode                                         */
    int32_t max_ticks;          /* > 0: the episode ends after this many ticks                                               */
    int32_t auto_reset;         /* 1: done environments start a new episode inside the call                                  */
    float w[4];                 /* reward weights of terms[0..3]                                                             */
} sf_agent_params;
typedef struct sf_agent_out {   /* device memory, any may be NULL                                                            */
    float *reward;              /* [n_envs]                                                                                  */
    uint8_t *done;              /* [n_envs]                                                                                  */
    int32_t *terms;             /* [n_envs][4]: newly BURNING + BURNED cells, points emitted, agents in the fire, blocked moves */
    int32_t *final_len;         /* [n_envs]                                                                                  */
    double *final_ret;          /* [n_envs]                                                                                  */
} sf_agent_out;
/* Allocates the agent state (all agents at (0, 0), ids 1..k, start cells (0, 0)); called again it replaces the state, k = 0 frees
 * it.  ignitions_xy: int32 [n_envs][2] host, where a done environment re-ignites (unused, may be NULL, without auto_reset).  k or
 * n_updates out of range or an ignition off the grid: SF_EINVAL. */
int sf_agents_create(sf_sim *sim, const sf_agent_params *params, const int32_t *ignitions_xy /* [n_envs][2] host */);
/* The k agents of environment envs[i] stand at xy[i] (int32 [n][k][2] = (column, row), host arrays); an environment named twice
 * keeps its last entry.  also_start != 0: these cells also become the environment's start cells and its episode statistics are
 * cleared (a new episode).  An environment out of range or a cell off the grid is SF_EINVAL before anything is enqueued. */
int sf_agents_place(sf_sim *sim, int32_t n, const int32_t *envs, const int32_t *xy /* [n][k][2] host */, int32_t also_start);
/* One tick (above).  device_actions: int32 [n_envs][k] in device memory; out may be NULL.  Before sf_agents_create: SF_ESTATE. */
int sf_agents_step(sf_sim *sim, const int32_t *device_actions /* [n_envs][k] */, const sf_agent_out *out);
/* The positions, int32 [n_envs][k][3] = (column, row, id = j + 1) in device memory: what sf_observe / sf_render take as agents
 * (agents_device = 1).  The address holds until the next sf_agents_create. */
int sf_agents_device(sf_sim *sim, void **xyid /* int32 [n_envs][k][3] */);

/* New episodes randomised on the device.  Step f of sf_agents_step re-ignites every done environment at the
 * same cell, under the same wind, with its agents at the same start cells: a deterministic simulator then replays one world for
 * ever.  With sf_episodes_set the parameters of a new episode are DRAWN, on the device, for exactly the environments a reset takes,
 * by a counter-based draw: what episode ep (0, 1, 2, ... counted per environment since sf_episodes_set) of environment env gets
 * depends on (seed, env, ep) alone - not on the tick, the launch structure or which other environments restart with it.
 *   mix(z):  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31             (mod 2^64)
 *   word(seed, env, ep, slot) = mix(mix(seed + G * (env + 1)) + G * ((uint64(ep) << 8) | slot)),  G = 0x9E3779B97F4A7C15
 *   an integer of [lo, hi] from a 32-bit half h: lo + ((uint64(h) * (hi - lo + 1)) >> 32)
 *   a double of [a, b) from a word w: a + (b - a) * ((w >> 11) * 2^-53), in double, the product rounded before the sum
 * Slots 0..63: the ignition attempts (x from the word's high half over the box's columns, y from its low half over its rows);
 * 64 + j: agent j's start cell (the same split over agent_box); 128: the wind speed, 129: the wind direction.
 *   SF_EP_IGNITION   the episode ignites at attempt 0's cell.  With SF_EP_LIVE_CELL at the cell of the FIRST attempt whose cell is
 *                    not dead - dead: all eight rates of the environment's R table are 0 there (unburnable fuel) -; if all 64
 *                    attempts hit dead cells, attempt 63's cell is taken as it is (the fire then goes out at once).
 *                    Without SF_EP_IGNITION new episodes ignite where the environment last ignited: the ignitions given to
 *                    sf_agents_create where agents exist, else those of the last sf_reset.
 *   SF_EP_WIND       a uniform wind U (ft/min) in [U[0], U[1]), U_dir (degrees) in [U_dir[0], U_dir[1]): the environment's R table is
 *                    rebuilt as by sf_set_wind behind the reset, inside the same call: the episode runs under its own wind from its
 *                    first update.  Needs per_env_terrain and layers in every table (SF_ESTATE), and excludes wind schedules: while
 *                    any schedule is set sf_episodes_set with SF_EP_WIND is SF_ESTATE, and while SF_EP_WIND is set
 *                    sf_set_wind_schedule is SF_ESTATE.  The cache of wind-independent terms (64 bytes per cell and table; counted
 *                    by sf_memory_bytes) is made current for every table; without memory for it the tables are built from the layers.
 *   SF_EP_AGENTS     every agent's start cell (and, on a restart, its position); agents may share a cell and may stand on the
 *                    ignition.  Allowed before sf_agents_create: it takes effect once agents exist, and a later
 *                    sf_agents_create keeps the setting.
 * sf_episodes_set: copies *params, zeroes every environment's episode index; NULL switches randomisation off and frees its buffers.
 * Unknown flag bits, reserved != 0, a box that is not x0 <= x1, y0 <= y1 on the grid (only the boxes of set flags are looked at), a
 * range that is not finite with lo <= hi (and U[0] >= 0), SF_EP_LIVE_CELL without SF_EP_IGNITION: SF_EINVAL before any device work.
 * Without SF_EP_IGNITION on a handle that has neither agents nor been reset: SF_ESTATE.  Ends a running closed loop; waits.
 * While it is set, step f of sf_agents_step draws before it resets (nothing else of a tick changes; off, a tick is what it was).
 * sf_episodes_begin: the mask form of sf_reset_where with drawn parameters, for callers without agents (and the first episodes of a
 * run): all != 0 takes every environment, else device_mask[e] != 0 decides, or - a null mask - "e is not running".  Needs
 * sf_episodes_set and sf_reset to have run once (SF_ESTATE); ends a running closed loop; under sf_set_async it only enqueues,
 * otherwise it waits once at its end.  As after sf_reset_where the next sf_get_fire_map_delta of every environment returns -1 once.
 * sf_episodes_device: zero-copy, for observations and logging - per environment the index of its NEXT episode (uint32), the last
 * ignition drawn (int32 (x, y); without SF_EP_IGNITION the fixed one) and the last wind drawn (double (U, U_dir); zeros before the
 * first draw and without SF_EP_WIND).  It reports DRAWS: a later sf_set_wind, sf_reset_envs or sf_copy_envs is not reflected.  The
 * addresses hold until the next sf_episodes_set; complete once the handle's stream has passed the call that drew.
 * The episode buffers belong to the handle, as the agent buffers do: sf_copy_envs and sf_save_state / sf_load_state do not carry
 * them (a forked or restored environment continues its own episode count).  Arrival recording: the plane of a restarted environment
 * is cleared and gets its ignition as in every reset.  The closed loop (sf_loop_start) has no resets inside it and draws nothing. */
#define SF_EP_IGNITION  1   /* draw the ignition cell in ign_box                                   */
#define SF_EP_LIVE_CELL 2   /* ... among cells whose R table is not all zero (64 attempts)         */
#define SF_EP_WIND      4   /* draw a uniform wind in [U[0], U[1]) x [U_dir[0], U_dir[1])          */
#define SF_EP_AGENTS    8   /* draw every agent's start cell in agent_box                          */
typedef struct sf_episode_params {
    uint64_t seed;
    int32_t flags, reserved;               /* reserved == 0 */
    int32_t ign_box[4], agent_box[4];      /* x0, y0, x1, y1, inclusive, on the grid, x0 <= x1, y0 <= y1 */
    double U[2], U_dir[2];                 /* lo <= hi, finite, U[0] >= 0 */
} sf_episode_params;
int sf_episodes_set(sf_sim *sim, const sf_episode_params *params /* NULL: off, buffers freed */);
int sf_episodes_begin(sf_sim *sim, const uint8_t *device_mask /* [n_envs] or NULL */, int32_t all);
int sf_episodes_device(sf_sim *sim, void **index /* u32 [n_envs] */, void **ignition /* i32 [n_envs][2] */, void **wind /* f64 [n_envs][2] */);

/* Frames of environments: what the reference's screen shows (simfire/game/game.py:117-131: the terrain image,
 * sprites.py:105-160 with the burned paint, the fire / line / agent sprites of sprites.py:20-203 in SpriteLayer order, enums.py:88-103)
 * as uint8 RGB, one pixel per cell, downscaled by an integer factor, written by ONE launch into caller-owned device memory.  It replaces
 * sim.rendering + game.update + Game.save (simulation.py:534-537, game.py:295-315) for a headless caller.  Frame t shows the state AFTER
 * update t (the reference's screen lags by up to one update; not reproduced).  The status bytes are read from whichever plane is
 * current, or from the history ring; no state of the handle changes (the current plane, the tile books, the reference point of
 * sf_get_fire_map_delta, the result block).  The per-table background (fuel colour + contour bit) is rebuilt on the device when the
 * layers or terrain_rgb changed since it was last built. */
#define SF_RENDER_MAX_SCALE 64
#define SF_RENDER_MAX_AGENTS 256
#define SF_RENDER_CURRENT 0        /* source: the current state                                                               */
#define SF_RENDER_HISTORY 1        /* source: the history ring of sf_enable_history, updates first .. first + count - 1      */
#define SF_RENDER_NEAREST 0        /* mode: the cell at (oy * scale, ox * scale)                                              */
#define SF_RENDER_MEAN 1           /* mode: per channel (sum + n / 2) / n over the block's n cells                           */
#define SF_RENDER_SPRITES 2        /* mode: the block's highest sprite (agent > wet > scratch > fire line > burning), else mean */
#define SF_RENDER_FUEL 0           /* background: FuelLayer.image (layers.py:654-667, 744-768)                                */
#define SF_RENDER_WHITE 1          /* background: white, what the v2.0.1 screen shows (sprites.py:155 draws the fuel image with alpha 0) */
typedef struct sf_render_params {
    int32_t source;                /* SF_RENDER_CURRENT / SF_RENDER_HISTORY                                                   */
    int32_t first, count;          /* history: frame t of an environment shows update first + t (sf_get_history numbering),   */
                                   /* 1 <= count <= capacity; current: ignored, one frame per environment                      */
    int32_t scale;                 /* 1..SF_RENDER_MAX_SCALE; oh = ceil(H / scale), ow = ceil(W / scale): the last partial     */
                                   /* block uses the cells it has                                                              */
    int32_t mode;                  /* SF_RENDER_NEAREST / MEAN / SPRITES (all the same at scale 1)                              */
    int32_t background;            /* SF_RENDER_FUEL / SF_RENDER_WHITE                                                         */
    int32_t contours;              /* 1: contour pixels are black                                                              */
    int32_t terrain_rgb[3];        /* 0..255: the terrain texture colour functional fuel is blended from                      */
    int32_t channels_last;         /* 1: out[frame][oh][ow][3], 0: out[frame][3][oh][ow]                                      */
    int32_t agents_k;              /* entries per environment of agents, 0..SF_RENDER_MAX_AGENTS                               */
    int32_t agents_device;         /* agents is a device pointer                                                               */
    const int32_t *agents;         /* int32 [n][agents_k][3] = (column, row, id) as sf_observe takes them; null: no agents    */
} sf_render_params;
/* Environment envs[i] (a host array; repeats allowed) lands in frames i * count .. i * count + count - 1 (count = 1 for the current
 * state).  Anything invalid is SF_EINVAL before a launch; a listed environment without layers (sf_set_layers*, sf_generate_layers)
 * and a history source without sf_enable_history are SF_ESTATE.  In async mode the call only enqueues. */
int sf_render(sf_sim *sim, const sf_render_params *params, int32_t n, const int32_t *envs, void *device_out);

/* Device buffer int32 [n_envs][8] filled by sf_update_status_device (same content as
 * sf_get_status) - the block that is all-gathered over RCCL by the multi-GPU host code. */
int sf_status_device(sf_sim *sim, void **ptr);
int sf_update_status_device(sf_sim *sim);
/* Refresh the result block and copy it (device to device) into caller-owned device memory,
 * e.g. the torch tensor that is then all-gathered over RCCL. */
int sf_copy_status_to(sf_sim *sim, void *device_dst /* int32 [n_envs][8] */);
/* A rollout in one call: sf_step(sim, n_steps) without a host wait of its own, then sf_copy_status_to(sim, device_dst) - n calls of
 * FireSimulation.run(1) per environment (simulation.py:501-553) and the attributes a harness reads afterwards (541-553), one
 * launch and one wait on grids the resident launch covers.  The handle's asynchronous mode is left as it was; a handle IN asynchronous
 * mode (sf_set_async) only enqueues - the block is in device_dst when the handle's stream has got there: sf_sync, or the caller's own
 * device-wide synchronisation (a harness whose next consumer is a kernel waits for nothing on the host). */
int sf_rollout(sf_sim *sim, int32_t n_steps, void *device_dst /* int32 [n_envs][8] */);
/* Register caller-owned device memory (int32 [n_envs][8]; NULL unregisters) as a second home of the
 * result block: every refresh of the block also writes it there.  In particular the resident launch
 * of sf_step(n >= 2) leaves the block behind itself (every workgroup counts its own environment when
 * its steps are done), so a rollout `sf_step(n)` in async mode + `sf_copy_status_to(sim, same pointer)`
 * costs one launch and one wait, and the episode returns (FireSimulation attributes of
 * simulation.py:541-553) are already in the harness's tensor.  The buffer must stay valid until it is
 * unregistered or the handle is destroyed. */
int sf_set_result_sink(sf_sim *sim, void *device_dst /* int32 [n_envs][8] or NULL */);

/* The ONE collective of the path, for hosts that have no torch.distributed: an all-gather of the result blocks of the
 * ranks' shards over RCCL (xGMI inside a node).  Environments never read each other's state (simulation.py:202-214: one
 * FireSimulation object each), so nothing else is ever exchanged.  librccl is loaded on first use (dlopen), not linked: a
 * one-GPU host needs no RCCL.  One process per GPU; every rank's handle holds the same number of environments.
 *   rank 0:  sf_comm_unique_id(id)  -> hand the 128 bytes to the other ranks (file, socket, MPI, the launcher's store)
 *   all:     sf_comm_init(sim, rank, world, id)          (collective: returns when every rank has called it)
 *   rollout: sf_step(sim, n) ... sf_allgather_status(sim, out)   out = device int32 [world][n_envs][8], rank-major
 *   end:     sf_comm_destroy(sim)                        (sf_destroy does it too) */
int sf_comm_unique_id(void *id_out /* 128 bytes */);
int sf_comm_init(sf_sim *sim, int32_t rank, int32_t world_size, const void *unique_id /* 128 bytes */);
int sf_allgather_status(sf_sim *sim, void *device_out /* int32 [world_size * n_envs][8] */);
int sf_comm_destroy(sf_sim *sim);

/* Drop-in for compute_rate_of_spread (rothermel.py:4-22): 17 float32 vectors of length n ->
 * R float64[n] (ft/min). */
int sf_compute_ros(int64_t n, const float *loc_x, const float *loc_y, const float *new_loc_x,
                   const float *new_loc_y, const float *w_0, const float *delta, const float *M_x,
                   const float *sigma, const float *h, const float *S_T, const float *S_e,
                   const float *p_p, const float *M_f, const float *U, const float *U_dir,
                   const float *slope_mag, const float *slope_dir, double *R_out, int32_t device);
/* Overwrite the ignition threshold only (the reference's tests assign manager.pixel_scale after
 * construction, test_fire.py:334; slopes keep the constructor value, fire.py:377). */
int sf_set_threshold(sf_sim *sim, double pixel_scale);
/* Asynchronous mode for rollout loops: sf_step / sf_apply_mitigation only enqueue work on the
 * handle's stream; every call that hands data back (sf_get_*, sf_step_timed, sf_copy_status_to,
 * sf_sync) synchronises.  Default: off (every call returns after its work is done). */
int sf_set_async(sf_sim *sim, int32_t on);
int sf_sync(sf_sim *sim);
/* Spread graph by-product - FireSpreadGraph.add_edges_from_manager (simfire/utils/graph.py:84-150,
 * called at fire.py:584): when enabled, every ignition records which of its 8 neighbours were
 * BURNING at that moment.  parents = uint8 [H*W]; bit j <=> edge from neighbour j of graph.py's
 * adj_locs order (x+1,y) (x+1,y+1) (x,y+1) (x-1,y+1) (x-1,y) (x-1,y-1) (x,y-1) (x+1,y-1). */
int sf_enable_spread_graph(sf_sim *sim, int32_t on);
int sf_get_spread_parents(sf_sim *sim, int32_t env, uint8_t *parents_out);
/* RothermelFireManager.update called again after it returned QUIT on the runtime check still prunes and ages the
 * sprites (fire.py:631-643 run before the check at 641): 1 = sf_step does the same for such environments (they stay
 * QUIT in the result block, spread stays off); 0 (default) = a QUIT environment is frozen, as FireSimulation.run
 * (simulation.py:533) never calls update again. */
int sf_set_prune_after_quit(sf_sim *sim, int32_t on);
/* A rollout in which control lines are drawn before every update - the loop of an RL harness whose agents' moves are known
 * in advance,   for s in range(n_steps): sim.update_mitigation(points[s]); sim.run(1)   (simulation.py:449-478, 501-553;
 * BASELINE config C5) - as ONE call.  pts: int32 [n_steps][n_envs][k][3] = (column, row, type) per environment and step, a
 * host pointer (device_pointer = 0) or a device pointer (1); entries whose type is not a control line (3, 4, 5) or whose
 * position is off the grid are skipped (use them as padding).  Where the environment-resident launch can run, an
 * environment's points are applied inside the kernel right before that environment's update; otherwise the call enqueues
 * n_steps scatter + step pairs.  ms_out (may be null): GPU milliseconds of the call. */
int sf_step_mitigated(sf_sim *sim, int32_t n_steps, const int32_t *pts, int32_t k, int32_t device_pointer, float *ms_out);
/* The closed loop of an RL harness - FireSimulation.update_mitigation(actions that depend on the last observation) followed
 * by run(1), simulation.py:449-478 and 501-553 - without a launch per step.  sf_loop_start leaves the environment-resident
 * launch on the GPU (one workgroup per environment, so: grids up to 1024 x 1024, no more environments than CUs); sf_loop_step
 * posts one step's points (int32 [n_envs][k][3] = column, row, type; k <= 64 as given to sf_loop_start; a type outside 3..5 is
 * padding; null = none) into host-mapped memory, rings a doorbell, waits until every environment has made
 * `update_mitigation(points); run(1)` and returns the result block of sf_get_status (either pointer may be null).
 * sf_loop_stop - or any other call on the handle - ends the loop: the workgroups commit their environments and leave.  A launch
 * that hears nothing for ~0.2 s leaves by itself (a host that went away cannot hang the GPU); the next sf_loop_step starts it
 * again, every environment resumes from the last step IT finished (sf_loop_restarts counts these).  While the loop is on the
 * GPU's CUs are taken: a policy network on the SAME GPU cannot run beside it (use sf_apply_mitigation_device + sf_step there). */
int sf_loop_start(sf_sim *sim, int32_t k);
int sf_loop_step(sf_sim *sim, const int32_t *points, int32_t *status_out, double *elapsed_out);
int sf_loop_stop(sf_sim *sim);
int sf_loop_restarts(sf_sim *sim, int32_t *count_out);

/* ---------------------------------------------------------------------------------------------- CFD wind field
 * The stable-fluids velocity solver behind `wind.function: cfd`: WindControllerCFD + Fluid
 * (simfire/world/wind_mechanics/wind_controller.py:100-185, cfd_wind.py:8-298), batched over n_envs independent
 * environments of one grid size, bit-identical to the reference's float64 loops.  Grids are square (the reference's
 * set_bnd raises IndexError on any other, cfd_wind.py:104-165) with 4 <= n <= 4096.  Arrays are [n][n] row-major with
 * the reference's first index i first (x[i][j]).  The density plane is not computed: it never feeds the velocity. */
typedef struct sf_cfd sf_cfd; /* opaque */
typedef struct sf_cfd_params {
    int32_t n;                /* screen_size[0] == screen_size[1]                                        */
    int32_t n_envs;           /* independent solvers batched in one launch (one workgroup each)          */
    int32_t result_accuracy;  /* Gauss-Seidel passes of every lin_solve (Fluid.itr, cfd_wind.py:176)    */
    int32_t direction;        /* inflow side: 0 north, 1 east, 2 south, 3 west (wind_controller.py:156-170) */
    double timestep_dt;       /* Fluid.dt                                                                */
    double viscosity;         /* Fluid.visc (diffuse's coefficient for the velocity, cfd_wind.py:50-51)  */
    double speed;             /* wind_speed added by the inflow                                          */
} sf_cfd_params;

/* Fluid.__init__ (cfd_wind.py:9-40): Vx, Vy, Vx0, Vy0 zeroed, every terrain mask zero (no terrain).  n < 4 -> SF_ESHAPE. */
int sf_cfd_create(const sf_cfd_params *params, sf_cfd **out);
int sf_cfd_destroy(sf_cfd *h);
/* Terrain mask of environment env (-1: every environment): uint8 [n][n], 1 where elevation > np.average(elevation)
 * (wind_controller.py:131-143; the caller forms it), else 0. */
int sf_cfd_set_terrain(sf_cfd *h, int32_t env, const uint8_t *mask);
/* n_steps Fluid.step()s (cfd_wind.py:49-60) on every environment; step k of this call is preceded by the inflow of
 * iterate_wind_step (wind_controller.py:156-170) when inflow_every > 0 && k % inflow_every == 0.  Training as in
 * generate_cfd_wind_layer (generate_cfd_wind_layer.py:99-105) for T iterations is (2T, 2); iterate_wind_step() is
 * (1, 1) and fvect.step() (1, 0).  The host splits the call into launches of bounded length; the state stays on the device. */
int sf_cfd_step(sf_cfd *h, int32_t n_steps, int32_t inflow_every);
/* Fluid.Vx / Fluid.Vy of environment env (get_wind_velocity_field_x/_y, wind_controller.py:178-182): float64 [n][n]
 * each; a null pointer is skipped. */
int sf_cfd_get_velocity(sf_cfd *h, int32_t env, double *vx, double *vy);

#ifdef __cplusplus
}
#endif
#endif /* SIMFIRE_HIP_H */
