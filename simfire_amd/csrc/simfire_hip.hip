// MI355X (gfx950 / CDNA4) Rothermel fire-spread stepper - kernels + C ABI (include/simfire_hip.h).
//
// What it replaces (reference mitrefireline/simfire v2.0.1):
//   RothermelFireManager.update / _prune_sprites / _get_new_locs / _update_rate_of_spread /
//   _update_with_new_locs          simfire/game/managers/fire.py:116-284, 550-589, 616-719
//   RothermelFireManager._compute_slopes                         fire.py:436-449
//   compute_rate_of_spread                                       simfire/world/rothermel.py:4-136
//   ControlLineManager.update + FireSimulation.update_mitigation mitigation.py:60-80, simulation.py:449-478
//
// Design (DESIGN.md has the derivation and the measurements):
//   * State per environment, structure-of-arrays in HBM, row pitch P = roundup(W, 16) bytes:
//       status u8 [H][P]      BurnStatus (the plane is fire_map as uint8)
//       age    u8 [H+2][P]    bitmask of the live sprites of a cell, indexed by ABSOLUTE ignition
//                             step modulo N = max_fire_duration + 3 (one zero guard row above/below)
//       burn   f64 [H][P]     RothermelFireManager.burn_amounts
//       settled u32 [H][P]    (attenuate_line_ros only) complete-update count a control-line cell is paid up to
//       seam   u8 [P/64+1][2][H+pad]  copies of the sprite-mask columns at the chunk boundaries
//     shared by all environments: rt f64 [8][H][P], the rate-of-spread table (ft/min), and a
//     per-wave-tile activity map (u8 flags: sprites in tile / on which edges).
//   * The reference's ordered sprite list is replaced by the order-free per-cell rule of
//     SURVEY.md section 8a.  Ages are not shifted every step: a sprite ignited at step s owns
//     bit (s mod N) until it is recycled at step s + max_fire_duration + 2, so the planes are
//     only written where something happens, and a step runs IN PLACE: every concurrent writer of
//     a step touches only the two slots (t and t - md - 2) that readers mask out.
//   * n steps of an sf_step(n) call = ONE launch of k_run (sf_run_kernels.h): a workgroup owns an environment for all n
//     steps, its vector bitmaps live in LDS, the cells in a blocked plane (sf_common.h); the automatic choice for n >= 2 on
//     grids up to 1024 cells wide.  Otherwise:
//   * One step = k_select + k_step.  k_select (one thread per 64 x 32 wave tile) folds the
//     per-environment predicates of fire.py:637-652 of the previous step (3-deep ring of flag
//     words), and compacts the tiles in which anything can change into a list (ballot + mbcnt +
//     one atomic per workgroup).  k_step: persistent waves walk that list; a wave loads its tile
//     (16 cells per lane, 16 B vectors) plus halo rows / seam columns, parks it in LDS, scans it
//     SWAR (4 cells per VALU op) for expiring sprites and frontier cells (eligible status next
//     to a live sprite), compacts those with one wave prefix sum into an LDS list and walks the
//     list one cell per lane: winner source from the 3 x 3 LDS neighbourhood, one f64 table
//     entry, f64 burn update, ignition.  Changed 16 B vectors are written back once.
//   * The whole-grid attenuation of control-line cells (fire.py:271-278) is lazy: a line cell is
//     touched only when it becomes a candidate, is overwritten or burn_amounts is read back; the
//     subtractions it is owed by then are made up bit for bit (lazy_sub, sf_common.h).
//   * A per-step launch lasts as long as its slowest wave (all live tiles are resident at once), so those
//     kernels are organised around a short per-tile dependency chain, not around throughput.
//
// No MFMA: there is no dense contraction anywhere on this path; it is byte / integer work plus a
// handful of float64 adds per frontier cell.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (no fast-math: burn_amounts and the
// ignition test burn > pixel_scale must round exactly like IEEE float64 on the CPU).
#include <emmintrin.h>
#include <hip/hip_runtime.h>

#include <cassert>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <algorithm>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include <dlfcn.h>
#include <rccl/rccl.h>        // types only: the library is loaded with dlopen on first use (sf_comm_*)

#include "../../include/simfire_hip.h"
#include "rothermel_dev.h"

// ------------------------------------------------------------------------------- errors
static thread_local std::string g_err;
static int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
#define HIPCHK(expr)                                                                      \
    do {                                                                                  \
        hipError_t _e = (expr);                                                           \
        if (_e != hipSuccess)                                                             \
            return fail(SF_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),   \
                        __FILE__, __LINE__);                                              \
    } while (0)

extern "C" const char *sf_last_error(void) { return g_err.c_str(); }
// the other translation units report through the same per-thread message (simfire_hip_cfd.hip)
int sf_fail_message(int code, const char *msg)
{
    g_err = msg;
    return code;
}
extern "C" const char *sf_version(void) { return "simfire_hip 0.2 (gfx950)"; }      // 0.2: the knob numbers and the 16 counter slots of simfire_hip_lab.h as they stand since round 5; sf_get_fire_map_delta

#include "sf_common.h"
#include "sf_step_kernels.h"
#include "sf_aux_kernels.h"
#include "sf_run_kernels.h"
#include "sf_run_table.h"
#include "sf_state_kernels.h"
#include "sf_reset_kernels.h"
#include "sf_obs_kernels.h"
#include "sf_render_kernels.h"
#include "sf_gen_kernels.h"
#include "sf_agent_kernels.h"
#include "sf_arrival_kernels.h"
#include "sf_value_kernels.h"
#include "sf_ensemble_kernels.h"
#include "sf_wind_kernels.h"
#include "sf_episode_kernels.h"

// Launch-geometry knobs of a handle (sf_set_tuning, include/simfire_hip_lab.h: SF_TUNE_*).  Results never depend on them; the
// defaults are the measured choices of NOTEBOOK.md 5.  The library does not read the environment for them (the measurement scripts under
// profiles/ set them through the Python binding, simfire_amd/engine.py: SF_DEBUG_KNOBS).
struct Tuning {
    int v[SF_TUNE_COUNT];
    bool set[SF_TUNE_COUNT];
};
static const int kTuneDefault[SF_TUNE_COUNT] = {
    /* SF_TUNE_WAVES_PER_CU */ 24, /* RUN_WAVES */ 16, /* RUN_MIN_ENVS */ 1, /* RUN_VCAP */ 4096, /* RUN_COMPACT */ 1,
    /* RUN_BATCH */ 64, /* RUN_RESULT */ 1, /* RUN_SEGMENT */ 64, /* RUN_TEAM */ 0, /* TEAM_PLACEMENT */ 0, /* TEAM_RECUT */ 1, /* RUN_WINDOW */ 1, /* TEAM_TIMEOUT_MS */ 2000,
    /* RUN_JOIN */ 1, /* LOOP_LIGHT */ 0};

// What a batched call sends ahead of its kernels (environment list, descriptors, host points): a device buffer, the pinned mirror it
// is copied from, and the event that marks the copy's completion - the next call of the feature waits for it before it writes the
// mirror again, so a call in async mode never waits for the one before it unless the mirror is still being read (block_reserve /
// block_send).  One block per feature: a shared one would make one feature's calls wait for another's.
struct CallBlock {
    uint8_t *dev = nullptr, *pinned = nullptr;
    size_t cap = 0;
    hipEvent_t ev = nullptr;
};

// ----------------------------------------------------------------------------- handle
struct sf_sim {
    sf_params p;
    Geo g;
    hipStream_t stream = nullptr;
    int loop_light = 0;                 // 1: the running closed loop is the light one (8-wave workgroups; SF_TUNE_LOOP_LIGHT)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    uint8_t *status = nullptr, *age_alloc = nullptr, *age = nullptr;
    uint8_t *cells_alloc = nullptr, *cells = nullptr;      // blocked cell plane of the resident launch (allocated at its first use)
    bool bl_cur = false;               // the blocked plane holds the sprite masks / status bytes; the row-major planes are stale
    double *burn = nullptr, *rt = nullptr;
    mutable std::map<std::tuple<const void *, unsigned, size_t>, int> occ_cache;      // k_run instantiations: workgroups per CU by hipOccupancyMaxActiveBlocksPerMultiprocessor (occupancy)
    double *rtc = nullptr;             // the R table(s) cell-major (k_rt_cellmajor): built when the resident launch first needs it, stale after every change of rt
    bool rtc_valid = false;
    std::vector<char> rtc_stale;       // per table: its cell-major copy does not match rt (all of them until the copy exists)
    unsigned long long *win_hint = nullptr;      // k_run's window phase: where the fire stood and where the window was when the phase last ended, per environment; 0 = unknown.  ADVICE only (sf_win_kernels.h)
    double *lay_all = nullptr;         // [tables][7][H*W] dense: w0 delta Mx sigma elev U Udir (kept for the observation planes)
    double *layer(int table, int i) const { return lay_all + ((size_t)table * 7 + i) * (size_t)g.H * g.W; }
    int8_t *history = nullptr;         // sf_enable_history: [E][history_cap][H][W] fire maps after each update
    int history_cap = 0;
    double *smag = nullptr, *sdir = nullptr;
    double slope_scale = 0.0;          // pixel_scale of the constructor: np.gradient spacing (fire.py:446), whatever the threshold becomes
    EnvState *commit = nullptr, *tmp = nullptr;
    uint32_t *flags = nullptr;
    unsigned long long *counters = nullptr;
    uint8_t *tflags = nullptr;
    size_t tflags_bytes = 0;
    int ring = 0;                      // tile activity map the next step reads (0/1)
    uint32_t *tile_list = nullptr, *n_active = nullptr;
    int n_cu = 256;
    int fused_mode = -1;               // -1 auto, 0 k_select + k_step, 1 one fused launch per step, 2 one resident launch per sf_step call
    bool generic = false;              // sf_set_generic: per-cell kernel instead of the tiled SWAR kernels
    uint8_t *seam = nullptr;           // seam planes (tiled kernels, 1-byte sprite plane)
    uint32_t *settled = nullptr;       // attenuation bookkeeping per cell (attenuate_line_ros only)
    uint8_t *tdirty = nullptr;         // per wave tile: status histogram stale
    uint16_t *thist = nullptr;         // per wave tile: cells per BurnStatus 1..5 (u16 [tiles][8])
    size_t n_tiles_max = 0;
    void *status_pinned = nullptr;     // pinned landing zone of the result block (int32 [E][8] + double [E])
    bool status_fresh = false;         // status_block / elapsed_dev (and the sink) hold the current result block: the resident launch wrote it
    int32_t *sink = nullptr;           // sf_set_result_sink: caller-owned device copy of the result block, written by every refresh
    bool tdirty_all = true;            // every histogram is stale (reset, fire_map replaced, geometry changed, per-cell kernel ran)
    int last_launches = 0;             // k_run launches of the last step call (sf_get_last_launches)
    // run(1) loops (one update per call, the result block looked at after each - FireSimulation.run(1) in a harness): after two such
    // pairs in a row the single update runs as the resident launch too, which leaves the block behind itself (measured, step(1) +
    // status() per call: 41 against 46 us on one environment, 47 against 58 on C3's 256; a loop that only enqueues step(1) calls, or
    // looks at the maps after each, is faster on the per-step kernels and keeps them)
    bool last_was_step1 = false;       // the last step call was one update and nothing has looked at its result yet
    int step1_polls = 0;               // step(1) + status pairs in a row
    int fire_rows = 0;                 // no environment's fire spans more rows than this (0: not known): 1 after sf_reset, + 2 per update (a fire
                                       // advances one row per update at most, fire.py:163-234), the grid's height after sf_load_fire_map
    unsigned long long *vbits = nullptr;   // vector bitmap of the resident launch (k_run)
    bool vbits_valid = false;          // vbits matches the sprite-mask planes (k_run / reset keep it; the per-step kernels do not)
    bool vbits_fl_valid = true;        // ... planes 1 / 2 of it too (first / last cell of the vector holds a sprite bit): k_run on rows of several words keeps only
                                       // plane 0 (plain dilation) unless it runs as teams - which need all three (rebuilt when a team launch follows such a launch)
    bool tiles_valid = false;          // tile activity map + seam planes match them (the per-step tiled kernels keep them; k_run does not)
    int last_kind = -1;                // launch structure of the last sf_step call: 0 k_select + k_step, 1 fused, 2 k_run, 3 per-cell
    int32_t *todo = nullptr;           // team launches with windows of rows: the steps an environment's team could not make (the catch-up launch's) [E]
    ncclComm_t comm = nullptr;         // sf_comm_init: communicator of the result-block all-gather
    int comm_world = 0;
    // k_run<TEAM>: an environment served by several workgroups (sf_run_kernels.h); allocated at the first team launch
    uint32_t *team_tab = nullptr, *team_size = nullptr, *xdone = nullptr;
    uint32_t *xj = nullptr;            // k_run<TEAM = 2> (teams that grow inside the launch): names put down / the board / counters (StepArgs::xj)
    unsigned long long *xcut = nullptr;
    uint32_t *jlog = nullptr;          // what happened to the teams in the last such launch (sf_get_join_log)
    bool jlog_valid = false;
    unsigned long long *xg = nullptr;
    uint8_t *xbuf = nullptr;
    uint32_t *xerr_pinned = nullptr, *xerr_mapped = nullptr;
    int team_slots = 0;                // entries of team_tab
    long long team_plan_ones = 0;      // != 0: team_tab / team_size hold the plan "every environment one workgroup" for this (E, slots, placement) - k_team_plan need not run again for it
    // LOOP mode (sf_loop_start): the resident launch driven step by step through host-mapped memory
    bool loop_on = false;
    int loop_k = 0;                    // points per environment and step
    uint32_t loop_seq = 0;             // sequence number of the last step posted
    uint32_t *loop_db = nullptr, *loop_db_dev = nullptr;         // (pinned, device-mapped) [0] doorbell, [64 ...] "done" numbers [E] (other cache lines)
    int32_t *loop_res = nullptr, *loop_res_dev = nullptr;        // u32 [E][16]: one 64-byte line per environment (pinned, device-mapped; k_run, loop_finish)
    int32_t *loop_pts = nullptr, *loop_pts_dev = nullptr;        // [2][slot] points ring (pinned, device-mapped)
    size_t loop_pts_cap = 0, loop_slot_ints = 0;
    uint32_t *loop_mem = nullptr;                                // device: [0] forwarded sequence number, [32 ...] done [E]
    int32_t *loop_pts_mem = nullptr;                             // device copy of the ring
    size_t loop_pts_mem_cap = 0;
    int loop_restarts = 0;             // times the launch had left by itself (timeout) and was started again
    int last_team_max = 0;             // upper bound of the team sizes in the last resident launch (0: it was not a team launch)
    int cost_steps = 0;                // steps the per-environment cost array covers (0: nothing recorded since the last reset)
    uint32_t *todo_cnt = nullptr;      // k_win: how many environments it left updates for (their numbers: run_order); two counts, by the parity of win_seq
    unsigned win_seq = 0;              // k_win launches so far
    uint32_t *run_cost = nullptr, *run_order = nullptr;   // k_run: clocks / 16 an environment's workgroup took in the last resident launch [E]; launch order built from it (k_order)
    mutable std::map<const void *, size_t> lds_allowed;       // dynamic LDS the resident kernels have been enabled for, by host handle (allow_lds)
    uint8_t *parents = nullptr;        // spread-graph parent masks, allocated by sf_enable_spread_graph
    bool graph_on = false;
    // sf_enable_arrival: the plane u32 [E][H][P] (update that created a cell's first sprite + 1, 0 = never; null =
    // recording off), updates made since the last pass (< md between the pieces of a call, 0 between calls), the lab's "always the
    // dense pass" and its count of passes made in the sparse / the dense form
    uint32_t *arrival1 = nullptr;
    int arr_pending = 0;
    bool arr_dense = false;
    int64_t arr_passes[2] = {0, 0};
    // sf_values_set: the handle's copy of the value plane, int32 [n][H][P] with n = E (val_per_env) or 1 and zeros
    // in the pitch padding (null = the feature is off); ONE allocation for the records ValueRec [E], tick_base and tick_loss int64 [E]
    // and the word the range check of a device plane leaves; the lab's "always the dense pass" and its count of passes made in the
    // sparse / the dense form; the fifth reward weight of sf_agents_step
    int32_t *val_plane = nullptr;
    bool val_per_env = false;
    uint8_t *val_aux = nullptr;
    bool val_dense = false;
    int64_t val_passes[2] = {0, 0};
    float val_w = 0.0f;
    bool val_w_on = false;
    size_t val_plane_bytes() const { return (size_t)(val_per_env ? g.E : 1) * g.plane_env * sizeof(int32_t); }
    size_t val_aux_bytes() const { return (size_t)g.E * (sizeof(ValueRec) + 16) + 16; }
    ValueRec *val_rec() const { return reinterpret_cast<ValueRec *>(val_aux); }
    long long *val_tick(int i) const { return reinterpret_cast<long long *>(val_aux + (size_t)g.E * (sizeof(ValueRec) + 8 * i)); }      // 0: base, 1: loss
    uint32_t *val_bad() const { return reinterpret_cast<uint32_t *>(val_aux + (size_t)g.E * (sizeof(ValueRec) + 16)); }
    // sf_get_fire_map_delta: the fire maps as the host last saw them (u8 [E][H][P], allocated at the first call), per environment whether that
    // reference point exists, the list of changed cells on the device ([0] = count) and its pinned landing zone
    uint8_t *snap = nullptr;
    std::vector<char> snap_valid;
    uint32_t *delta_dev = nullptr, *delta_pinned = nullptr;
    int delta_cap = 0;
    uint32_t delta_base = 0;           // what the list's count stood at after the last query (it counts on: nothing zeroes it)
    int32_t *status_block = nullptr;   // [E][8]
    double *elapsed_dev = nullptr;     // [E]
    void *stage = nullptr;             // dense staging for host copies
    size_t stage_bytes = 0;
    // control-line points: a ring of pinned, device-mapped staging buffers which the scatter kernels read
    // directly, so that in async mode the host can run several scatter + step pairs ahead of the GPU
    static constexpr int kPtsRing = 16;
    int32_t *pts_pinned[kPtsRing] = {}, *pts_mapped[kPtsRing] = {};
    size_t pts_cap = 0;
    hipEvent_t ev_pts[kPtsRing] = {};
    int pts_slot = 0;
    int32_t *mit_stage = nullptr;      // sf_step_mitigated: device copy of a host point block / expanded rows of one step
    size_t mit_stage_bytes = 0;
    bool async = false;                // sf_set_async: calls that return no data do not synchronise
    CallBlock obs_blk;                 // sf_observe: ObsHead, environment list, host centers / agents
    // sf_render: per table, layers present / FBFM-coded fuel / background stale; the background words [tables][H * W], the FBFM
    // colour index plane [tables][H * W] (allocated by the first sf_set_layers_fbfm), the terrain_rgb the fuel colours were made from
    // (-1: none yet) and the per-call block (lists of environments and tables, the min / max words its kernels write, host agents)
    std::vector<char> rd_lay, rd_fbfm, rd_stale;
    uint32_t *rd_bg = nullptr;
    uint8_t *rd_fuel_ix = nullptr;
    int64_t rd_rgb = -1;
    CallBlock rd_blk;
    CallBlock rs_blk;                  // sf_reset_envs / sf_reset_where: the environment list and host ignitions of a call
    bool rs_timed = false, rs_have_ms = false;   // sf_time_resets: ev0 / ev1 recorded around the launches of every batched reset
    CallBlock gen_blk;                 // sf_generate_layers: its descriptors + environment list
    // wind changes: the cache plane of wind-independent terms, float [tables][kWindPlanes][H * W], allocated at the
    // first wind change, and per table whether its part is stale (next to rtc_stale; wt_off: the lab has switched the cache off); the
    // schedules on the device [E] with their host mirror (segments per environment, the scheduled environments, whether the cache has been
    // made current for them since the last change of either), the due list of a schedule pass and its winds; the call block (list, scalars,
    // schedule rows); the lab's events around the launches
    float *wterms = nullptr;
    std::vector<char> wt_stale;
    bool wt_off = false;
    WindSched *wsched = nullptr;
    std::vector<int32_t> wind_K, wind_sched;
    bool wind_sched_ready = false, wind_sched_cached = false;
    int32_t *wdue = nullptr;
    uint32_t *wdue_cnt = nullptr;
    double *wdue_U = nullptr, *wdue_D = nullptr;
    CallBlock wind_blk;
    bool wind_timed = false, wind_have_ms = false;
    // sf_agents_* (DESIGN.md section 16): the parameters of sf_agents_create (ag.k == 0: no agent state), ONE device allocation that
    // holds every agent buffer - positions, start cells, this tick's points, the counts and episode statistics between the two
    // kernels of a tick, the done mask, the ignitions of a new episode - and the call block of sf_agents_place.  Not slices of
    // env_segs: fork, snapshot and restore do not carry agents.
    sf_agent_params ag = {};
    uint8_t *ag_mem = nullptr;
    size_t ag_bytes = 0;
    int32_t *ag_xyid = nullptr, *ag_start = nullptr, *ag_points = nullptr, *ag_prev = nullptr, *ag_terms = nullptr, *ag_len = nullptr, *ag_ign = nullptr;
    double *ag_ret = nullptr;
    uint8_t *ag_done = nullptr;
    CallBlock ag_blk;
    CallBlock ens_blk;                 // sf_ensemble_stats: the member list of a call
    bool ag_has_ign = false;           // sf_agents_create was given ignitions
    // sf_episodes_* (DESIGN.md section 19): the parameters of sf_episodes_set (ep_on: randomisation is set) and ONE device allocation
    // for the episode buffers - the next episode's index, the ignition a new episode takes (drawn, or the fixed one), the last wind
    // drawn, the due list k_episode_draw leaves for k_wind_rtable (the list, its count, the winds) and a mask of ones (all = 1).
    // The handle's like the agent buffers: not slices of env_segs.  last_ign: the ignitions of the last sf_reset (host copy).
    // ep_nocache: the cache of wind-independent terms could not be had (no memory, or the lab has it off): not asked for again
    // until sf_episodes_set / sf_set_wind_lab.
    sf_episode_params ep = {};
    bool ep_on = false, ep_nocache = false;
    uint8_t *ep_mem = nullptr, *ep_ones = nullptr;
    size_t ep_bytes = 0;
    uint32_t *ep_index = nullptr, *ep_due_cnt = nullptr;
    int32_t *ep_ign = nullptr, *ep_due = nullptr;
    double *ep_wind = nullptr, *ep_due_U = nullptr, *ep_due_D = nullptr;
    std::vector<int32_t> last_ign;
    bool have_rt = false, was_reset = false, counters_on = false;
    int seq = 0;                       // index (mod 6) of the next step launch
    Tuning tune;                       // sf_set_tuning
    bool committed = true;             // commit[] is current (no step launch since the last k_commit / reset)
    std::vector<char> rt_set;          // per table: layers / R table supplied?
    int64_t bytes = 0;
};

// The host code of the step path has two layers.  The ENQUEUE layer (enqueue_steps, enqueue_call, enqueue_pair, stage_lines, step_impl,
// refresh_status, scatter_points, delta_enqueue, reset_launch, arrival_pass) puts work on the handle's stream and keeps the handle's
// bookkeeping: such a function never waits for the work of the call (growing a buffer that enqueued kernels may read is the one wait:
// stage_lines, delta_enqueue) and never reads or writes `async` - what it needs to know it takes as an argument.  The CALL layer is the extern "C" entries: argument checks, one prologue (begin_call), enqueue-layer calls, one
// epilogue (finish_call: the wait of a synchronous call, timing, the team-error check).  A composite entry (sf_rollout, sf_run_delta,
// sf_agents_step, sf_step_mitigated) is made of enqueue-layer calls, never of other entries.
static int ensure_commit(sf_sim *s);
static int loop_stop(sf_sim *s);
static int comm_close(sf_sim *s);
static int destroy(sf_sim *s);
// every entry point except sf_loop_step ends the closed loop (sf_loop_start) first: the handle's stream is busy with the resident launch
#define LOOP_QUIESCE(s) do { if ((s)->loop_on) { int _rq = loop_stop(s); if (_rq) return _rq; } } while (0)
static int ensure_rm(sf_sim *s);
static int alloc_bl(sf_sim *s);
static bool prefers_bl(const sf_sim *s);
static int arrival_pass(sf_sim *s);
static int arrival_seg(const sf_sim *s, EnvSeg *seg, int n);
static int value_seg(const sf_sim *s, EnvSeg *seg, int n);
static int value_pass(sf_sim *s);
static int value_recount(sf_sim *s);
static int wind_forget(sf_sim *s, const int32_t *envs, int n);

// Behind every wait for the handle's stream: has a workgroup of a team launch (k_run<TEAM>) given up waiting for a team member?
// Then what the launch left behind is void - say so wherever data is handed back, not only in sf_sync / a synchronous sf_step.
// (A reset of every environment rewrites all the state a team launch touches and clears the word: the handle recovers.)
static int check_team_error(const sf_sim *s, const char *where)
{
    if (s->xerr_pinned && *s->xerr_pinned)
        return fail(SF_EHIP, "%s: a workgroup of a team launch (k_run<TEAM>) gave up waiting for a team member; the state of this handle is void until every environment is reset", where);
    return SF_OK;
}

// The prologue of a call (call layer): what the handle must have been given (SF_ESTATE before anything else happens), the device, the
// end of a closed loop, then - where asked for - the refusal of a handle a failed team launch has voided and the step rings folded
// into commit[] (after which tmp / flags carry nothing: the next launch starts from commit).
enum { kNeedRt = 1, kNeedReset = 2, kNotVoid = 4, kCommit = 8, kStateCall = kNeedReset | kNotVoid | kCommit };
static int check_ready(const sf_sim *s, const char *who, int need)
{
    if ((need & kNeedRt) && !s->have_rt) return fail(SF_ESTATE, "%s: call sf_set_layers or sf_set_rtable first", who);
    if ((need & kNeedReset) && !s->was_reset) return fail(SF_ESTATE, "%s: call sf_reset first", who);
    return SF_OK;
}
static int begin_call(sf_sim *s, const char *who, int need)
{
    { int rc = check_ready(s, who, need); if (rc) return rc; }
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    if (need & kNotVoid) { int rc = check_team_error(s, who); if (rc) return rc; }
    return (need & kCommit) ? ensure_commit(s) : SF_OK;
}
// The epilogue of a call: with `ms`, the GPU time between ev0 (recorded by the enqueue layer in front of the step launches) and here;
// the wait where the call waits (a timed call always does), and behind it the look at the team launches' error word - under the name
// `who`; without one (entries outside the step path that wait and have never looked) the wait alone.
static int finish_call(sf_sim *s, const char *who, bool wait, float *ms)
{
    if (ms) HIPCHK(hipEventRecord(s->ev1, s->stream));
    HIPCHK(hipGetLastError());
    if (!wait && !ms) return SF_OK;
    HIPCHK(hipStreamSynchronize(s->stream));
    if (ms) HIPCHK(hipEventElapsedTime(ms, s->ev0, s->ev1));
    return who ? check_team_error(s, who) : SF_OK;
}
// A look at the result of a single update (a status query, a delta query): what makes step(1) + look pairs a run(1) loop.
static void note_result_look(sf_sim *s)
{
    if (s->last_was_step1) { s->last_was_step1 = false; if (s->step1_polls < 1000) s->step1_polls++; }
}

// The environment list of a batched call: every entry names an environment of the handle and, where `twice` is given (the words of
// the refusal), none is named twice.  (n < 0 and null lists are the caller's to refuse: it knows what else must not be null.)
static int check_envs(const sf_sim *s, const char *who, int32_t n, const int32_t *envs, const char *twice = nullptr)
{
    std::vector<char> seen(twice ? (size_t)s->g.E : 0, 0);
    for (int i = 0; i < n; ++i) {
        const int e = envs[i];
        if (e < 0 || e >= s->g.E) return fail(SF_EINVAL, "%s: environment %d out of range", who, e);
        if (twice && seen[e]) return fail(SF_EINVAL, "%s: environment %d %s", who, e, twice);
        if (twice) seen[e] = 1;
    }
    return SF_OK;
}

static int ensure_stage(sf_sim *s, size_t bytes)
{
    if (bytes <= s->stage_bytes) return SF_OK;
    if (s->stage) HIPCHK(hipFree(s->stage));
    s->stage = nullptr; s->stage_bytes = 0;
    HIPCHK(hipMalloc(&s->stage, bytes));
    s->stage_bytes = bytes;
    return SF_OK;
}

template <typename T>
static int dev_alloc(sf_sim *s, T **p, size_t n)
{
    HIPCHK(hipMalloc(reinterpret_cast<void **>(p), n * sizeof(T)));
    s->bytes += (int64_t)(n * sizeof(T));
    return SF_OK;
}

// Room for `bytes` in a call block, its mirror free to be written: the last call's copy has left it.  Growing (to twice the request,
// 4 KB at least) waits for the stream first: enqueued kernels may still read the device buffer.
static int block_reserve(sf_sim *s, CallBlock &b, size_t bytes)
{
    if (!b.ev) HIPCHK(hipEventCreateWithFlags(&b.ev, hipEventDisableTiming));
    HIPCHK(hipEventSynchronize(b.ev));
    if (bytes <= b.cap) return SF_OK;
    HIPCHK(hipStreamSynchronize(s->stream));
    if (b.dev) { HIPCHK(hipFree(b.dev)); b.dev = nullptr; }
    if (b.pinned) { HIPCHK(hipHostFree(b.pinned)); b.pinned = nullptr; }
    b.cap = 0;
    const size_t cap = std::max<size_t>(bytes * 2, 4096);
    HIPCHK(hipMalloc(reinterpret_cast<void **>(&b.dev), cap));
    HIPCHK(hipHostMalloc(reinterpret_cast<void **>(&b.pinned), cap, hipHostMallocDefault));
    b.cap = cap;
    return SF_OK;
}
// The mirror's bytes [0, head) and, if any, [off, off + more) -> the device buffer on the handle's stream, then the event.
static int block_send(sf_sim *s, CallBlock &b, size_t head, size_t off = 0, size_t more = 0)
{
    HIPCHK(hipMemcpyAsync(b.dev, b.pinned, head, hipMemcpyHostToDevice, s->stream));
    if (more) HIPCHK(hipMemcpyAsync(b.dev + off, b.pinned + off, more, hipMemcpyHostToDevice, s->stream));
    HIPCHK(hipEventRecord(b.ev, s->stream));
    return SF_OK;
}

static void choose_rows_per_band(Geo &g, int rows)
{
    int rb = 1;
    while (rb * 2 <= rows && rb < 8) rb *= 2;    // the kernel is instantiated for 1, 2, 4, 8
    // per wave: list + sprite-mask tile [LR * RB + 2][LC * 16 + 16] + 16 + status tile [LR * RB][LC * 16]
    auto wave_bytes = [&](int r) { return kListCap * 2 + (g.LR * r + 2) * (g.LC * 16 + 16) + 16 + g.LR * r * g.LC * 16; };
    while (rb > 1 && wave_bytes(rb) > 40 * 1024) rb /= 2;
    g.RB = rb;
    g.lds_wave_bytes = (wave_bytes(rb) + 15) / 16 * 16;
    const int tile_h = kWaves * g.LR * g.RB;
    g.tiles_per_env = g.chunks_x * ((g.H + tile_h - 1) / tile_h);
    g.TX = g.chunks_x;
    g.TY = (g.H + g.LR * g.RB - 1) / (g.LR * g.RB);
    g.TXp = g.TX + 2;
    g.TYp = g.TY + 2;
}

extern "C" int sf_create(const sf_params *p, sf_sim **out)
{
    if (!p || !out) return fail(SF_EINVAL, "sf_create: null argument");
    if (p->n_envs < 1 || p->height < 1 || p->width < 1)
        return fail(SF_EINVAL, "sf_create: n_envs, height and width must be >= 1 (got %d, %d, %d)", p->n_envs,
                    p->height, p->width);
    if (p->max_fire_duration < 1)
        return fail(SF_EINVAL, "sf_create: max_fire_duration must be >= 1 (got %d)", p->max_fire_duration);
    if (p->max_fire_duration > 28)
        return fail(SF_ENOTSUP, "sf_create: max_fire_duration %d > 28 does not fit the 32-bit sprite-mask plane",
                    p->max_fire_duration);
    if (!(p->update_rate > 0.0)) return fail(SF_EINVAL, "sf_create: update_rate must be > 0");
    const long long P = ((long long)p->width + 15) / 16 * 16;
    if ((long long)p->height * P > (1ll << 26))
        return fail(SF_ENOTSUP, "sf_create: grids above 2^26 cells per environment are not supported");
    if (p->height > 65535 || p->n_envs > 65535)
        return fail(SF_ENOTSUP, "sf_create: more than 65535 rows or environments are not supported (launch grid limits)");
    HIPCHK(hipSetDevice(p->device));
    sf_sim *s = new sf_sim();
    s->p = *p;
    Geo &g = s->g;
    g.E = p->n_envs; g.H = p->height; g.W = p->width; g.P = (int)P; g.PV = g.P / 16;
    // lanes across a wave tile: 4 x 16 = 64 cells wide for large grids, so that a wave tile is
    // 64 x (16 * RB) cells = 64 x 64 at RB = 4 - square tiles minimise the number of tiles a fire
    // front crosses (measured on C3: 64 x 64 beats 128 x 32 by 8 % and 256 x 16 by 25 %)
    g.LC = 1; g.logLC = 0;
    while (g.LC < g.PV && g.LC < 4) { g.LC <<= 1; g.logLC++; }      // narrower tiles only on grids of one chunk (no seams)
    g.LR = 64 / g.LC;
    g.chunks_x = (g.PV + g.LC - 1) / g.LC;
    g.dense = 0;
    for (int i = 0; i < SF_TUNE_COUNT; ++i) { s->tune.v[i] = kTuneDefault[i]; s->tune.set[i] = false; }
    g.md = p->max_fire_duration; g.N = g.md + 3;
    g.ab = g.N <= 8 ? 1 : (g.N <= 16 ? 2 : 4);
    g.rt_env = p->per_env_terrain ? (long long)8 * g.H * P : 0;   // 1-byte plane: SWAR kernels; wider: generic per-cell kernel
    g.diag = p->diagonal_spread != 0; g.att = p->attenuate_line_ros != 0; g.has_max_time = p->has_max_time != 0;
    g.pixel_scale = p->pixel_scale; g.update_rate = p->update_rate; g.max_time = p->max_time;
    s->slope_scale = p->pixel_scale;
    g.prune_after_quit = 0;
    g.age_env = (long long)(g.H + 2) * g.P; g.plane_env = (long long)g.H * g.P;
    // rows per lane band: 2, i.e. wave tiles of 64 x 32 cells.  Measured on C3 / C4 / C5 once a wave needed
    // only 5.5 KB of LDS: shorter per-tile latency chains beat the fewer, larger 64 x 64 tiles by 6 / 14 / 17 %
    // (a step lasts as long as its slowest wave); 64 x 16 loses again to the halo overhead.
    int rb = 2;
    choose_rows_per_band(g, rb);

    int rc;
#define TRY(x) do { rc = (x); if (rc != SF_OK) { destroy(s); return rc; } } while (0)
#define TRYHIP(x) do { hipError_t _e = (x); if (_e != hipSuccess) { destroy(s); return fail(SF_EHIP, "%s failed: %s", #x, hipGetErrorString(_e)); } } while (0)
    if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess) { delete s; return fail(SF_EHIP, "hipStreamCreate failed"); }
    TRYHIP(hipEventCreate(&s->ev0)); TRYHIP(hipEventCreate(&s->ev1));
    for (int i = 0; i < sf_sim::kPtsRing; ++i) TRYHIP(hipEventCreate(&s->ev_pts[i]));
    const size_t cells = (size_t)g.E * g.plane_env;
    TRY(dev_alloc(s, &s->status, cells));
    TRY(dev_alloc(s, &s->age_alloc, ((size_t)g.E * g.age_env + 2 * (size_t)g.P) * g.ab));
    s->age = s->age_alloc + (size_t)g.P * g.ab;   // row 0 of env 0; guard rows at -1 and H of every env
    TRY(dev_alloc(s, &s->burn, cells));
    TRY(dev_alloc(s, &s->rt, (size_t)8 * g.plane_env * (p->per_env_terrain ? g.E : 1)));
    s->rt_set.assign(p->per_env_terrain ? g.E : 1, 0);
    s->rd_lay.assign(s->rt_set.size(), 0); s->rd_fbfm.assign(s->rt_set.size(), 0); s->rd_stale.assign(s->rt_set.size(), 1);
    TRY(dev_alloc(s, &s->lay_all, (size_t)7 * g.H * g.W * (p->per_env_terrain ? g.E : 1)));
    TRY(dev_alloc(s, &s->smag, (size_t)g.H * g.W));
    TRY(dev_alloc(s, &s->sdir, (size_t)g.H * g.W));
    TRY(dev_alloc(s, &s->commit, (size_t)g.E));
    TRY(dev_alloc(s, &s->tmp, (size_t)2 * g.E));
    TRY(dev_alloc(s, &s->flags, (size_t)3 * g.E));
    TRY(dev_alloc(s, &s->counters, (size_t)kCounterShards * kCounterRow));
    s->tflags_bytes = (size_t)2 * g.E * ((size_t)(g.H + g.LR - 1) / g.LR + 2) * (g.chunks_x + 2) + 64;
    TRY(dev_alloc(s, &s->tflags, s->tflags_bytes));
    // + 64: every wave of k_step requests its first list entry before it knows the list length
    TRY(dev_alloc(s, &s->tile_list, (size_t)g.E * ((size_t)(g.H + g.LR - 1) / g.LR) * g.chunks_x + 64));
    TRY(dev_alloc(s, &s->n_active, (size_t)16));
    g.Hs = (g.H + 512 + 2 * kSeamPad + 7) / 8 * 8;      // a tile may reach up to 512 rows past H
    g.seam_env = (long long)(g.chunks_x + 1) * 2 * g.Hs;
    TRY(dev_alloc(s, &s->seam, (size_t)g.E * g.seam_env));
    if (g.att) TRY(dev_alloc(s, &s->settled, cells));
    g.VW = (g.PV + 63) / 64; g.vb_env = (long long)g.H * g.VW;
    g.cells_env = (long long)((g.H + 3) / 4 + 2) * g.PV * 128;
    TRY(dev_alloc(s, &s->vbits, (size_t)3 * g.E * g.vb_env));
    TRY(dev_alloc(s, &s->todo, (size_t)g.E));
    TRY(dev_alloc(s, &s->run_cost, (size_t)g.E));
    TRY(dev_alloc(s, &s->run_order, (size_t)g.E));
    TRY(dev_alloc(s, &s->win_hint, (size_t)g.E));
    TRYHIP(hipMemsetAsync(s->run_cost, 0, (size_t)g.E * sizeof(uint32_t), s->stream));
    TRYHIP(hipMemsetAsync(s->win_hint, 0, (size_t)g.E * sizeof(unsigned long long), s->stream));
    TRYHIP(hipMemsetAsync(s->todo, 0, (size_t)g.E * sizeof(int32_t), s->stream));
    s->n_tiles_max = (size_t)g.E * ((size_t)(g.H + g.LR - 1) / g.LR) * g.chunks_x;      // RB = 1 is the finest tiling
    TRY(dev_alloc(s, &s->tdirty, s->n_tiles_max));
    TRY(dev_alloc(s, &s->thist, s->n_tiles_max * 8));
    { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, p->device) == hipSuccess) s->n_cu = prop.multiProcessorCount; }
    TRY(dev_alloc(s, &s->status_block, (size_t)8 * g.E));
    TRY(dev_alloc(s, &s->elapsed_dev, (size_t)g.E));
    TRYHIP(hipMemsetAsync(s->flags, 0, sizeof(uint32_t) * 3 * g.E, s->stream));
    TRYHIP(hipMemsetAsync(s->tflags, 0, s->tflags_bytes, s->stream));
    TRYHIP(hipMemsetAsync(s->n_active, 0, 16 * sizeof(uint32_t), s->stream));
    TRYHIP(hipMemsetAsync(s->seam, 0, (size_t)g.E * g.seam_env, s->stream));
    TRYHIP(hipMemsetAsync(s->vbits, 0, (size_t)3 * g.E * g.vb_env * sizeof(unsigned long long), s->stream));
    if (s->settled) TRYHIP(hipMemsetAsync(s->settled, 0, cells * sizeof(uint32_t), s->stream));
    TRYHIP(hipMemsetAsync(s->counters, 0, sizeof(unsigned long long) * kCounterShards * kCounterRow, s->stream));
    TRYHIP(hipMemsetAsync(s->commit, 0, sizeof(EnvState) * g.E, s->stream));
    TRYHIP(hipMemsetAsync(s->age_alloc, 0, ((size_t)g.E * g.age_env + 2 * (size_t)g.P) * g.ab, s->stream));
    TRYHIP(hipMemsetAsync(s->status, 0, cells, s->stream));
    TRYHIP(hipMemsetAsync(s->burn, 0, cells * sizeof(double), s->stream));
    TRYHIP(hipStreamSynchronize(s->stream));
#undef TRY
#undef TRYHIP
    *out = s;
    return SF_OK;
}

extern "C" int sf_destroy(sf_sim *s) { return destroy(s); }
static int destroy(sf_sim *s)
{
    if (!s) return SF_OK;
    hipSetDevice(s->p.device);
    if (s->loop_on) (void)loop_stop(s);
    if (s->stream) hipStreamSynchronize(s->stream);
    (void)comm_close(s);
    if (s->xerr_pinned) (void)hipHostFree(s->xerr_pinned);
    for (void *hp : {(void *)s->loop_db, (void *)s->loop_res, (void *)s->loop_pts}) if (hp) (void)hipHostFree(hp);
    for (void *dp : {(void *)s->loop_mem, (void *)s->loop_pts_mem}) if (dp) (void)hipFree(dp);
    void *ptrs[] = {s->team_tab, s->team_size, s->xdone, s->xg, s->xbuf, s->xj, s->xcut, s->jlog, s->status, s->age_alloc, s->cells_alloc, s->burn, s->rt, s->rtc, s->lay_all, s->history, s->smag, s->sdir, s->commit, s->tmp, s->flags, s->counters, s->tflags, s->tile_list, s->n_active, s->seam, s->settled, s->tdirty, s->thist, s->vbits, s->todo, s->run_cost, s->run_order, s->todo_cnt, s->win_hint, s->mit_stage,
                    s->status_block, s->elapsed_dev, s->stage, s->parents, s->arrival1, s->val_plane, s->val_aux, s->wterms, s->wsched, s->wdue, s->wdue_U};
    if (s->status_pinned) (void)hipHostFree(s->status_pinned);
    if (s->delta_pinned) (void)hipHostFree(s->delta_pinned);
    for (void *dp : {(void *)s->snap, (void *)s->delta_dev, (void *)s->rd_bg, (void *)s->rd_fuel_ix, (void *)s->ag_mem, (void *)s->ep_mem}) if (dp) (void)hipFree(dp);
    for (CallBlock *b : {&s->obs_blk, &s->rd_blk, &s->rs_blk, &s->gen_blk, &s->ag_blk, &s->wind_blk, &s->ens_blk}) {
        if (b->dev) (void)hipFree(b->dev);
        if (b->pinned) (void)hipHostFree(b->pinned);
        if (b->ev) (void)hipEventDestroy(b->ev);
    }
    for (int i = 0; i < sf_sim::kPtsRing; ++i) {
        if (s->pts_pinned[i]) (void)hipHostFree(s->pts_pinned[i]);
        if (s->ev_pts[i]) (void)hipEventDestroy(s->ev_pts[i]);
    }
    for (void *p : ptrs) if (p) hipFree(p);
    if (s->ev0) hipEventDestroy(s->ev0);
    if (s->ev1) hipEventDestroy(s->ev1);
    if (s->stream) hipStreamDestroy(s->stream);
    delete s;
    return SF_OK;
}

extern "C" int sf_get_geometry(sf_sim *s, int32_t *out)
{
    if (!s || !out) return fail(SF_EINVAL, "sf_get_geometry: null argument");
    const Geo &g = s->g;
    out[0] = g.LC * 16; out[1] = g.LR * g.RB; out[2] = g.TX; out[3] = g.TY; out[4] = g.RB; out[5] = g.P;
    out[6] = g.lds_wave_bytes; out[7] = g.dense;
    return SF_OK;
}

extern "C" int sf_memory_bytes(sf_sim *s, int64_t *bytes)
{
    if (!s || !bytes) return fail(SF_EINVAL, "sf_memory_bytes: null argument");
    *bytes = s->bytes + (int64_t)s->stage_bytes;
    return SF_OK;
}

static int rebuild_tflags(sf_sim *s, int env0, int n)
{
    const Geo &g = s->g;
    hipLaunchKernelGGL(k_rebuild_tflags, dim3(g.TX, g.TY, n), dim3(64), 0, s->stream, g, (const uint8_t *)s->status,
                       (const uint8_t *)s->age, s->tflags, s->ring, env0);
    HIPCHK(hipGetLastError());
    return SF_OK;
}

static int rebuild_seams(sf_sim *s, int env0, int n)
{
    const Geo &g = s->g;
    if (g.ab != 1) return SF_OK;       // wider sprite planes always run in the per-cell kernel
    hipLaunchKernelGGL(k_rebuild_seams, dim3((g.Hs + 255) / 256, (g.chunks_x + 1) * 2, n), dim3(256), 0, s->stream, g,
                       (const uint8_t *)s->age, s->seam, env0);
    HIPCHK(hipGetLastError());
    return SF_OK;
}

extern "C" int sf_set_rows_per_band(sf_sim *s, int32_t rows)
{
    if (!s || rows < 1 || rows > 4096) return fail(SF_EINVAL, "sf_set_rows_per_band: rows must be in [1, 4096]");
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    { int rc0 = ensure_commit(s); if (rc0) return rc0; }     // also clears the list counters of the tiled path
    choose_rows_per_band(s->g, rows);
    s->status_fresh = false;
    s->tdirty_all = true;
    s->tiles_valid = false;            // the tile activity map is laid out per wave tile: rebuilt for the new geometry before the next tiled step
    return SF_OK;
}

/* RothermelFireManager.pixel_scale is a plain attribute that the reference's own test overwrites
 * after construction (test_fire.py:334): only the ignition threshold changes, the slopes keep the
 * value used at construction (fire.py:377, 568). */
extern "C" int sf_set_threshold(sf_sim *s, double pixel_scale)
{
    if (!s) return fail(SF_EINVAL, "sf_set_threshold: null handle");
    s->g.pixel_scale = pixel_scale;
    return SF_OK;
}

/* Asynchronous mode for rollout loops: sf_step / sf_apply_mitigation enqueue their work on the
 * handle's stream and return; every call that hands data back (sf_get_*, sf_step_timed,
 * sf_copy_status_to, sf_sync) synchronises. */
extern "C" int sf_set_async(sf_sim *s, int32_t on)
{
    if (!s) return fail(SF_EINVAL, "sf_set_async: null handle");
    s->async = on != 0;
    return SF_OK;
}
/* 1 = environments that QUIT on the runtime check keep pruning / ageing their sprites when sf_step is called again,
 * like RothermelFireManager.update does on every call after that QUIT (fire.py:631-643); 0 (default) = frozen. */
extern "C" int sf_set_prune_after_quit(sf_sim *s, int32_t on)
{
    if (!s) return fail(SF_EINVAL, "sf_set_prune_after_quit: null handle");
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    { int rc0 = ensure_commit(s); if (rc0) return rc0; }
    s->g.prune_after_quit = on != 0;
    return SF_OK;
}
extern "C" int sf_sync(sf_sim *s)
{
    if (!s) return fail(SF_EINVAL, "sf_sync: null handle");
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    return finish_call(s, "sf_sync", true, nullptr);
}

/* Spread graph (FireSpreadGraph, simfire/utils/graph.py): record for every ignition which of the 8
 * neighbours were BURNING at that moment.  Off by default (one more small launch per step and one
 * more byte per cell). */
extern "C" int sf_enable_spread_graph(sf_sim *s, int32_t on)
{
    if (!s) return fail(SF_EINVAL, "sf_enable_spread_graph: null handle");
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    if (on && !s->parents) {
        const size_t n = (size_t)s->g.E * s->g.plane_env;
        HIPCHK(hipMalloc(reinterpret_cast<void **>(&s->parents), n));
        s->bytes += (int64_t)n;
        HIPCHK(hipMemsetAsync(s->parents, 0, n, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));
    }
    s->graph_on = on != 0;
    return SF_OK;
}

extern "C" int sf_get_spread_parents(sf_sim *s, int32_t env, uint8_t *out)
{
    if (!s || !out) return fail(SF_EINVAL, "sf_get_spread_parents: null argument");
    const Geo &g = s->g;
    if (env < 0 || env >= g.E) return fail(SF_EINVAL, "sf_get_spread_parents: environment %d out of range", env);
    if (!s->parents) return fail(SF_ESTATE, "sf_get_spread_parents: call sf_enable_spread_graph first");
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    HIPCHK(hipMemcpy2DAsync(out, (size_t)g.W, s->parents + (size_t)env * g.plane_env, (size_t)g.P, (size_t)g.W,
                            (size_t)g.H, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return SF_OK;
}

/* 1 = step with the generic per-cell kernel (always used when max_fire_duration > 5); switching
 * back to the tiled kernels rebuilds their tile activity map from the cell planes. */
extern "C" int sf_set_generic(sf_sim *s, int32_t on)
{
    if (!s) return fail(SF_EINVAL, "sf_set_generic: null handle");
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    { int rc0 = ensure_commit(s); if (rc0) return rc0; }     // the list counters of the tiled path restart clean
    s->generic = on != 0;
    s->tdirty_all = true;
    return SF_OK;
}

/* -1 = choose by problem size (default), 0 = always k_select + k_step, 1 = always one fused launch per step,
 * 2 = one environment-resident launch per sf_step call (k_run) whenever the handle's options allow it */
extern "C" int sf_set_fused(sf_sim *s, int32_t mode)
{
    if (!s || mode < -1 || mode > 2) return fail(SF_EINVAL, "sf_set_fused: mode must be -1 ... 2");
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    { int rc0 = ensure_commit(s); if (rc0) return rc0; }
    s->fused_mode = mode;
    return SF_OK;
}

extern "C" int sf_set_tuning(sf_sim *s, int32_t knob, int32_t value)
{
    if (!s || knob < 0 || knob >= SF_TUNE_COUNT) return fail(SF_EINVAL, "sf_set_tuning: unknown knob %d", knob);
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    { int rc0 = ensure_commit(s); if (rc0) return rc0; }
    s->tune.v[knob] = value;
    s->tune.set[knob] = true;
    return SF_OK;
}
extern "C" int sf_get_run_cost(sf_sim *s, uint32_t *out)
{
    if (!s || !out) return fail(SF_EINVAL, "sf_get_run_cost: null argument");
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(hipMemcpy(out, s->run_cost, (size_t)s->g.E * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return SF_OK;
}
extern "C" int sf_get_team_sizes(sf_sim *s, uint32_t *out)
{
    if (!s || !out) return fail(SF_EINVAL, "sf_get_team_sizes: null argument");
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    HIPCHK(hipStreamSynchronize(s->stream));
    if (!s->last_team_max || !s->team_size) { for (int e = 0; e < s->g.E; ++e) out[e] = 0; return SF_OK; }
    HIPCHK(hipMemcpy(out, s->team_size, (size_t)s->g.E * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return SF_OK;
}
extern "C" int sf_get_join_log(sf_sim *s, uint32_t *out, int32_t cap, int32_t *n_out)
{
    if (!s || !n_out || cap < 0 || (cap > 0 && !out)) return fail(SF_EINVAL, "sf_get_join_log: bad argument");
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    HIPCHK(hipStreamSynchronize(s->stream));
    *n_out = 0;
    if (!s->jlog || !s->jlog_valid) return SF_OK;
    uint32_t n = 0;
    HIPCHK(hipMemcpy(&n, s->jlog, sizeof n, hipMemcpyDeviceToHost));
    if (n > (uint32_t)kJoinLog) n = kJoinLog;
    if (n > (uint32_t)cap) n = (uint32_t)cap;
    if (n) HIPCHK(hipMemcpy(out, s->jlog + 1, (size_t)n * 3 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    *n_out = (int32_t)n;
    return SF_OK;
}
extern "C" int sf_get_last_launches(sf_sim *s, int32_t *out)
{
    if (!s || !out) return fail(SF_EINVAL, "sf_get_last_launches: null argument");
    *out = s->last_launches;
    return SF_OK;
}
extern "C" int sf_get_team_fallbacks(sf_sim *s, int32_t *out)
{
    if (!s || !out) return fail(SF_EINVAL, "sf_get_team_fallbacks: null argument");
    *out = 0;
    if (!s->xdone) return SF_OK;                   // (no team launch yet)
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    HIPCHK(hipStreamSynchronize(s->stream));
    uint32_t v = 0;
    HIPCHK(hipMemcpy(&v, s->xdone + (size_t)2 * s->g.E, sizeof v, hipMemcpyDeviceToHost));
    *out = (int32_t)v;
    return SF_OK;
}
extern "C" int sf_get_tuning(sf_sim *s, int32_t knob, int32_t *value)
{
    if (!s || !value || knob < 0 || knob >= SF_TUNE_COUNT) return fail(SF_EINVAL, "sf_get_tuning: unknown knob %d", knob);
    *value = s->tune.v[knob];
    return SF_OK;
}

/* 1 = visit every tile every step (cross-check of the tile activity map), 0 = default */
extern "C" int sf_set_dense(sf_sim *s, int32_t dense)
{
    if (!s) return fail(SF_EINVAL, "sf_set_dense: null handle");
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    { int rc0 = ensure_commit(s); if (rc0) return rc0; }
    s->g.dense = dense != 0;
    return SF_OK;
}

// which R tables an env argument addresses: env < 0 = all of them
static int table_range(sf_sim *s, int env, const char *who, int *lo, int *hi)
{
    const int n_tab = (int)s->rt_set.size();
    if (env < 0) { *lo = 0; *hi = n_tab; return SF_OK; }
    if (n_tab == 1) return fail(SF_ESTATE, "%s: this handle shares one terrain between all environments "
                                "(create it with per_env_terrain = 1)", who);
    if (env >= n_tab) return fail(SF_EINVAL, "%s: environment %d out of range", who, env);
    *lo = env; *hi = env + 1;
    return SF_OK;
}
// tables tabs[0 .. n) were replaced: only their cell-major copies are rebuilt (ensure_rtc)
static void mark_tables(sf_sim *s, const int32_t *tabs, int n)
{
    if (s->rtc_stale.size() != s->rt_set.size()) s->rtc_stale.assign(s->rt_set.size(), 1);
    for (int k = 0; k < n; ++k) s->rt_set[tabs[k]] = s->rtc_stale[tabs[k]] = 1;
    if (!s->wt_stale.empty()) for (int k = 0; k < n; ++k) s->wt_stale[tabs[k]] = 1;      // (the cache of wind-independent terms: ensure_wterms)
    s->wind_sched_ready = false;
    s->rtc_valid = false;
    s->have_rt = true;
    for (char c : s->rt_set) if (!c) s->have_rt = false;
}
static void mark_tables(sf_sim *s, int lo, int hi)
{
    std::vector<int32_t> tabs;
    for (int i = lo; i < hi; ++i) tabs.push_back(i);
    mark_tables(s, tabs.data(), hi - lo);
}

// theta = arctan2(src_y - dst_y, dst_x - src_x) of the 8 travel directions, float32 (rothermel.py:102)
static Thetas rt_thetas()
{
    Thetas th;
    for (int k = 0; k < 8; ++k) th.v[k] = atan2f((float)SF_SRC_DY[k], (float)(-SF_SRC_DX[k]));
    return th;
}

// src[i] == nullptr: plane i of table `lo` is already on the device (filled from a fuel-code raster)
static int set_layers_impl(sf_sim *s, int env, const double *const src[7])
{
    int lo, hi, rc = table_range(s, env, "sf_set_layers", &lo, &hi);
    if (rc) return rc;
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    const Geo &g = s->g;
    const size_t n = (size_t)g.H * g.W;
    for (int i = 0; i < 7; ++i)
        if (src[i]) HIPCHK(hipMemcpyAsync(s->layer(lo, i), src[i], n * sizeof(double), hipMemcpyHostToDevice, s->stream));
    dim3 blk(256), grd((g.W + 255) / 256, g.H);
    hipLaunchKernelGGL(k_slopes, grd, blk, 0, s->stream, g.H, g.W, s->layer(lo, 4), s->slope_scale, s->smag, s->sdir);
    const Thetas th = rt_thetas();
    dim3 grd2((g.P + 255) / 256, g.H);
    const size_t tab = (size_t)8 * g.plane_env;
    hipLaunchKernelGGL(k_rtable, grd2, blk, 0, s->stream, g.H, g.W, g.P, s->layer(lo, 0), s->layer(lo, 1), s->layer(lo, 2),
                       s->layer(lo, 3), s->layer(lo, 5), s->layer(lo, 6), s->smag, s->sdir, (float)s->p.h, (float)s->p.S_T,
                       (float)s->p.S_e, (float)s->p.p_p, (float)s->p.M_f, th, s->rt + (size_t)lo * tab);
    HIPCHK(hipGetLastError());
    for (int i = lo + 1; i < hi; ++i) {   // same terrain for several environments: replicate layers and table
        HIPCHK(hipMemcpyAsync(s->layer(i, 0), s->layer(lo, 0), 7 * n * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
        HIPCHK(hipMemcpyAsync(s->rt + (size_t)i * tab, s->rt + (size_t)lo * tab, tab * sizeof(double),
                              hipMemcpyDeviceToDevice, s->stream));
    }
    HIPCHK(hipStreamSynchronize(s->stream));
    mark_tables(s, lo, hi);
    for (int i = lo; i < hi; ++i) { s->rd_lay[i] = 1; s->rd_fbfm[i] = src[0] == nullptr; s->rd_stale[i] = 1; }
    if (s->wsched) {
        std::vector<int32_t> tabs;
        for (int i = lo; i < hi; ++i) tabs.push_back(i);
        rc = wind_forget(s, tabs.data(), hi - lo);
        if (!rc && !s->wind_sched.empty()) HIPCHK(hipStreamSynchronize(s->stream));
    }
    return rc;
}

extern "C" int sf_set_layers(sf_sim *s, const double *w_0, const double *delta, const double *M_x,
                             const double *sigma, const double *elevation, const double *U, const double *U_dir)
{
    if (!s) return fail(SF_EINVAL, "sf_set_layers: null handle");
    const double *src[7] = {w_0, delta, M_x, sigma, elevation, U, U_dir};
    return set_layers_impl(s, -1, src);
}

extern "C" int sf_set_layers_env(sf_sim *s, int32_t env, const double *w_0, const double *delta, const double *M_x,
                                 const double *sigma, const double *elevation, const double *U, const double *U_dir)
{
    if (!s) return fail(SF_EINVAL, "sf_set_layers_env: null handle");
    if (env < 0) return fail(SF_EINVAL, "sf_set_layers_env: environment %d out of range", env);
    const double *src[7] = {w_0, delta, M_x, sigma, elevation, U, U_dir};
    return set_layers_impl(s, env, src);
}

// FuelLayer._get_data (simfire/utils/layers.py:670-676): FBFM13 code raster -> Fuel through the
// FuelModelToFuel table (simfire/enums.py:176-198), done on the device.  The table is the caller's.
extern "C" int sf_set_layers_fbfm(sf_sim *s, int32_t env, const int32_t *codes, int32_t n_lut, const int32_t *lut_codes,
                                  const double *lut_fuel, const double *elevation, const double *U, const double *U_dir)
{
    if (!s || !codes || !lut_codes || !lut_fuel || !elevation || !U || !U_dir)
        return fail(SF_EINVAL, "sf_set_layers_fbfm: null argument");
    if (n_lut < 1 || n_lut > kMaxFuelLut) return fail(SF_EINVAL, "sf_set_layers_fbfm: n_lut must be 1..%d", kMaxFuelLut);
    int lo, hi, rc = table_range(s, env, "sf_set_layers_fbfm", &lo, &hi);
    if (rc) return rc;
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    const Geo &g = s->g;
    const size_t n = (size_t)g.H * g.W;
    rc = ensure_stage(s, n * sizeof(int32_t) + (1 + kRdFbfmColours) * sizeof(int32_t));      // codes | bad | sf_render's colour codes
    if (rc) return rc;
    int32_t *codes_dev = (int32_t *)s->stage, *bad_dev = codes_dev + n;
    HIPCHK(hipMemcpyAsync(codes_dev, codes, n * sizeof(int32_t), hipMemcpyHostToDevice, s->stream));
    const int32_t none = INT32_MIN;
    HIPCHK(hipMemcpyAsync(bad_dev, &none, sizeof none, hipMemcpyHostToDevice, s->stream));
    FuelLut lut;
    lut.n = n_lut;
    for (int i = 0; i < n_lut; ++i) {
        lut.code[i] = lut_codes[i];
        for (int k = 0; k < 4; ++k) lut.fuel[i][k] = lut_fuel[4 * i + k];
    }
    hipLaunchKernelGGL(k_fuel_lut, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, (long long)n,
                       (const int32_t *)codes_dev, lut, s->layer(lo, 0), s->layer(lo, 1), s->layer(lo, 2), s->layer(lo, 3), bad_dev);
    HIPCHK(hipGetLastError());
    int32_t bad = none;
    HIPCHK(hipMemcpyAsync(&bad, bad_dev, sizeof bad, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    if (bad != none) return fail(SF_EINVAL, "sf_set_layers_fbfm: fuel model code %d is not in the table", bad);
    // the codes' colours for sf_render (FuelLayer._make_image, layers.py:654-667): the codes are dropped after the lookup above
    if (!s->rd_fuel_ix) HIPCHK(hipMalloc(reinterpret_cast<void **>(&s->rd_fuel_ix), n * s->rt_set.size()));
    int32_t *tab_dev = bad_dev + 1;
    HIPCHK(hipMemcpyAsync(tab_dev, kRdFbfmCodes, sizeof kRdFbfmCodes, hipMemcpyHostToDevice, s->stream));
    hipLaunchKernelGGL(k_render_fuel_ix, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, (long long)n, (const int32_t *)codes_dev,
                       (const int32_t *)tab_dev, kRdFbfmColours, s->rd_fuel_ix + (size_t)lo * n);
    HIPCHK(hipGetLastError());
    for (int i = lo + 1; i < hi; ++i)
        HIPCHK(hipMemcpyAsync(s->rd_fuel_ix + (size_t)i * n, s->rd_fuel_ix + (size_t)lo * n, n, hipMemcpyDeviceToDevice, s->stream));
    const double *src[7] = {nullptr, nullptr, nullptr, nullptr, elevation, U, U_dir};
    return set_layers_impl(s, env, src);
}

// FireSimulation.get_attribute_data (simfire/sim/simulation.py:376-403): w_0 / delta / M_x as float32,
// sigma as uint32 (astype truncation), elevation and wind as supplied (float64).  Null pointers are
// skipped; device_pointers != 0: the outputs are device buffers (observation tensors stay in HBM).
extern "C" int sf_get_attribute_data(sf_sim *s, int32_t env, float *w_0, uint32_t *sigma, float *delta, float *M_x,
                                     double *elevation, double *wind_speed, double *wind_direction, int32_t device_pointers)
{
    if (!s) return fail(SF_EINVAL, "sf_get_attribute_data: null handle");
    const int n_tab = (int)s->rt_set.size();
    if (env < 0 || env >= s->g.E) return fail(SF_EINVAL, "sf_get_attribute_data: environment %d out of range", env);
    const int t = n_tab == 1 ? 0 : env;
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    const Geo &g = s->g;
    const size_t n = (size_t)g.H * g.W;
    const hipMemcpyKind kind = device_pointers ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (w_0 || sigma || delta || M_x) {
        int rc = ensure_stage(s, 4 * n * sizeof(float));
        if (rc) return rc;
        float *st = (float *)s->stage;
        float *d_w0 = device_pointers && w_0 ? w_0 : st, *d_de = device_pointers && delta ? delta : st + 2 * n,
              *d_mx = device_pointers && M_x ? M_x : st + 3 * n;
        uint32_t *d_si = device_pointers && sigma ? sigma : (uint32_t *)(st + n);
        hipLaunchKernelGGL(k_attribute_planes, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, (long long)n,
                           (const double *)s->layer(t, 0), (const double *)s->layer(t, 1), (const double *)s->layer(t, 2),
                           (const double *)s->layer(t, 3), d_w0, d_si, d_de, d_mx);
        HIPCHK(hipGetLastError());
        if (!device_pointers) {
            if (w_0) HIPCHK(hipMemcpyAsync(w_0, st, n * 4, kind, s->stream));
            if (sigma) HIPCHK(hipMemcpyAsync(sigma, st + n, n * 4, kind, s->stream));
            if (delta) HIPCHK(hipMemcpyAsync(delta, st + 2 * n, n * 4, kind, s->stream));
            if (M_x) HIPCHK(hipMemcpyAsync(M_x, st + 3 * n, n * 4, kind, s->stream));
        }
    }
    if (elevation) HIPCHK(hipMemcpyAsync(elevation, s->layer(t, 4), n * sizeof(double), kind, s->stream));
    if (wind_speed) HIPCHK(hipMemcpyAsync(wind_speed, s->layer(t, 5), n * sizeof(double), kind, s->stream));
    if (wind_direction) HIPCHK(hipMemcpyAsync(wind_direction, s->layer(t, 6), n * sizeof(double), kind, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return SF_OK;
}

// sf_generate_layers (include/simfire_hip.h; sf_gen_kernels.h): every argument is checked before any device work
static int check_noise(const sf_noise &p, int e, const char *plane)
{
    if (p.kind == SF_GEN_NONE || p.kind == SF_GEN_CONSTANT) return SF_OK;
    if (p.kind != SF_GEN_SIMPLEX) return fail(SF_EINVAL, "sf_generate_layers: environment %d, %s: unknown kind %d", e, plane, p.kind);
    if (!(p.scale > 0.0)) return fail(SF_EINVAL, "sf_generate_layers: environment %d, %s: scale must be > 0", e, plane);
    if (p.octaves < 1 || p.octaves > kGenMaxOctaves)
        return fail(SF_EINVAL, "sf_generate_layers: environment %d, %s: octaves must be 1..%d", e, plane, kGenMaxOctaves);
    if (!(p.lo < p.hi)) return fail(SF_EINVAL, "sf_generate_layers: environment %d, %s: range_min must be less than range_max", e, plane);
    return SF_OK;
}

extern "C" int sf_generate_layers(sf_sim *s, int32_t n, const int32_t *envs, const sf_layer_gen *gen)
{
    if (!s) return fail(SF_EINVAL, "sf_generate_layers: null handle");
    if (n < 0) return fail(SF_EINVAL, "sf_generate_layers: n = %d", n);
    if (n > 0 && (!envs || !gen)) return fail(SF_EINVAL, "sf_generate_layers: null argument");
    if (!s->p.per_env_terrain)
        return fail(SF_ESTATE, "sf_generate_layers: this handle shares one terrain between all environments (create it with per_env_terrain = 1)");
    const Geo &g = s->g;
    { int rc = check_envs(s, "sf_generate_layers", n, envs, "listed twice"); if (rc) return rc; }
    for (int k = 0; k < n; ++k) {
        const int e = envs[k];
        const sf_layer_gen &d = gen[k];
        int rc = check_noise(d.elevation, e, "elevation");
        if (!rc) rc = check_noise(d.wind_speed, e, "wind_speed");
        if (!rc) rc = check_noise(d.wind_direction, e, "wind_direction");
        if (rc) return rc;
        if (d.fuel != SF_GEN_NONE && d.fuel != SF_GEN_CONSTANT)
            return fail(SF_EINVAL, "sf_generate_layers: environment %d, fuel: unknown kind %d", e, d.fuel);
    }
    if (n == 0) return SF_OK;
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    const size_t gen_bytes = (size_t)n * sizeof(sf_layer_gen), bytes = gen_bytes + (size_t)n * sizeof(int32_t);
    CallBlock &blk = s->gen_blk;
    { int rc = block_reserve(s, blk, bytes); if (rc) return rc; }
    memcpy(blk.pinned, gen, gen_bytes);
    memcpy(blk.pinned + gen_bytes, envs, (size_t)n * sizeof(int32_t));
    { int rc = block_send(s, blk, bytes); if (rc) return rc; }
    const sf_layer_gen *gen_d = (const sf_layer_gen *)blk.dev;
    const int32_t *envs_d = (const int32_t *)(blk.dev + gen_bytes);
    const long long cells = (long long)g.H * g.W;
    const Thetas th = rt_thetas();
    for (int k0 = 0; k0 < n; k0 += kGenChunk) {          // (grid y / z hold at most kGenChunk environments)
        const int m = std::min(n - k0, kGenChunk);
        hipLaunchKernelGGL(k_gen_planes, dim3((unsigned)((cells + kGenThreads - 1) / kGenThreads), (unsigned)m, 4), dim3(kGenThreads), 0,
                           s->stream, g.H, g.W, s->lay_all, envs_d, gen_d, k0);
        HIPCHK(hipGetLastError());
    }
    for (int k0 = 0; k0 < n; k0 += kGenChunk) {
        const int m = std::min(n - k0, kGenChunk);
        hipLaunchKernelGGL(k_gen_rtable, dim3((unsigned)((g.P + kGenThreads - 1) / kGenThreads), (unsigned)g.H, (unsigned)m), dim3(kGenThreads), 0,
                           s->stream, g.H, g.W, g.P, (const double *)s->lay_all, envs_d, k0, s->slope_scale, (float)s->p.h, (float)s->p.S_T,
                           (float)s->p.S_e, (float)s->p.p_p, (float)s->p.M_f, th, s->rt, (long long)8 * g.plane_env);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(s->stream));
    mark_tables(s, envs, n);
    for (int k = 0; k < n; ++k) { s->rd_lay[envs[k]] = 1; s->rd_fbfm[envs[k]] = 0; s->rd_stale[envs[k]] = 1; }
    return wind_forget(s, envs, n);
}

// ----------------------------------------------------------------------------- wind changes
// The wind-independent terms of the listed tables (host list) made current in the cache plane, modelled on ensure_rtc: allocated at
// the first wind change, filled per run of stale tables.  SF_ENOTSUP: no cache (no memory for it, or switched off by the lab) - the
// caller builds from the layers.
static int ensure_wterms(sf_sim *s, const int32_t *tabs, int n)
{
    if (s->wt_off) return SF_ENOTSUP;
    const Geo &g = s->g;
    const size_t n_tab = s->rt_set.size(), per = (size_t)kWindPlanes * g.H * g.W;
    if (!s->wterms) {
        if (hipMalloc(reinterpret_cast<void **>(&s->wterms), per * n_tab * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); s->wterms = nullptr; return SF_ENOTSUP; }
        s->bytes += (int64_t)(per * n_tab * sizeof(float));
        s->wt_stale.assign(n_tab, 1);
    }
    std::vector<int32_t> stale;
    for (int k = 0; k < n; ++k) if (s->wt_stale[tabs[k]]) stale.push_back(tabs[k]);
    std::sort(stale.begin(), stale.end());
    const Thetas th = rt_thetas();
    for (size_t i = 0; i < stale.size();) {
        size_t j = i + 1;
        while (j < stale.size() && stale[j] == stale[j - 1] + 1 && j - i < 65535) ++j;
        hipLaunchKernelGGL(k_wind_terms, dim3((unsigned)((g.W + kWindThreads - 1) / kWindThreads), (unsigned)g.H, (unsigned)(j - i)), dim3(kWindThreads), 0,
                           s->stream, g.H, g.W, (const double *)s->lay_all, (const int32_t *)nullptr, (int)stale[i], s->slope_scale, (float)s->p.h,
                           (float)s->p.S_T, (float)s->p.S_e, (float)s->p.p_p, (float)s->p.M_f, th, s->wterms);
        for (size_t k = i; k < j; ++k) s->wt_stale[stale[k]] = 0;
        i = j;
    }
    HIPCHK(hipGetLastError());
    return SF_OK;
}

// k_wind_rtable for `count` listed tables, or - cnt_dev - for as many as the device says (at most max_count); enqueue layer
static int wind_launch(sf_sim *s, const int32_t *list_dev, const uint32_t *cnt_dev, int count, int max_count, const double *U, const double *U_dir,
                       int field, bool cached)
{
    const Geo &g = s->g;
    WindArgs a;
    a.H = g.H; a.W = g.W; a.P = g.P;
    a.lay = s->lay_all; a.cache = s->wterms; a.rt = s->rt; a.rtc = s->rtc;
    a.tab_stride = (long long)8 * g.plane_env;
    a.list = list_dev; a.count_dev = cnt_dev; a.count = count;
    a.U = U; a.U_dir = U_dir; a.field = field;
    a.ps = s->slope_scale;
    a.h = (float)s->p.h; a.S_T = (float)s->p.S_T; a.S_e = (float)s->p.S_e; a.p_p = (float)s->p.p_p; a.M_f = (float)s->p.M_f;
    a.th = rt_thetas();
    const long long items = (long long)max_count * g.H * ((g.P + kWindThreads - 1) / kWindThreads);
    const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>(items, (long long)s->n_cu * 8));
    if (cached) hipLaunchKernelGGL(k_wind_rtable<true>, dim3(grid), dim3(kWindThreads), 0, s->stream, a);
    else hipLaunchKernelGGL(k_wind_rtable<false>, dim3(grid), dim3(kWindThreads), 0, s->stream, a);
    HIPCHK(hipGetLastError());
    return SF_OK;
}

static void wind_sched_count(sf_sim *s)
{
    s->wind_sched.clear();
    for (int e = 0; e < (int)s->wind_K.size(); ++e) if (s->wind_K[e]) s->wind_sched.push_back(e);
    s->wind_sched_ready = false;
}

// An environment list -> the wind call block (enqueue layer); *dev: where it is
static int wind_list(sf_sim *s, const int32_t *envs, int n, const int32_t **dev)
{
    CallBlock &blk = s->wind_blk;
    { int rc = block_reserve(s, blk, (size_t)n * 4); if (rc) return rc; }
    memcpy(blk.pinned, envs, (size_t)n * 4);
    *dev = (const int32_t *)blk.dev;
    return block_send(s, blk, (size_t)n * 4);
}

// The tables of these environments were rebuilt from their layers (or their state was loaded): whichever segment a schedule built
// them for, the next stepping call decides anew.
static int wind_forget(sf_sim *s, const int32_t *envs, int n)
{
    bool any = false;
    for (int k = 0; k < n && !any; ++k) any = s->wsched && s->wind_K[envs[k]] != 0;
    if (!any) return SF_OK;
    const int32_t *list_dev = nullptr;
    { int rc = wind_list(s, envs, n, &list_dev); if (rc) return rc; }
    hipLaunchKernelGGL(k_wind_sched_forget, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, n, list_dev, s->wsched);
    HIPCHK(hipGetLastError());
    return SF_OK;
}

// In front of the updates of a stepping call while a schedule is set (enqueue layer): the cache made current for the scheduled
// tables, the due list made on the device, the due tables rebuilt.  Nothing is read back.
static int wind_sched_pass(sf_sim *s)
{
    const Geo &g = s->g;
    const int n = (int)s->wind_sched.size();
    bool cached = s->wind_sched_cached;
    if (!s->wind_sched_ready) {
        const int rc = ensure_wterms(s, s->wind_sched.data(), n);
        if (rc && rc != SF_ENOTSUP) return rc;
        cached = s->wind_sched_cached = rc == SF_OK;
        s->wind_sched_ready = true;
    }
    if (s->wind_timed) HIPCHK(hipEventRecord(s->ev0, s->stream));
    HIPCHK(hipMemsetAsync(s->wdue_cnt, 0, sizeof(uint32_t), s->stream));
    hipLaunchKernelGGL(k_wind_due, dim3((unsigned)((g.E + 255) / 256)), dim3(256), 0, s->stream, g, (const EnvState *)s->commit, (const EnvState *)s->tmp,
                       (const uint32_t *)s->flags, s->seq, s->committed ? 1 : 0, s->wsched, s->wdue_cnt, s->wdue, s->wdue_U, s->wdue_D);
    { int rc = wind_launch(s, s->wdue, s->wdue_cnt, 0, n, s->wdue_U, s->wdue_D, 0, cached); if (rc) return rc; }
    if (s->wind_timed) { HIPCHK(hipEventRecord(s->ev1, s->stream)); s->wind_have_ms = true; }
    return SF_OK;
}

// the tables a wind call addresses: the list, or every table in order; what must hold before any device work
static int wind_targets(const sf_sim *s, const char *who, int32_t n, const int32_t *envs, bool need_per_env, std::vector<int32_t> &tabs)
{
    if (n < 0) return fail(SF_EINVAL, "%s: n = %d", who, n);
    const int n_tab = (int)s->rt_set.size();
    if ((envs || need_per_env) && !s->p.per_env_terrain)
        return fail(SF_ESTATE, "%s: this handle shares one terrain between all environments (create it with per_env_terrain = 1)", who);
    if (envs) { int rc = check_envs(s, who, n, envs, "listed twice"); if (rc) return rc; }
    else if (n != 0 && n != n_tab) return fail(SF_EINVAL, "%s: without a list n must be the number of tables, %d (got %d)", who, n_tab, n);
    tabs.resize((size_t)n);
    for (int i = 0; i < n; ++i) tabs[i] = envs ? envs[i] : i;
    for (int i = 0; i < n; ++i)
        if (!s->rd_lay[tabs[i]]) return fail(SF_ESTATE, "%s: table %d has no layers (sf_set_layers*, sf_generate_layers)", who, tabs[i]);
    return SF_OK;
}

// fire.py:365, 490-494: self.U / self.U_dir reassigned between two update() calls
extern "C" int sf_set_wind(sf_sim *s, int32_t n, const int32_t *envs, const double *U, const double *U_dir, int32_t flags)
{
    if (!s) return fail(SF_EINVAL, "sf_set_wind: null handle");
    if (flags & ~(SF_WIND_FIELD | SF_WIND_DEVICE)) return fail(SF_EINVAL, "sf_set_wind: unknown flags 0x%x", flags);
    if (n > 0 && (!U || !U_dir)) return fail(SF_EINVAL, "sf_set_wind: null argument");
    std::vector<int32_t> tabs;
    { int rc = wind_targets(s, "sf_set_wind", n, envs, false, tabs); if (rc) return rc; }
    if (n == 0) return SF_OK;
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    const Geo &g = s->g;
    const bool field = (flags & SF_WIND_FIELD) != 0, device = (flags & SF_WIND_DEVICE) != 0;
    const size_t cells = (size_t)g.H * g.W, list_bytes = ((size_t)n * 4 + 7) / 8 * 8;
    const bool scalars = !field && !device;         // the host scalars travel behind the list
    CallBlock &blk = s->wind_blk;
    { int rc = block_reserve(s, blk, list_bytes + (scalars ? (size_t)n * 16 : 0)); if (rc) return rc; }
    memcpy(blk.pinned, tabs.data(), (size_t)n * 4);
    if (scalars) { memcpy(blk.pinned + list_bytes, U, (size_t)n * 8); memcpy(blk.pinned + list_bytes + (size_t)n * 8, U_dir, (size_t)n * 8); }
    { int rc = block_send(s, blk, list_bytes + (scalars ? (size_t)n * 16 : 0)); if (rc) return rc; }
    const int32_t *list_dev = (const int32_t *)blk.dev;
    const int rcw = ensure_wterms(s, tabs.data(), n);
    if (rcw && rcw != SF_ENOTSUP) return rcw;
    const bool cached = rcw == SF_OK;
    if (s->wind_timed) HIPCHK(hipEventRecord(s->ev0, s->stream));
    if (field && !device) {
        // host fields go through the stage buffer, as many tables at a time as fit 64 MB of it (one at least)
        const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)n, ((size_t)64 << 20) / (cells * 16)));
        { int rc = ensure_stage(s, (size_t)chunk * cells * 16); if (rc) return rc; }
        double *su = (double *)s->stage, *sd = su + (size_t)chunk * cells;
        for (int i0 = 0; i0 < n; i0 += chunk) {
            const int cnt = std::min(chunk, n - i0);
            HIPCHK(hipMemcpyAsync(su, U + (size_t)i0 * cells, (size_t)cnt * cells * 8, hipMemcpyHostToDevice, s->stream));
            HIPCHK(hipMemcpyAsync(sd, U_dir + (size_t)i0 * cells, (size_t)cnt * cells * 8, hipMemcpyHostToDevice, s->stream));
            int rc = wind_launch(s, list_dev + i0, nullptr, cnt, cnt, su, sd, 1, cached);
            if (rc) return rc;
        }
    } else {
        const double *u = scalars ? (const double *)(blk.dev + list_bytes) : U, *d = scalars ? (const double *)(blk.dev + list_bytes) + n : U_dir;
        int rc = wind_launch(s, list_dev, nullptr, n, n, u, d, field ? 1 : 0, cached);
        if (rc) return rc;
    }
    if (s->wind_timed) { HIPCHK(hipEventRecord(s->ev1, s->stream)); s->wind_have_ms = true; }
    // the direction-major table was replaced; the cell-major copy, where the buffer exists, was written in the same pass
    if (s->rtc_stale.size() != s->rt_set.size()) s->rtc_stale.assign(s->rt_set.size(), 1);
    for (int i = 0; i < n; ++i) {
        s->rt_set[tabs[i]] = 1;
        s->rtc_stale[tabs[i]] = s->rtc ? 0 : 1;
    }
    s->have_rt = true;
    for (char c : s->rt_set) if (!c) s->have_rt = false;
    bool had = false;
    for (int i = 0; i < n; ++i) if (s->wsched && s->wind_K[tabs[i]]) { had = true; s->wind_K[tabs[i]] = 0; }
    if (had) {           // a wind set by hand ends the environment's schedule
        hipLaunchKernelGGL(k_wind_sched_set, dim3((unsigned)n), dim3(SF_WIND_MAX_SEGS), 0, s->stream, n, list_dev, 0, (const sf_wind_seg *)nullptr, s->wsched);
        HIPCHK(hipGetLastError());
        wind_sched_count(s);
    }
    return finish_call(s, nullptr, !s->async, nullptr);
}

extern "C" int sf_set_wind_schedule(sf_sim *s, int32_t n, const int32_t *envs, int32_t K, const sf_wind_seg *segs)
{
    const char *who = "sf_set_wind_schedule";
    if (!s) return fail(SF_EINVAL, "%s: null handle", who);
    if (K < 0 || K > SF_WIND_MAX_SEGS) return fail(SF_EINVAL, "%s: 0 .. %d segments (got %d)", who, SF_WIND_MAX_SEGS, K);
    if (s->ep_on && (s->ep.flags & SF_EP_WIND))
        return fail(SF_ESTATE, "%s: every new episode draws its wind (sf_episodes_set with SF_EP_WIND): a schedule would fight it over the table", who);
    if (n > 0 && K > 0 && !segs) return fail(SF_EINVAL, "%s: null argument", who);
    std::vector<int32_t> tabs;
    { int rc = wind_targets(s, who, n, envs, true, tabs); if (rc) return rc; }
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < K; ++k) {
            const sf_wind_seg &r = segs[(size_t)i * K + k];
            if (r.reserved != 0) return fail(SF_EINVAL, "%s: environment %d, segment %d: reserved must be 0", who, tabs[i], k);
            if (k == 0 ? r.first_update != 0 : r.first_update <= segs[(size_t)i * K + k - 1].first_update)
                return fail(SF_EINVAL, "%s: environment %d: first_update must be 0 for segment 0 and strictly increasing (segment %d: %d)", who,
                            tabs[i], k, r.first_update);
        }
    if (n == 0) return SF_OK;
    if (K == 0 && !s->wsched) return SF_OK;
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    const Geo &g = s->g;
    if (!s->wsched) {
        { int rc = dev_alloc(s, &s->wsched, (size_t)g.E); if (rc) return rc; }
        { int rc = dev_alloc(s, &s->wdue_U, (size_t)2 * g.E); if (rc) return rc; }
        { int rc = dev_alloc(s, &s->wdue, (size_t)g.E + 2); if (rc) return rc; }
        s->wdue_D = s->wdue_U + g.E;
        s->wdue_cnt = reinterpret_cast<uint32_t *>(s->wdue + g.E);
        HIPCHK(hipMemsetAsync(s->wsched, 0, sizeof(WindSched) * g.E, s->stream));
        s->wind_K.assign((size_t)g.E, 0);
    }
    const size_t list_bytes = ((size_t)n * 4 + 7) / 8 * 8, rows_bytes = (size_t)n * K * sizeof(sf_wind_seg);
    CallBlock &blk = s->wind_blk;
    { int rc = block_reserve(s, blk, list_bytes + rows_bytes); if (rc) return rc; }
    memcpy(blk.pinned, tabs.data(), (size_t)n * 4);
    if (rows_bytes) memcpy(blk.pinned + list_bytes, segs, rows_bytes);
    { int rc = block_send(s, blk, list_bytes + rows_bytes); if (rc) return rc; }
    hipLaunchKernelGGL(k_wind_sched_set, dim3((unsigned)n), dim3(SF_WIND_MAX_SEGS), 0, s->stream, n, (const int32_t *)blk.dev, K,
                       (const sf_wind_seg *)(blk.dev + list_bytes), s->wsched);
    HIPCHK(hipGetLastError());
    for (int i = 0; i < n; ++i) s->wind_K[tabs[i]] = K;
    wind_sched_count(s);
    return finish_call(s, nullptr, !s->async, nullptr);
}

// Laboratory (include/simfire_hip_lab.h): the cache switched off (freed; every wind change then builds from the layers) or on again;
// HIP events around the launches of every wind change and every schedule pass.
extern "C" int sf_set_wind_lab(sf_sim *s, int32_t cache_on, int32_t timed)
{
    if (!s) return fail(SF_EINVAL, "sf_set_wind_lab: null handle");
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    if (!cache_on && s->wterms) {
        HIPCHK(hipStreamSynchronize(s->stream));
        HIPCHK(hipFree(s->wterms));
        s->wterms = nullptr;
        s->bytes -= (int64_t)((size_t)kWindPlanes * s->g.H * s->g.W * s->rt_set.size() * sizeof(float));
    }
    s->wt_off = !cache_on;
    s->wind_sched_ready = false;
    s->ep_nocache = false;
    s->wind_timed = timed != 0;
    s->wind_have_ms = false;
    return SF_OK;
}
extern "C" int sf_get_wind_ms(sf_sim *s, float *ms_out)
{
    if (!s || !ms_out) return fail(SF_EINVAL, "sf_get_wind_ms: null argument");
    if (!s->wind_have_ms) return fail(SF_ESTATE, "sf_get_wind_ms: no wind change or schedule pass has been timed (sf_set_wind_lab)");
    HIPCHK(hipSetDevice(s->p.device));
    HIPCHK(hipEventSynchronize(s->ev1));
    HIPCHK(hipEventElapsedTime(ms_out, s->ev0, s->ev1));
    return SF_OK;
}

static int set_rtable_impl(sf_sim *s, int env, const double *R8)
{
    int lo, hi, rc = table_range(s, env, "sf_set_rtable", &lo, &hi);
    if (rc) return rc;
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    const Geo &g = s->g;
    const size_t n = (size_t)8 * g.H * g.W * sizeof(double);
    rc = ensure_stage(s, n);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(s->stage, R8, n, hipMemcpyHostToDevice, s->stream));
    dim3 blk(256), grd((g.P + 255) / 256, g.H, 8);
    const size_t tab = (size_t)8 * g.plane_env;
    for (int i = lo; i < hi; ++i)
        hipLaunchKernelGGL(k_pack_rt, grd, blk, 0, s->stream, g.H, g.W, g.P, (const double *)s->stage, s->rt + (size_t)i * tab);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s->stream));
    mark_tables(s, lo, hi);
    return SF_OK;
}

extern "C" int sf_set_rtable(sf_sim *s, const double *R8)
{
    if (!s || !R8) return fail(SF_EINVAL, "sf_set_rtable: null argument");
    return set_rtable_impl(s, -1, R8);
}

extern "C" int sf_set_rtable_env(sf_sim *s, int32_t env, const double *R8)
{
    if (!s || !R8) return fail(SF_EINVAL, "sf_set_rtable_env: null argument");
    if (env < 0) return fail(SF_EINVAL, "sf_set_rtable_env: environment %d out of range", env);
    return set_rtable_impl(s, env, R8);
}

static int get_rtable_impl(sf_sim *s, int env, double *out)
{
    const int n_tab = (int)s->rt_set.size();
    const int t = n_tab == 1 ? 0 : env;
    if (t < 0 || t >= n_tab) return fail(SF_EINVAL, "sf_get_rtable: environment %d out of range", env);
    if (!s->rt_set[t]) return fail(SF_ESTATE, "sf_get_rtable: no layers / table set");
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    const Geo &g = s->g;
    const size_t n = (size_t)8 * g.H * g.W * sizeof(double);
    int rc = ensure_stage(s, n);
    if (rc) return rc;
    dim3 blk(256), grd((g.W + 255) / 256, g.H, 8);
    hipLaunchKernelGGL(k_unpack_f64, grd, blk, 0, s->stream, g.H, g.W, g.P,
                       (const double *)(s->rt + (size_t)t * 8 * g.plane_env), (double *)s->stage);
    HIPCHK(hipMemcpyAsync(out, s->stage, n, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return SF_OK;
}

extern "C" int sf_get_rtable(sf_sim *s, double *out)
{
    if (!s || !out) return fail(SF_EINVAL, "sf_get_rtable: null argument");
    return get_rtable_impl(s, 0, out);
}

extern "C" int sf_get_rtable_env(sf_sim *s, int32_t env, double *out)
{
    if (!s || !out) return fail(SF_EINVAL, "sf_get_rtable_env: null argument");
    return get_rtable_impl(s, env, out);
}

extern "C" int sf_get_slopes(sf_sim *s, double *mag, double *dir)
{
    if (!s || !mag || !dir) return fail(SF_EINVAL, "sf_get_slopes: null argument");
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    const size_t n = (size_t)s->g.H * s->g.W * sizeof(double);
    HIPCHK(hipMemcpyAsync(mag, s->smag, n, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipMemcpyAsync(dir, s->sdir, n, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return SF_OK;
}

// The environment states live in the tmp / flags rings while steps are being enqueued; they are folded
// into commit[] only when something needs them (status queries, resets, burn_amounts transfers).
static int ensure_commit(sf_sim *s)
{
    LOOP_QUIESCE(s);
    if (s->committed) return SF_OK;
    hipLaunchKernelGGL(k_commit, dim3((s->g.E + 255) / 256), dim3(256), 0, s->stream, s->g, s->commit,
                       (const EnvState *)s->tmp, s->flags, (s->seq + 5) % 6, s->n_active);
    HIPCHK(hipGetLastError());
    s->committed = true;
    return SF_OK;
}

// The per-environment slices of the handle's buffers, of the kinds asked for, in the layout that is current (sf_env_segs.h; what each
// is: DESIGN.md section 11).  Looked up per call: the blocked plane, settled, parents, snap, the sink and rtc exist lazily or not at
// all, and a slice that does not exist is left out.  out holds kEnvSegs entries; the number written is returned.
static int env_segs(const sf_sim *s, unsigned kinds, EnvSeg *out)
{
    const Geo &g = s->g;
    int n = 0;
    auto add = [&](unsigned kind, void *base, long long len) {
        if (!(kinds & kind) || !base) return;
        assert(n < kEnvSegs);
        out[n++] = {static_cast<uint8_t *>(base), len, len};
    };
    if (s->bl_cur) add(kSegCells, s->cells_alloc, g.cells_env);
    else {
        add(kSegCells, s->status, g.plane_env);
        add(kSegCells, s->age_alloc, g.age_env * g.ab);      // (with its guard rows)
    }
    add(kSegBurn, s->burn, g.plane_env * 8);
    add(kSegSettled, s->settled, g.plane_env * 4);
    add(kSegParents, s->parents, g.plane_env);
    add(kSegSnap, s->snap, g.plane_env);
    add(kSegState, s->commit, sizeof(EnvState));
    add(kSegResult, s->status_block, 32);
    add(kSegResult, s->elapsed_dev, 8);
    add(kSegResult, s->sink, 32);
    const long long fplane = (long long)g.TYp * g.TXp, tiles = (long long)g.TY * g.TX;
    for (int k = 0; k < 2; ++k) add(kSegTflags, s->tflags + (size_t)k * g.E * fplane, fplane);
    for (int k = 0; k < 3; ++k) add(kSegVbits, s->vbits + (size_t)k * g.E * g.vb_env, g.vb_env * 8);
    add(kSegSeam, s->seam, g.seam_env);
    add(kSegHist, s->tdirty, tiles);
    add(kSegHist, s->thist, tiles * 16);
    add(kSegHint, s->win_hint, 8);
    add(kSegCost, s->run_cost, 4);
    const long long tab = 8 * g.plane_env * (long long)sizeof(double), lay = 7LL * g.H * g.W * (long long)sizeof(double);
    add(kSegTerrain, s->rt, tab);            // (per table: a caller asks for these on a per-environment-terrain handle only)
    add(kSegTerrain, s->lay_all, lay);
    add(kSegTerrain, s->rtc, tab);
    return n;
}
// x extent of the grid of a kernel that walks these slices (env_seg_walk): ~8 vectors per lane of the longest slice
static unsigned seg_grid_x(const EnvSeg *seg, int n)
{
    long long longest = 0;
    for (int k = 0; k < n; ++k) longest = std::max(longest, seg[k].len);
    return (unsigned)std::min<long long>(1024, std::max<long long>(1, (longest / 16 + 2047) / 2048));
}

// rows (env, column, row, type) in device memory -> the two scatter kernels (clear, then write with the
// type precedence of simulation.py:449-478); rows with an out-of-range field are skipped by the kernels
static int scatter_points(sf_sim *s, const int32_t *pts_dev, int n)
{
    const Geo &g = s->g;
    uint8_t *cells = s->bl_cur ? s->cells : nullptr;
    s->status_fresh = false;
    const dim3 grd((unsigned)((n + 255) / 256)), blk(256);
    hipLaunchKernelGGL(k_mitigate_clear, grd, blk, 0, s->stream, g, s->status, cells, (const uint32_t *)s->settled, s->burn,
                       (const EnvState *)s->commit, (const EnvState *)s->tmp, (const uint32_t *)s->flags, s->seq,
                       s->committed ? 1 : 0, pts_dev, n);
    hipLaunchKernelGGL(k_mitigate_write, grd, blk, 0, s->stream, g, s->status, cells, s->settled, s->tdirty,
                       (const EnvState *)s->commit, (const EnvState *)s->tmp, (const uint32_t *)s->flags, s->seq,
                       s->committed ? 1 : 0, pts_dev, n);
    HIPCHK(hipGetLastError());
    return SF_OK;
}

extern "C" int sf_apply_mitigation(sf_sim *s, const int32_t *pts, int32_t n)
{
    if (!s) return fail(SF_EINVAL, "sf_apply_mitigation: null handle");
    if (n < 0 || (n > 0 && !pts)) return fail(SF_EINVAL, "sf_apply_mitigation: bad point list");
    if (n == 0) return SF_OK;
    const Geo &g = s->g;
    for (int i = 0; i < n; ++i) {
        const int32_t *q = pts + 4 * i;
        if (q[0] < 0 || q[0] >= g.E || q[1] < 0 || q[1] >= g.W || q[2] < 0 || q[2] >= g.H)
            return fail(SF_EINVAL, "sf_apply_mitigation: point %d = (env %d, x %d, y %d) is out of range", i, q[0], q[1], q[2]);
    }
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    const size_t bytes = (size_t)4 * n * sizeof(int32_t);
    if ((size_t)4 * n > s->pts_cap) {
        HIPCHK(hipStreamSynchronize(s->stream));
        for (int i = 0; i < sf_sim::kPtsRing; ++i) {
            if (s->pts_pinned[i]) HIPCHK(hipHostFree(s->pts_pinned[i]));
            s->pts_pinned[i] = nullptr;
        }
        s->pts_cap = (size_t)4 * n * 2;
        for (int i = 0; i < sf_sim::kPtsRing; ++i) {
            HIPCHK(hipHostMalloc(reinterpret_cast<void **>(&s->pts_pinned[i]), s->pts_cap * sizeof(int32_t), hipHostMallocMapped));
            HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void **>(&s->pts_mapped[i]), s->pts_pinned[i], 0));
        }
    }
    const int slot = s->pts_slot;
    s->pts_slot = (slot + 1) % sf_sim::kPtsRing;
    // The scatter kernels read the points straight from this pinned, device-mapped buffer (a few
    // KB over the host link; no copy to enqueue).  It may still feed kernels enqueued kPtsRing calls ago.
    HIPCHK(hipEventSynchronize(s->ev_pts[slot]));
    memcpy(s->pts_pinned[slot], pts, bytes);
    int rc = scatter_points(s, s->pts_mapped[slot], n);
    if (rc) return rc;
    HIPCHK(hipEventRecord(s->ev_pts[slot], s->stream));
    return finish_call(s, nullptr, !s->async, nullptr);
}

extern "C" int sf_apply_mitigation_device(sf_sim *s, const int32_t *device_pts, int32_t n)
{
    if (!s) return fail(SF_EINVAL, "sf_apply_mitigation_device: null handle");
    if (n < 0 || (n > 0 && !device_pts)) return fail(SF_EINVAL, "sf_apply_mitigation_device: bad point list");
    if (n == 0) return SF_OK;
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    const int rc = scatter_points(s, device_pts, n);
    return rc ? rc : finish_call(s, nullptr, !s->async, nullptr);
}

extern "C" int sf_load_fire_map(sf_sim *s, int32_t env, const uint8_t *map)
{
    if (!s || !map) return fail(SF_EINVAL, "sf_load_fire_map: null argument");
    const Geo &g = s->g;
    if (env < 0 || env >= g.E) return fail(SF_EINVAL, "sf_load_fire_map: environment %d out of range", env);
    const size_t n = (size_t)g.H * g.W;
    for (size_t i = 0; i < n; ++i)
        if (map[i] > SF_WETLINE) return fail(SF_EINVAL, "sf_load_fire_map: value %d at cell %zu is not a BurnStatus", map[i], i);
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    s->fire_rows = 0;                  // (a map from outside: its fire may be of any size)
    if (s->snap) s->snap_valid[env] = 0;      // (sf_get_fire_map_delta: no reference point any more)
    int rc = ensure_stage(s, n);
    if (rc) return rc;
    dim3 blk(256), grd((g.W + 255) / 256, g.H);
    rc = ensure_commit(s);
    if (rc) return rc;
    rc = ensure_rm(s);
    if (rc) return rc;
    s->status_fresh = false;
    if (g.att)
        hipLaunchKernelGGL(k_settle_env, grd, blk, 0, s->stream, g, (const uint8_t *)s->status, s->settled, s->burn,
                           (const EnvState *)s->commit, env, 1);
    HIPCHK(hipMemcpyAsync(s->stage, map, n, hipMemcpyHostToDevice, s->stream));
    hipLaunchKernelGGL(k_pack_status, grd, blk, 0, s->stream, g, s->status, s->settled, (const EnvState *)s->commit, env,
                       (const uint8_t *)s->stage);
    HIPCHK(hipGetLastError());
    rc = rebuild_tflags(s, env, 1);
    s->tdirty_all = true;
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(s->stream));
    return SF_OK;
}

// The resident launch works on the blocked cell plane (sf_common.h, bl_vec), everything else on the row-major planes; the
// one that is current is converted when the other kind of work comes next (one sweep over the cell planes).
static int ensure_rm(sf_sim *s)
{
    if (!s->bl_cur) return SF_OK;
    const Geo &g = s->g;
    hipLaunchKernelGGL(k_bl_to_rm, dim3((g.PV + 63) / 64, g.H, g.E), dim3(64), 0, s->stream, g, (const uint8_t *)s->cells, s->status, s->age);
    HIPCHK(hipGetLastError());
    s->bl_cur = false;
    return SF_OK;
}
static int alloc_bl(sf_sim *s)
{
    if (s->cells_alloc) return SF_OK;
    const Geo &g = s->g;
    const size_t bytes = (size_t)g.E * g.cells_env;
    int rc = dev_alloc(s, &s->cells_alloc, bytes);
    if (rc) return rc;
    s->cells = s->cells_alloc + (size_t)g.PV * 128;        // quad 0 of environment 0 (a guard quad above and below every environment)
    HIPCHK(hipMemsetAsync(s->cells_alloc, 0, bytes, s->stream));
    return SF_OK;
}
// Will sf_step(n >= 2) of this handle pick the resident launch (the automatic rule of plan_step)?  Then a reset writes the
// blocked plane straight away.
static bool prefers_bl(const sf_sim *s)
{
    const Geo &g = s->g;
    return g.ab == 1 && !s->generic && (g.VW == 1 || (g.VW == 2 && s->tune.v[SF_TUNE_RUN_TEAM] != 1)) && !s->graph_on && !s->history &&
           (s->fused_mode < 0 || s->fused_mode == 2);
}
// the cell-major copy of the R table(s) the window phase of k_run reads (one sweep after every change of the table)
static int ensure_rtc(sf_sim *s)
{
    if (s->rtc_valid) return SF_OK;
    const Geo &g = s->g;
    const size_t n_tab = s->rt_set.size(), tab = (size_t)8 * g.plane_env;
    if (!s->rtc) {
        // (the copy doubles the handle's largest allocation with per-environment terrain; the window phase it serves is optional: a handle
        // that cannot have it runs without - the caller switches the phase off for the call, results never depend on it)
        if (hipMalloc(reinterpret_cast<void **>(&s->rtc), tab * n_tab * sizeof(double)) != hipSuccess) { (void)hipGetLastError(); s->rtc = nullptr; return SF_ENOTSUP; }
        s->bytes += (int64_t)(tab * n_tab * sizeof(double));
        s->rtc_stale.assign(n_tab, 1);
    }
    if (s->rtc_stale.size() != n_tab) s->rtc_stale.assign(n_tab, 1);
    for (size_t i = 0; i < n_tab; ++i)
        if (s->rtc_stale[i]) {
            hipLaunchKernelGGL(k_rt_cellmajor, dim3((g.P + 255) / 256, g.H), dim3(256), 0, s->stream, g.H, g.P, (const double *)(s->rt + i * tab), s->rtc + i * tab);
            s->rtc_stale[i] = 0;
        }
    HIPCHK(hipGetLastError());
    s->rtc_valid = true;
    return SF_OK;
}

static int ensure_bl(sf_sim *s)
{
    if (s->bl_cur) return SF_OK;
    const Geo &g = s->g;
    { int rc = alloc_bl(s); if (rc) return rc; }
    hipLaunchKernelGGL(k_rm_to_bl, dim3((g.PV + 63) / 64, g.H, g.E), dim3(64), 0, s->stream, g, (const uint8_t *)s->status, (const uint8_t *)s->age, s->cells);
    HIPCHK(hipGetLastError());
    s->bl_cur = true;
    return SF_OK;
}

// The per-step tiled kernels keep the tile activity map and the seam planes, the resident launch keeps the vector
// bitmap; whichever a launch needs is rebuilt from the sprite-mask planes if the other kind ran in between.
static int ensure_tiles(sf_sim *s)
{
    if (s->tiles_valid) return SF_OK;
    { int rc0 = ensure_rm(s); if (rc0) return rc0; }
    HIPCHK(hipMemsetAsync(s->tflags, 0, s->tflags_bytes, s->stream));
    int rc = rebuild_tflags(s, 0, s->g.E);
    if (rc) return rc;
    rc = rebuild_seams(s, 0, s->g.E);
    if (rc) return rc;
    s->tiles_valid = true;
    return SF_OK;
}
static int ensure_vbits(sf_sim *s)
{
    if (s->vbits_valid) return SF_OK;
    { int rc0 = ensure_rm(s); if (rc0) return rc0; }
    const Geo &g = s->g;
    hipLaunchKernelGGL(k_rebuild_vbits, dim3(g.VW, g.H, g.E), dim3(64), 0, s->stream, g, (const uint8_t *)s->age, s->vbits, 0);
    HIPCHK(hipGetLastError());
    s->vbits_valid = true;
    s->vbits_fl_valid = true;
    return SF_OK;
}

// ----------------------------------------------------------------------------- arrival times
// The pass behind the launches (sf_arrival_kernels.h): reads every environment's update count from commit[], so the step rings are
// folded first.  Sparse where the blocked plane is current and every plane of the vector bitmap is known to match it, else dense over
// whichever plane is current.  Recording off: nothing.
static int arrival_pass(sf_sim *s)
{
    if (!s->arrival1) return SF_OK;
    { int rc0 = ensure_commit(s); if (rc0) return rc0; }
    const Geo &g = s->g;
    const bool sparse = s->bl_cur && s->vbits_valid && s->vbits_fl_valid && !s->arr_dense;
    if (sparse) {
        hipLaunchKernelGGL(k_arrival_bits, dim3((unsigned)((g.H * g.VW + 255) / 256), (unsigned)g.E), dim3(256), 0, s->stream, g, (const uint8_t *)s->cells,
                           (const unsigned long long *)s->vbits, (const EnvState *)s->commit, s->arrival1);
    } else {
        const dim3 grd((unsigned)((g.W + 255) / 256), (unsigned)g.H, (unsigned)g.E), blk(256);
        const uint8_t *cells = s->bl_cur ? s->cells : nullptr;
        if (g.ab == 1) hipLaunchKernelGGL(k_arrival_cells<uint8_t>, grd, blk, 0, s->stream, g, (const uint8_t *)s->age, cells, (const EnvState *)s->commit, s->arrival1);
        else if (g.ab == 2) hipLaunchKernelGGL(k_arrival_cells<uint16_t>, grd, blk, 0, s->stream, g, (const uint8_t *)s->age, cells, (const EnvState *)s->commit, s->arrival1);
        else hipLaunchKernelGGL(k_arrival_cells<uint32_t>, grd, blk, 0, s->stream, g, (const uint8_t *)s->age, cells, (const EnvState *)s->commit, s->arrival1);
    }
    HIPCHK(hipGetLastError());
    s->arr_passes[sparse ? 0 : 1]++;
    s->arr_pending = 0;
    return s->val_plane ? value_pass(s) : SF_OK;      // the plane is complete up to commit[].steps: so is the damage behind this
}
// The plane's per-environment slice behind the n slices env_segs has filled (a reset zeroes it, a fork copies it): appended here and not
// a kind of sf_env_segs.h - the plane is not one of the buffers the step kernels know.  Returns the new count.
static int arrival_seg(const sf_sim *s, EnvSeg *seg, int n)
{
    if (!s->arrival1) return n;
    assert(n < kEnvSegs);
    const long long len = s->g.plane_env * 4;
    seg[n] = {reinterpret_cast<uint8_t *>(s->arrival1), len, len};
    return n + 1;
}

// ----------------------------------------------------------------------------- values at risk
static ValueArgs value_args(const sf_sim *s)
{
    ValueArgs a;
    a.values = s->val_plane; a.values_env = s->val_per_env ? s->g.plane_env : 0;
    a.arrival1 = s->arrival1; a.commit = s->commit; a.rec = s->val_rec();
    return a;
}
// The pass behind the arrival pass (sf_value_kernels.h; arrival_pass has folded the step rings and completed the plane): the sum
// over the window in the sparse form under the arrival pass's own condition, else dense, then the commit of the records.
static int value_pass(sf_sim *s)
{
    const Geo &g = s->g;
    const bool sparse = s->bl_cur && s->vbits_valid && s->vbits_fl_valid && !s->val_dense;
    if (sparse) hipLaunchKernelGGL(k_value_bits, dim3((unsigned)((g.H * g.VW + 255) / 256), (unsigned)g.E), dim3(256), 0, s->stream, g,
                                   (const unsigned long long *)s->vbits, value_args(s));
    else hipLaunchKernelGGL(k_value_cells, dim3((unsigned)((g.W + 255) / 256), (unsigned)g.H, (unsigned)g.E), dim3(256), 0, s->stream, g, value_args(s));
    hipLaunchKernelGGL(k_value_commit, dim3((unsigned)((g.E + 255) / 256)), dim3(256), 0, s->stream, g.E, (const EnvState *)s->commit, s->val_rec());
    HIPCHK(hipGetLastError());
    s->val_passes[sparse ? 0 : 1]++;
    return SF_OK;
}
// Every record from the arrival plane as it stands (sf_values_set, sf_load_state): records of zeros, then the dense form once over
// every environment - by the invariant exact for all of them.  A handle that was never reset has nothing to count.
static int value_recount(sf_sim *s)
{
    if (!s->val_plane) return SF_OK;
    const Geo &g = s->g;
    HIPCHK(hipMemsetAsync(s->val_rec(), 0, (size_t)g.E * sizeof(ValueRec), s->stream));
    if (!s->was_reset) return SF_OK;
    if (s->arr_pending) return arrival_pass(s);       // (a call that failed half way left updates behind: the plane first, the pass behind it counts)
    { int rc = ensure_commit(s); if (rc) return rc; }
    hipLaunchKernelGGL(k_value_cells, dim3((unsigned)((g.W + 255) / 256), (unsigned)g.H, (unsigned)g.E), dim3(256), 0, s->stream, g, value_args(s));
    hipLaunchKernelGGL(k_value_commit, dim3((unsigned)((g.E + 255) / 256)), dim3(256), 0, s->stream, g.E, (const EnvState *)s->commit, s->val_rec());
    HIPCHK(hipGetLastError());
    s->val_passes[1]++;
    return SF_OK;
}
// The record's slice behind the arrival plane's (a reset zeroes it: upto1 == 0, the pass behind the reset sums the ignition; a fork
// copies it with the plane): appended like arrival_seg.  Returns the new count.
static int value_seg(const sf_sim *s, EnvSeg *seg, int n)
{
    if (!s->val_plane) return n;
    assert(n < kEnvSegs);
    seg[n] = {reinterpret_cast<uint8_t *>(s->val_rec()), (long long)sizeof(ValueRec), (long long)sizeof(ValueRec)};
    return n + 1;
}
static int value_free(sf_sim *s)
{
    if (!s->val_plane) return SF_OK;
    HIPCHK(hipStreamSynchronize(s->stream));
    s->bytes -= (int64_t)(s->val_plane_bytes() + s->val_aux_bytes());
    HIPCHK(hipFree(s->val_plane)); s->val_plane = nullptr;
    HIPCHK(hipFree(s->val_aux)); s->val_aux = nullptr;
    s->val_w_on = false;
    return SF_OK;
}

extern "C" int sf_values_set(sf_sim *s, const int32_t *values, int32_t per_env, int32_t device_pointer)
{
    if (!s) return fail(SF_EINVAL, "sf_values_set: null handle");
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    if (!values) return value_free(s);
    if (!s->arrival1) return fail(SF_ESTATE, "sf_values_set: call sf_enable_arrival first (the arrival plane says which cells count)");
    const Geo &g = s->g;
    const size_t n_planes = per_env ? (size_t)g.E : 1, rows = n_planes * g.H, cells = rows * g.W;
    if (!device_pointer)
        for (size_t i = 0; i < cells; ++i)
            if (values[i] > kValueMax || values[i] < -kValueMax)
                return fail(SF_EINVAL, "sf_values_set: value %d (entry %lld) is outside -2^24 .. 2^24", values[i], (long long)i);
    { int rc = check_team_error(s, "sf_values_set"); if (rc) return rc; }
    // the new plane and, the first time, the records: made and checked before the handle changes (a refused call leaves it as it was)
    int32_t *plane = nullptr;
    uint8_t *aux = s->val_aux;
    const size_t plane_bytes = rows * g.P * sizeof(int32_t);
    HIPCHK(hipMalloc(reinterpret_cast<void **>(&plane), plane_bytes));
    if (!aux && hipMalloc(reinterpret_cast<void **>(&aux), s->val_aux_bytes()) != hipSuccess) { (void)hipFree(plane); return fail(SF_EHIP, "sf_values_set: hipMalloc failed"); }
    hipError_t err = hipMemsetAsync(aux, 0, s->val_aux_bytes(), s->stream);      // (records and ticks start from zero under a new plane)
    if (err == hipSuccess) err = hipMemsetAsync(plane, 0, plane_bytes, s->stream);
    if (err == hipSuccess) err = hipMemcpy2DAsync(plane, (size_t)g.P * 4, values, (size_t)g.W * 4, (size_t)g.W * 4, rows,
                                                  device_pointer ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s->stream);
    uint32_t bad = 0;
    if (err == hipSuccess && device_pointer) {
        uint32_t *word = reinterpret_cast<uint32_t *>(aux + (size_t)g.E * (sizeof(ValueRec) + 16));
        hipLaunchKernelGGL(k_value_range, dim3((unsigned)std::min<size_t>((cells + 255) / 256, 4096)), dim3(256), 0, s->stream, values, (long long)cells, word);
        err = hipGetLastError();
        if (err == hipSuccess) err = hipMemcpyAsync(&bad, word, sizeof bad, hipMemcpyDeviceToHost, s->stream);
    }
    if (err == hipSuccess) err = hipStreamSynchronize(s->stream);      // (the caller's memory is free again; kernels that read the old plane are through)
    if (err != hipSuccess || bad) {
        (void)hipFree(plane);
        if (!s->val_aux) (void)hipFree(aux);
        else if (s->was_reset) (void)value_recount(s);      // (the records were zeroed above: counted again under the plane that stays)
        if (bad) return fail(SF_EINVAL, "sf_values_set: a value of the device plane is outside -2^24 .. 2^24");
        return fail(SF_EHIP, "sf_values_set: %s", hipGetErrorString(err));
    }
    if (s->val_plane) { s->bytes -= (int64_t)s->val_plane_bytes(); HIPCHK(hipFree(s->val_plane)); }
    else s->bytes += (int64_t)s->val_aux_bytes();
    s->val_plane = plane; s->val_aux = aux; s->val_per_env = per_env != 0;
    s->bytes += (int64_t)s->val_plane_bytes();
    { int rc = value_recount(s); if (rc) return rc; }
    return finish_call(s, nullptr, !s->async, nullptr);
}

extern "C" int sf_values_get(sf_sim *s, int64_t *damage_out)
{
    if (!s || !damage_out) return fail(SF_EINVAL, "sf_values_get: null argument");
    if (!s->val_plane) return fail(SF_ESTATE, "sf_values_get: call sf_values_set first");
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    HIPCHK(hipMemcpy2DAsync(damage_out, 8, s->val_rec(), sizeof(ValueRec), 8, (size_t)s->g.E, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return check_team_error(s, "sf_values_get");
}

extern "C" int sf_values_device(sf_sim *s, void **damage, int64_t *damage_stride, void **tick_loss)
{
    if (!s || !damage || !damage_stride || !tick_loss) return fail(SF_EINVAL, "sf_values_device: null argument");
    if (!s->val_plane) return fail(SF_ESTATE, "sf_values_device: call sf_values_set first");
    *damage = s->val_rec(); *damage_stride = (int64_t)sizeof(ValueRec); *tick_loss = s->val_tick(1);
    return SF_OK;
}

extern "C" int sf_values_set_weight(sf_sim *s, float w_value, int32_t on)
{
    if (!s) return fail(SF_EINVAL, "sf_values_set_weight: null handle");
    if (!s->ag.k) return fail(SF_ESTATE, "sf_values_set_weight: call sf_agents_create first");
    if (!s->val_plane) return fail(SF_ESTATE, "sf_values_set_weight: call sf_values_set first");
    s->val_w = w_value; s->val_w_on = on != 0;
    return SF_OK;
}

extern "C" int sf_set_values_dense(sf_sim *s, int32_t on)
{
    if (!s) return fail(SF_EINVAL, "sf_set_values_dense: null handle");
    s->val_dense = on != 0;
    return SF_OK;
}

extern "C" int sf_get_value_passes(sf_sim *s, int64_t *out)
{
    if (!s || !out) return fail(SF_EINVAL, "sf_get_value_passes: null argument");
    out[0] = s->val_passes[0]; out[1] = s->val_passes[1];
    return SF_OK;
}

// ----------------------------------------------------------------------------- ensemble statistics
// One launch of k_ensemble (sf_ensemble_kernels.h) over the arrival plane as it stands: the call converts no plane, folds no ring and
// looks at no result row - it reads arrival1 (complete behind every stepping call) and the value plane, and writes the caller's outputs.
template <int TP>
static void ensemble_launch(bool loss, dim3 grd, hipStream_t st, const EnsArgs &a)
{
    if (loss) hipLaunchKernelGGL((k_ensemble<TP, true>), grd, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_ensemble<TP, false>), grd, dim3(256), 0, st, a);
}

extern "C" int sf_ensemble_stats(sf_sim *s, const sf_ensemble_params *p, const int32_t *members, const sf_ensemble_out *out)
{
    if (!s || !p || !members || !out) return fail(SF_EINVAL, "sf_ensemble_stats: null argument");
    if (!out->count && !out->prob && !out->first && !out->mean && !out->loss) return fail(SF_EINVAL, "sf_ensemble_stats: no output asked for");
    const Geo &g = s->g;
    const int G = p->n_groups, K = p->group_size, T = p->n_horizons;
    if (G < 1 || K < 1 || K > 65535 || (long long)G * K > (1LL << 20))
        return fail(SF_EINVAL, "sf_ensemble_stats: %d groups of %d members (G >= 1, 1 <= K <= 65535, G * K <= 2^20)", G, K);
    if (T < 1 || T > SF_ENS_MAX_HORIZONS) return fail(SF_EINVAL, "sf_ensemble_stats: %d horizons (1..%d)", T, SF_ENS_MAX_HORIZONS);
    if (p->reserved != 0) return fail(SF_EINVAL, "sf_ensemble_stats: reserved must be 0");
    for (int t = 0; t < T; ++t) {
        const int h = p->horizons[t];
        if (h < -1 || (h == -1 && t != T - 1)) return fail(SF_EINVAL, "sf_ensemble_stats: horizon %d is %d (>= 0; -1, no limit, only last)", t, h);
        if (t > 0 && h != -1 && h <= p->horizons[t - 1]) return fail(SF_EINVAL, "sf_ensemble_stats: the horizons are not strictly ascending (%d behind %d)", h, p->horizons[t - 1]);
    }
    if (((uintptr_t)out->count | (uintptr_t)out->prob | (uintptr_t)out->first | (uintptr_t)out->mean) & 3 || ((uintptr_t)out->loss & 7))
        return fail(SF_EINVAL, "sf_ensemble_stats: an output is not aligned to its element");
    { int rc = check_envs(s, "sf_ensemble_stats", G * K, members); if (rc) return rc; }
    if (!s->arrival1) return fail(SF_ESTATE, "sf_ensemble_stats: call sf_enable_arrival first (the statistics are read off the arrival plane)");
    if (out->loss && !s->val_plane) return fail(SF_ESTATE, "sf_ensemble_stats: loss needs a value plane (sf_values_set)");
    { int rc = begin_call(s, "sf_ensemble_stats", kNotVoid); if (rc) return rc; }

    const size_t bytes = (size_t)G * K * sizeof(int32_t);
    CallBlock &blk = s->ens_blk;
    { int rc = block_reserve(s, blk, bytes); if (rc) return rc; }
    memcpy(blk.pinned, members, bytes);
    { int rc = block_send(s, blk, bytes); if (rc) return rc; }

    EnsArgs a;
    memset(&a, 0, sizeof a);
    a.arrival1 = s->arrival1; a.plane_env = g.plane_env;
    a.H = g.H; a.W = g.W; a.P = g.P; a.Q = (g.W + 3) / 4;
    a.members = reinterpret_cast<const int32_t *>(blk.dev);
    a.G = G; a.K = K; a.T = T;
    int TP = 1;
    while (TP < T) TP *= 2;
    for (int t = 0; t < SF_ENS_MAX_HORIZONS; ++t) {
        const int h = p->horizons[std::min(t, T - 1)];
        a.hz[t] = h < 0 ? 0xFFFFFFFEu : (uint32_t)h;
    }
    if (out->loss) { a.values = s->val_plane; a.values_env = s->val_per_env ? g.plane_env : 0; }
    a.vec = g.W % 4 == 0 && !(((uintptr_t)out->count | (uintptr_t)out->prob | (uintptr_t)out->first | (uintptr_t)out->mean) & 15);
    a.count = out->count; a.prob = out->prob; a.first = out->first; a.mean = out->mean;
    a.loss = reinterpret_cast<unsigned long long *>(out->loss);
    if (out->loss) HIPCHK(hipMemsetAsync(out->loss, 0, (size_t)G * T * sizeof(int64_t), s->stream));
    const long long quads = (long long)g.H * a.Q;
    const dim3 grd((unsigned)((quads + 255) / 256), (unsigned)std::min(G, kEnsGroupsY), (unsigned)((G + kEnsGroupsY - 1) / kEnsGroupsY));
    const bool loss = out->loss != nullptr;
    if (TP == 1) ensemble_launch<1>(loss, grd, s->stream, a);
    else if (TP == 2) ensemble_launch<2>(loss, grd, s->stream, a);
    else if (TP == 4) ensemble_launch<4>(loss, grd, s->stream, a);
    else ensemble_launch<8>(loss, grd, s->stream, a);
    return finish_call(s, "sf_ensemble_stats", !s->async, nullptr);
}

extern "C" int sf_last_step_launch(sf_sim *s, int32_t *kind)
{
    if (!s || !kind) return fail(SF_EINVAL, "sf_last_step_launch: null argument");
    *kind = s->last_kind;
    return SF_OK;
}

// ----------------------------------------------------------------------------- resident launches
// One word per thread: [attenuation off / on][diagonal spread read at run time / known to be on - every reference config]; control lines
// inside the launch: an instantiation without them (MIT = 0) where diagonal spread is known to be on, the others look at the argument.
// (every other k_run instantiation lives in the library's other translation units: simfire_hip_run2.hip / _run3.hip / _run4.hip)
static RunTable sf_run1_table()
{
    static const RunEntry runs[] = {SF_RUN_ENTRY(1, 0, -1, -1, 0), SF_RUN_ENTRY(1, 0, 1, -1, 0), SF_RUN_ENTRY(1, 1, -1, -1, 0),
                                    SF_RUN_ENTRY(1, 1, 1, -1, 0), SF_RUN_ENTRY(1, 0, 1, 0, 0), SF_RUN_ENTRY(1, 1, 1, 0, 0)};
    return {runs, (int)(sizeof runs / sizeof runs[0]), sizeof(StepArgs)};
}
RunTable sf_run2_table(), sf_run3_table(), sf_run4_table();

enum RunKind { kRunPlain, kRunTeam, kRunJoin, kRunLoop };

// Bitmap words a thread of a k_run workgroup owns (rows per thread x words per row), rounded up to an instantiated 1, 2 or 4 (grids up to
// 1024 x 1024 in 16 waves: one, thirteen registers fewer than four).
static int run_words(int rows, int waves, int vw)
{
    const int need = ((rows + waves * 64 - 1) / (waves * 64)) * vw;
    return need <= 1 ? 1 : (need <= 2 ? 2 : kRunMaxD);      // (two words per thread = 1024 rows in 8 waves: the many-environments regime; the kernel for four spills there, +7 %)
}

// The instantiation k_run<MAXD, ATT, DIAG, MIT, TEAM> a launch of this kind takes.  lines: control lines come inside the launch.
static RunKey run_key(const Geo &g, RunKind kind, int words, bool lines)
{
    const int att = g.att ? 1 : 0, diag = g.diag ? 1 : -1;
    switch (kind) {
    case kRunJoin: return {1, att, 1, 0, 2};                      // (one-word rows, diagonal spread, no control lines inside the launch)
    case kRunLoop: return {words, att, -1, -2, 0};                // (the closed loop looks diagonal spread up at run time)
    // teams: diagonal spread on, no control lines inside the launch on two-word rows = BASELINE config C4: its own instantiations, without the
    // control-line code and its registers; one-word teams look control lines up at run time
    case kRunTeam: return {words, att, diag, (words == 2 && g.diag && !lines) ? 0 : -1, 1};
    default:
        if (words > 2) return {kRunMaxD, att, -1, -1, 0};        // (four words per thread: diagonal spread looked up at run time only)
        return {words, att, diag, (g.diag && !lines) ? 0 : -1, 0};
    }
}

// The host handle of an instantiation, from the tables of the four translation units (sf_run_table.h); null: none, or a unit that was built
// with another StepArgs.
static const void *run_fn(const RunKey &k)
{
    static const RunTable tables[] = {sf_run1_table(), sf_run2_table(), sf_run3_table(), sf_run4_table()};
    for (const RunTable &t : tables)
        for (int i = 0; i < t.n; ++i)
            if (t.entries[i].key == k) return t.args_bytes == sizeof(StepArgs) ? t.entries[i].fn : nullptr;
    return nullptr;
}

// More than 64 KB of dynamic LDS has to be allowed for a kernel first: once per kernel and size (hipFuncSetAttribute is not free).
static hipError_t allow_lds(const sf_sim *s, const void *fn, size_t lds)
{
    if (lds <= 64 * 1024) return hipSuccess;
    auto it = s->lds_allowed.find(fn);
    if (it != s->lds_allowed.end() && it->second >= lds) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) s->lds_allowed[fn] = lds;
    return e;
}

// Every resident launch (k_run, k_win) goes through here: fn is the kernel's host handle, args its arguments.
static int launch_resident(sf_sim *s, const void *fn, unsigned grid, unsigned block, size_t lds, void **args)
{
    HIPCHK(allow_lds(s, fn, lds));
    HIPCHK(hipLaunchKernel(fn, dim3(grid), dim3(block), args, lds, s->stream));
    return SF_OK;
}
static int launch_run(sf_sim *s, const RunKey &k, unsigned grid, unsigned block, size_t lds, StepArgs &a, int n_steps, int vcap, int bsz)
{
    const void *fn = run_fn(k);
    if (!fn) return fail(SF_EHIP, "k_run<%d, %d, %d, %d, %d> is not in this library (or its unit was built with another StepArgs)", k.maxd, k.att, k.diag, k.mit, k.team);
    void *args[] = {&a, &n_steps, &vcap, &bsz};
    return launch_resident(s, fn, grid, block, lds, args);
}

// Workgroups of this instantiation (block threads, lds bytes of dynamic LDS) one CU holds at once, as the runtime computes it from the
// kernel's registers and LDS (hipOccupancyMaxActiveBlocksPerMultiprocessor): what the host sizes a team launch's grid by - the members of a
// team wait for each other inside the launch, so a grid the chip cannot hold at once would be a team that is never complete.  Asked once
// per kernel and geometry; -1: the runtime would not say.
static int occupancy(const sf_sim *s, const RunKey &k, unsigned block, size_t lds)
{
    const void *fn = run_fn(k);
    const auto key = std::make_tuple(fn, block, lds);
    auto it = s->occ_cache.find(key);
    if (it != s->occ_cache.end()) return it->second;
    int occ = -1;
    if (!fn || allow_lds(s, fn, lds) != hipSuccess || hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, (int)block, lds) != hipSuccess) {
        (void)hipGetLastError();
        occ = -1;
    }
    s->occ_cache[key] = occ;
    return occ;
}

struct TeamGeo;
static int team_occupancy(const sf_sim *s, const TeamGeo &t, bool join);
// Geometry of a team launch (k_run<TEAM>, sf_run_kernels.h): waves per workgroup, list entries, bitmap rows a member keeps in LDS
// (0 = all), dynamic LDS, workgroup slots the chip holds at once, smallest team an environment needs.
struct TeamGeo { int waves, vcap, rcap, slots, t_min; size_t lds; bool ok; };
static TeamGeo team_geometry(const sf_sim *s)
{
    const Geo &g = s->g;
    TeamGeo t = {};
    const int th = g.LR * g.RB;
    if (g.ab != 1 || g.VW > 2 || g.TY > 64 || g.E > 1024 || g.dense) return t;       // (k_team_plan: one thread per environment; the split: one lane per tile row)
    if (g.VW == 1) {
        // rows of one word: every member keeps the whole grid's bitmaps.  Few environments (at most half as many as CUs: C5's 64): members
        // of 16 waves, one workgroup per CU - the CUs a team takes would idle otherwise; more: 8 waves, two workgroups per CU
        const bool roomy = g.E * 2 <= s->n_cu && g.H <= 16 * 64;
        t.waves = roomy ? 16 : 8; t.vcap = roomy ? 4096 : 1024; t.rcap = 0; t.t_min = 1;
        if ((g.H + t.waves * 64 - 1) / (t.waves * 64) * g.VW > 2) return t;       // (k_run<TEAM> is instantiated for 1 and 2 bitmap words per thread)
    } else {
        // rows of two words (2048-wide grids): a member keeps a window of rows; 16 waves, one workgroup per CU
        t.waves = 16; t.vcap = 2048; t.rcap = 1024 / th * th; t.t_min = (g.H + t.rcap - 1) / t.rcap;
        if (t.rcap < th || (t.rcap + t.waves * 64 - 1) / (t.waves * 64) * g.VW > 2) return t;
    }
    long long all_vec = (long long)g.H * g.PV;
    if (t.vcap > all_vec) t.vcap = (int)((all_vec + 63) / 64 * 64);
    t.lds = run_lds_bytes(g, t.waves, t.vcap, 1, t.rcap);
    if (t.lds > 160 * 1024 || t.t_min > kTeamMax || t.t_min > g.TY) return t;
    int per_cu = (int)((160 * 1024) / t.lds);
    if (per_cu * t.waves > 32) per_cu = 32 / t.waves;
    if (per_cu > 2) per_cu = 2;
    // ... and no more than the runtime says a CU holds of THIS kernel with this much LDS (registers count too): a team's members wait for
    // each other inside the launch, the grid must not be larger than what the chip holds at once
    const int occ = team_occupancy(s, t, false);
    if (occ == 0) return t;
    if (occ > 0 && occ < per_cu) per_cu = occ;
    t.slots = s->n_cu * per_cu;
    t.ok = (long long)g.E * t.t_min <= t.slots;
    return t;
}

// Workgroups per CU of the team kernel this geometry launches (the smaller figure of its instantiations with / without control lines inside
// the launch).  -1: the runtime would not say (the LDS formula stands).
static int team_occupancy(const sf_sim *s, const TeamGeo &t, bool join)
{
    const unsigned block = (unsigned)t.waves * 64;
    if (join) return occupancy(s, run_key(s->g, kRunJoin, 1, false), block, t.lds);
    const int words = run_words(t.rcap ? t.rcap : s->g.H, t.waves, s->g.VW);
    const int occ = occupancy(s, run_key(s->g, kRunTeam, words, false), block, t.lds);
    const int o2 = occ < 0 ? -1 : occupancy(s, run_key(s->g, kRunTeam, words, true), block, t.lds);
    return (o2 >= 0 && o2 < occ) ? o2 : occ;
}

// Teams that GROW inside the launch (k_run<TEAM = 2>, sf_run_kernels.h): one-word rows, one 16-wave workgroup per CU, every environment starts
// with ONE member; a workgroup whose environment is done (or that had none) joins the team of the running environment that would finish
// last, at that team's next cut (every `recut` updates).  Results never depend on who joined whom when.
static TeamGeo join_geometry(const sf_sim *s)
{
    const Geo &g = s->g;
    TeamGeo t = {};
    if (g.ab != 1 || g.VW != 1 || g.TY > 64 || g.H > 16 * 64 || g.E > 1024 || g.E > s->n_cu || g.dense || !g.diag) return t;
    t.waves = 16; t.vcap = 4096; t.rcap = 0; t.t_min = 1;
    const long long all_vec = (long long)g.H * g.PV;
    if (t.vcap > all_vec) t.vcap = (int)((all_vec + 63) / 64 * 64);
    t.lds = run_lds_bytes(g, t.waves, t.vcap, 1, 0);
    if (t.lds > 160 * 1024 || g.TY < 2) return t;
    if (team_occupancy(s, t, true) == 0) return t;      // (one 16-wave workgroup per CU: the kernel must fit a CU at all)
    t.slots = s->n_cu;
    t.ok = true;
    return t;
}
static int team_buffers(sf_sim *s, const TeamGeo &t)
{
    const Geo &g = s->g;
    if (!s->team_tab || s->team_slots < t.slots) {
        if (s->team_tab) { HIPCHK(hipFree(s->team_tab)); s->team_tab = nullptr; }
        { int rc = dev_alloc(s, &s->team_tab, (size_t)t.slots); if (rc) return rc; }
        s->team_slots = t.slots;
        s->team_plan_ones = 0;
    }
    if (!s->xg) {
        int rc = dev_alloc(s, &s->xg, (size_t)g.E * kTeamMax * 3); if (rc) return rc;
        rc = dev_alloc(s, &s->xbuf, (size_t)g.E * kTeamMax * 4 * team_xrow(g)); if (rc) return rc;
        rc = dev_alloc(s, &s->xdone, (size_t)2 * g.E + 1); if (rc) return rc;       // members that have left [E] | the teams' start words [E] | teams that started as one
        HIPCHK(hipMemsetAsync(s->xdone, 0, sizeof(uint32_t) * ((size_t)2 * g.E + 1), s->stream));
        rc = dev_alloc(s, &s->team_size, (size_t)g.E); if (rc) return rc;
        HIPCHK(hipHostMalloc(reinterpret_cast<void **>(&s->xerr_pinned), sizeof(uint32_t), hipHostMallocMapped));
        HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void **>(&s->xerr_mapped), s->xerr_pinned, 0));
        *s->xerr_pinned = 0;
        HIPCHK(hipMemsetAsync(s->xbuf, 0, (size_t)g.E * kTeamMax * 4 * team_xrow(g), s->stream));
    }
    return SF_OK;
}

// The fields of StepArgs every team launch (k_run<TEAM>) sets from the handle.  rcap: bitmap rows a member keeps (0 = all); cost: the cost array
// the launch reads and records, or null.
static void team_args(const sf_sim *s, StepArgs &a, int rcap, uint32_t *cost)
{
    a.cost = cost;
    a.team_tab = s->team_tab; a.xg = s->xg; a.xbuf = s->xbuf; a.xdone = s->xdone; a.xerr = s->xerr_mapped;
    a.xrow = team_xrow(s->g); a.team_rcap = rcap;
    // placement of the members: 0 (default) = the slots of one XCD, 1 = consecutive slots (eight XCDs in turn), 2 = as 0 but the
    // hand-off written through as if they were apart - results never depend on it (tests run all three)
    a.team_far = s->tune.v[SF_TUNE_TEAM_PLACEMENT] == 2;
    a.order = nullptr;
}

static int launch_k_run_join(sf_sim *s, StepArgs &a, int n_steps, const TeamGeo &t, bool eager)
{
    const Geo &g = s->g;
    { int rc = team_buffers(s, t); if (rc) return rc; }
    if (!s->xj) {
        int rc = dev_alloc(s, &s->xj, (size_t)3 * g.E + 2); if (rc) return rc;
        rc = dev_alloc(s, &s->xcut, (size_t)g.E); if (rc) return rc;
        rc = dev_alloc(s, &s->jlog, (size_t)1 + 3 * kJoinLog); if (rc) return rc;
    }
    HIPCHK(hipMemsetAsync(s->jlog, 0, sizeof(uint32_t), s->stream));
    s->jlog_valid = true;
    hipLaunchKernelGGL(k_team_plan, dim3(1), dim3(1024), 0, s->stream, g.E, t.slots, 1, 1, 0u, 0u, 1, s->run_cost, s->team_tab, s->team_size, s->xg, s->xdone, 0,
                       s->xj, s->xcut);
    s->team_plan_ones = 0;             // (this plan spreads the environments over the XCDs: not the table a launch of fixed teams of one keeps)
    team_args(s, a, 0, s->run_cost);
    a.xj = s->xj; a.xcut = s->xcut; a.tsize = s->team_size; a.jlog = s->jlog;
    // (k_team_plan's model of a team: the chain no member's update gets shorter than, what belonging to a team costs per update; eager - tests -:
    // every workgroup that is free joins whatever runs)
    // Where the newcomers come from: the environment's own XCD (default: the team's step boundaries and cuts stay in one L2 - measured on C3, 1000 updates:
    // teams spread over the XCDs pay ~12 k clocks per update for belonging, and every cut writes back and invalidates a whole L2 under 31 other
    // environments; 10.9 -> 12.7 us per update); SF_TUNE_TEAM_PLACEMENT 1 = from anywhere, 2 = the own XCD but every hand-off as if they were apart
    const int place = s->tune.v[SF_TUNE_TEAM_PLACEMENT];
    a.join_local = place == 1 ? 0 : (place == 2 ? 2 : 1);
    a.join_floor = eager ? 0 : 12000; a.join_ovh = eager ? 0 : (a.join_local == 1 ? 3000 : 12000);
    return launch_run(s, run_key(g, kRunJoin, 1, false), (unsigned)t.slots, (unsigned)t.waves * 64, t.lds, a, n_steps, t.vcap, 64);
}


// keep_cost: the launch neither reads nor records what the environments cost (the catch-up launch behind a windowed one)
static int launch_k_run_team(sf_sim *s, StepArgs &a, int n_steps, const TeamGeo &t, int t_min, int t_max, int steps_before, bool keep_cost = false)
{
    const Geo &g = s->g;
    { int rc = team_buffers(s, t); if (rc) return rc; }
    // what a member pays per step for belonging to a team (publish, wait for the slowest member, read: ~6.5 k clocks measured) and the
    // latency chain no member's step gets shorter than (~12 k clocks), in the unit of the cost array
    const uint32_t ovh = (uint32_t)((long long)(steps_before > 0 ? steps_before : 0) * 6500 / 16);
    const uint32_t floor_c = (uint32_t)((long long)(steps_before > 0 ? steps_before : 0) * 12000 / 16);
    // (the plan also clears the granules, the "left" counters and the cost array it has read: the members add their clocks)
    // Teams of ONE (C4's young fires in the driver's window): the plan does not depend on what anything cost, teams of one touch neither
    // the granules nor the counters and store their cost - the table of the launch before stands, and the call is one launch instead of two
    // (k_team_plan + the gap behind it: ~5 us of a 57 us call).
    const int scatter = s->tune.v[SF_TUNE_TEAM_PLACEMENT] == 1 ? 1 : 0;
    const long long ones_key = (t_min == 1 && t_max == 1) ? 1 + (long long)scatter + 2ll * t.slots + ((long long)g.E << 32) : 0;
    if (!ones_key || s->team_plan_ones != ones_key)
        hipLaunchKernelGGL(k_team_plan, dim3(1), dim3(1024), 0, s->stream, g.E, t.slots, t_min, t_max, ovh, floor_c, scatter,
                           s->run_cost, s->team_tab, s->team_size, s->xg, s->xdone, keep_cost ? 1 : 0, (uint32_t *)nullptr, (unsigned long long *)nullptr);
    s->team_plan_ones = ones_key;
    team_args(s, a, t.rcap, keep_cost ? nullptr : s->run_cost);
    const int words = run_words(t.rcap ? t.rcap : g.H, t.waves, g.VW);
    return launch_run(s, run_key(g, kRunTeam, words, a.mit != nullptr), (unsigned)t.slots, (unsigned)t.waves * 64, t.lds, a, n_steps, t.vcap, 64);
}

// ----------------------------------------------------------------------------- the launch plan of a sf_step call
// Which launches a call makes, decided from the handle alone (plan_step: nothing here changes it): the per-step launches - k_select + k_step,
// one fused launch per step or the per-cell kernel - or the resident launch k_run (nw > 0), with k_win in front of it or not.
struct StepPlan {
    bool generic, fused;               // per-step launches: the per-cell kernel / one fused launch per step
    int nw, vcap, bsz;                 // the resident launch: waves per workgroup (0: the per-step launches), vector list entries, vectors per batch
    size_t lds;
    int win;                           // StepArgs::win
    bool result;                       // the resident launch leaves the result block behind
    TeamGeo tgeo, jgeo;
    bool team_forced, team_wide, team_auto;
    bool win_first;                    // k_win in front of k_run (more environments than CUs, young fires)
    bool win_only;                     // ... and nothing is left behind it for sure: no k_run launch
    bool balance;                      // segments that start their environments most expensive first (k_order)
    bool team_any, team_segments;
};

// The choices that follow from win_first (plan_step; again where the call cannot have the window phase after all).
static void plan_modes(const sf_sim *s, StepPlan &p, int n_steps)
{
    const int seg_knob = s->tune.v[SF_TUNE_RUN_SEGMENT];
    // More environments than the chip holds workgroups: the launch would end with whatever large fire happened to start late.
    // The rollout is cut into segments, and every segment starts its environments in the order of what they cost in the one
    // before (k_order: most expensive first) - the tail of a segment is then made of the cheapest environments.
    p.balance = seg_knob > 0 && s->g.E > s->n_cu * (p.nw <= 8 ? 2 : 1) && !p.win_first;       // (with every environment resident from the start there is nothing to order; nor behind k_win: the few environments that have updates left)
    // Teams (k_run<TEAM>): forced by sf_set_tuning; always on grids of two-word rows; on one-word rows in long calls, which are then
    // cut into segments like above - the first one runs one workgroup per environment and records what every environment costs,
    // the following ones size the teams from that (k_team_plan) and cut the bands where the fires are by then.
    p.team_any = (p.team_forced || p.team_wide || p.team_auto) && p.bsz == 64 && !p.win_first;      // (behind k_win: ONE launch of the plain kernel for what is left - found by the soak, world 6005034: teams sized by cost cut the call into segments, and every segment's launch made the left-over updates again)
    p.team_segments = p.team_any && seg_knob > 0 && !p.balance;
    p.win_only = false;
    if (p.win_first) {
        // Is anything left for sure not?  A fire that spans F cells (rows and columns alike: one cell after sf_reset, a cell more per side and
        // update, fire.py:163-234) sits in a window placed to the row and - where a window placed to the vector may not hold it for the call -
        // around the middle of the (F + 14) / 16 + 1 vectors it can straddle at worst (run_window, PL4): (64 - F) / 2 rows and 32 - 8 x vectors
        // columns lie between it and the window's ring on every open side, and it needs one per update (+ 1: the ring itself).
        const int F = s->fire_rows, wv = (F + 14) / 16 + 1;
        const int room = wv > 3 ? 0 : std::min((64 - F) / 2, 32 - 8 * wv);
        p.win_only = n_steps + 1 <= room && p.win == 1;      // (SF_TUNE_RUN_WINDOW = k > 1 leaves the window after k updates: tests)
    }
}

// lines: control lines come inside the launch (sf_step_mitigated).
static StepPlan plan_step(const sf_sim *s, int n_steps, bool lines)
{
    StepPlan p = {};
    const Geo &g = s->g;
    const Tuning &tn = s->tune;
    // run(1) loops: after two step(1) + status pairs in a row (sf_sim::step1_polls) the single update runs as the resident launch
    const bool polled = n_steps == 1 && !lines && !s->last_was_step1 && s->step1_polls >= 2;
    const long long n_wave_tiles = (long long)g.E * g.TY * g.TX;
    // few tiles: one fused launch per step; many: select the live tiles first, then persistent waves
    // (measured crossover on 1024^2 environments: 16 envs = 8192 tiles fused 11.2 vs 13.3 us, 32 envs 14.8 vs 14.0 us)
    p.fused = s->fused_mode == 1 || (s->fused_mode < 0 && n_wave_tiles <= 12288);
    p.generic = g.ab > 1 || s->generic;
    p.win = tn.v[SF_TUNE_RUN_WINDOW] < 0 ? 0 : tn.v[SF_TUNE_RUN_WINDOW];
    // Environment-resident launch (k_run): all n steps of an environment in one workgroup.  Not with the
    // per-step by-products (spread graph, history) and not for the wide sprite planes.
    if (!p.generic && !(s->graph_on && s->parents) && !s->history && s->fused_mode != 0 && s->fused_mode != 1) {
        const int waves_knob = tn.v[SF_TUNE_RUN_WAVES], envs_knob = tn.v[SF_TUNE_RUN_MIN_ENVS], vcap_knob = tn.v[SF_TUNE_RUN_VCAP];
        int nw = waves_knob < 1 ? 1 : (waves_knob > 16 ? 16 : waves_knob);
        const int need = (g.H + 63) / 64;                     // a thread per bitmap row is all the interest pass can use
        if (nw > need) nw = need;
        const int min_nw = (int)(((long long)g.H * g.VW + 64 * kRunMaxD - 1) / (64 * kRunMaxD));   // rows per thread x words per row <= kRunMaxD
        if (nw < min_nw) nw = min_nw;
        long long all_vec = (long long)g.H * g.PV;
        int vcap = vcap_knob < 64 ? 64 : vcap_knob;
        if (vcap > all_vec) vcap = (int)((all_vec + 63) / 64 * 64);
        size_t lds = run_lds_bytes(g, nw, vcap);
        // More environments than CUs (the throughput regime): a CU works through several environments one after the other, and a
        // workgroup of 16 waves mostly waits.  Half the waves and a shorter vector list (longer ones are taken in chunks): two
        // workgroups fit the 160 KB of LDS and fill each other's gaps.
        // Not while every fire is surely young (the bound on the fires' rows since the last reset says this call ends with every fire inside a
        // window of 64 rows): an 8-wave workgroup holds a window of 32 rows only, a fire 33 rows tall leaves it for the general loop -
        // measured on 1024 environments in the driver's window: 11.3 us per update in 8-wave workgroups, 9.6 in 16-wave ones.
        // ... and while the fires may still fit their windows (the bound on the fires' rows since the last reset) the window phase runs as a
        // kernel of its own in front, k_win: 63 VGPRs and 69 KB of LDS - two 16-wave workgroups to a CU, whose dependent chains fill each other's
        // gaps (sf_run_kernels.h).  The k_run launch behind it makes what is left - the updates of fires that outgrew their windows - in the
        // 8-wave workgroups of this regime.  (Round 5 kept 16-wave k_run workgroups in rounds of 256 while every fire was surely young: 9.8 us per
        // update on 1024 environments in the driver's window.)  SF_TUNE_RUN_COMPACT = 2: the window kernel in front whatever the batch size (tests).
        // (k_win needs the window phase: SF_TUNE_RUN_WINDOW > 0)
        p.win_first = p.win != 0 && tn.v[SF_TUNE_RUN_COMPACT] != 0 && (g.E > s->n_cu || tn.v[SF_TUNE_RUN_COMPACT] == 2) && !lines && g.VW == 1 &&
                      g.H >= 64 && g.H <= 1024 && g.PV >= 4 && !g.dense && s->fire_rows > 0 && s->fire_rows <= 62 && n_steps <= 64 && !tn.set[SF_TUNE_RUN_WAVES] &&
                      g.diag && (tn.v[SF_TUNE_RUN_TEAM] == 0 || tn.v[SF_TUNE_RUN_TEAM] == 1) && s->fused_mode != 2;
        // (the launch behind k_win: while every fire surely ends the call inside 64 rows, 16-wave workgroups - an environment whose fire reached the
        // ring of a window placed to the vector gets a new window of 64 rows around where the fire stands now, 2 us per update instead of the
        // general loop's 6 in an 8-wave workgroup; everybody else's workgroup returns at once)
        const bool all_young = tn.v[SF_TUNE_RUN_WINDOW] != 0 && s->fire_rows > 0 && s->fire_rows + 2LL * n_steps <= 60;
        if (tn.v[SF_TUNE_RUN_COMPACT] && g.E > s->n_cu && nw > 8 && min_nw <= 8 && !tn.set[SF_TUNE_RUN_WAVES] && !all_young) {
            const int vcap2 = vcap > 1024 ? 1024 : vcap;
            const size_t lds2 = run_lds_bytes(g, 8, vcap2);
            if (lds2 <= 80 * 1024) { nw = 8; vcap = vcap2; lds = lds2; }
        }
        const bool fits = nw <= 16 && g.W <= 4096 && g.H <= 65535 && g.VW <= kRunMaxD && lds <= 160 * 1024;
        // automatic: multi-step calls on grids up to 1024 cells wide (measured on 1024^2, 1 .. 1024 environments: 1.2 - 1.4 x
        // faster than the per-step launches at every batch size; on 2048^2 an environment's fire is too much work for the one
        // CU that owns it and the per-step launches, which spread tiles over the whole chip, win by 1.4 - 2 x)
        // ... which the team launch (k_run<TEAM>: several workgroups per environment, each with the bitmaps of its own band of rows) takes away:
        // grids of two-word rows run there in the automatic mode too
        p.tgeo = team_geometry(s);
        p.jgeo = join_geometry(s);
        const int team_knob = tn.v[SF_TUNE_RUN_TEAM];
        p.team_forced = p.tgeo.ok && team_knob >= 2 && team_knob <= kTeamMax && team_knob <= g.TY && team_knob >= p.tgeo.t_min && (long long)g.E * team_knob <= p.tgeo.slots;
        // (control lines inside the launch: every row needs an owner, so the members' windows of rows have to hold the whole grid between them)
        if (lines && p.tgeo.rcap > 0 && (long long)team_knob * p.tgeo.rcap < g.H) p.team_forced = false;
        p.team_wide = p.tgeo.ok && team_knob != 1 && g.VW == 2 && !lines;      // (control lines inside the launch: every row needs an owner, a window of rows leaves some without)
        const bool wanted = s->fused_mode == 2 || ((n_steps >= 2 || lines || polled) && (g.VW == 1 || p.team_wide) && g.E >= envs_knob);
        // Rows of one word: NOT automatic.  Measured on C3 / C5 (profiles/r03_team/): a member's step is a latency chain that does not get
        // shorter with half the rows, and a team's step boundary costs 5 - 10 k clocks (publish, wait for the slowest member, read), so
        // teams of 8-wave members lose to one 16-wave workgroup per environment until a fire is far larger than these get (C3: 11.0 ->
        // 15.0 us per step with teams sized by cost).  sf_set_tuning(SF_TUNE_RUN_TEAM, -1) turns the cost-sized teams on.
        // Except where most CUs idle anyway: with at most a quarter as many environments as CUs the members are 16-wave workgroups on CUs
        // of their own, and teams sized by cost are automatic from the second 64-step segment on (C5, 64 environments: 18.2 -> 17.3 us per
        // step; 128 environments: 9.9 -> 10.6, not automatic).  The gain is small because a member's step is never shorter than the ~12 k
        // clocks of the chain and the team kernel itself is ~10 % slower for an environment that stays whole.
        p.team_auto = p.tgeo.ok && g.VW == 1 && g.E < p.tgeo.slots && (team_knob == -1 || (team_knob == 0 && g.E >= 2 && g.E * 4 <= s->n_cu && p.tgeo.waves == 16));
        // (one environment - FireSimulation.run(), C2 -: its fire fits one workgroup for hundreds of steps, and the segments of a team rollout -
        // a plan, a prologue that reads the bitmaps and an epilogue per launch - cost a lone young fire 16 %: 3.23 against 3.74 us per step)
        if (fits && wanted) { p.nw = nw; p.vcap = vcap; p.lds = lds; }
    }
    const int bsz_knob = tn.v[SF_TUNE_RUN_BATCH];       // vectors per batch (<= 64)
    p.bsz = bsz_knob < 8 ? 8 : (bsz_knob > 64 ? 64 : bsz_knob);
    p.result = tn.v[SF_TUNE_RUN_RESULT] != 0;           // the launch leaves the result block behind (every workgroup counts its own environment when its steps are done)
    plan_modes(s, p, n_steps);
    return p;
}

// One launch of the resident rollout's segment loop: how many updates, and which kernel makes them.
struct Segment {
    int n;                             // updates
    int recut;                         // StepArgs::team_recut
    bool join, team;                   // k_run<TEAM = 2> / k_run<TEAM = 1> (else the plain kernel)
    bool windows;                      // the team launch leaves what did not fit its windows of rows to a second launch
    int t_min, t_max;                  // team sizes (k_team_plan)
    int team_max;                      // sf_sim::last_team_max
};

// The segment of a resident rollout that starts after `done` of its n_steps updates.
static Segment plan_segment(const sf_sim *s, const StepPlan &p, int n_steps, int done, bool lines)
{
    const Geo &g = s->g;
    const Tuning &tn = s->tune;
    const TeamGeo &tgeo = p.tgeo;
    const int seg_knob = tn.v[SF_TUNE_RUN_SEGMENT];
    Segment sg = {};
    sg.n = p.balance && n_steps - done > seg_knob + seg_knob / 2 ? seg_knob : n_steps - done;
    // (two-word rows: twice the segment - every launch costs a plan, a prologue that reads the environment's whole bitmap and an
    // epilogue; measured on C4's share: 64 / 128 / 256 steps per launch = 26.3 / 26.1 / 26.8 us per step - the cuts have to follow the fires)
    // (one-word rows, teams sized by cost: C5 10.56 / 10.23 / 10.31 us per step with 64 / 128 / 256)
    const int tseg = (p.team_wide || p.team_auto) && !p.team_forced ? 2 * seg_knob : seg_knob;
    // Teams of a fixed size - forced, or every workgroup slot taken at the smallest size (C4's share: 128 x 2 = 256) -: nothing to
    // plan between segments, so the rollout is ONE launch and the teams cut their bands anew inside it (k_run, team_recut).  Cut
    // into launches a rollout lasts the sum of the launches' slowest environments instead of the slowest sum (measured on C4's
    // share: + 12 %, profiles/segment_penalty_probe.py) and pays a plan, a prologue and an epilogue per segment.
    const int tk = tn.v[SF_TUNE_RUN_TEAM];
    const bool team_fixed = p.team_segments && tn.v[SF_TUNE_TEAM_RECUT] != 0 && !(tgeo.rcap > 0 && tk == -1) &&
                            (long long)tgeo.t_min * (tgeo.rcap ? tgeo.rcap : g.H) >= g.H &&
                            (p.team_forced || (p.team_wide && tgeo.slots - (long long)g.E * tgeo.t_min < (g.E + 3) / 4));
    if (p.team_segments && !team_fixed && n_steps - done > tseg + tseg / 2) sg.n = tseg;
    sg.recut = team_fixed ? (p.team_forced ? 2 * seg_knob : tseg) : 0;
    // Two-word rows, YOUNG fires: one member holds any fire whose rows (+ what it can grow during the launch + the cut's margins)
    // fit its window of team_rcap rows - and a young fire cut in two only pays the step boundary (C4's share, the driver's
    // window: 8.7 us per step with two members).  The host knows an upper bound without asking the device: a fire spans one row
    // after sf_reset and advances one row per update at most.  A call that ends with every fire still under 480 rows gives every
    // environment ONE member.
    bool young = false;
    if (p.team_wide && !p.team_forced && tk == 0 && tgeo.rcap > 0 && s->fire_rows > 0) {
        // (cut_bands: the fire's tile rows, + ceil((updates + 1) / tile height) + 1 tile rows either side)
        const long long room = (long long)tgeo.rcap - s->fire_rows - 2LL * done - 7LL * g.LR * g.RB - 2;
        const long long fit = room / 2;              // updates the window is sure to hold
        // (only where the whole call stays young - measured on C4's share: one member for the first ~ 380 of 1000 updates and two
        // for the rest loses to two members throughout, 23.5 against 21.9 us per step; the driver's 20 after 5: 7.0 against 8.7)
        // (C4's share, calls of 60 / 100 / 150 / 250 / 350 updates after 20: one member 7.8 / 8.3 / 9.6 / 11.9 / 15.8 us per step, two 9.1 / 9.3 / 10.8 / 12.1 / 14.1)
        if (done == 0 && fit >= n_steps && s->fire_rows + 2LL * n_steps <= 480) { young = true; sg.n = n_steps - done; sg.recut = 0; }
    }
    // Teams that grow inside the launch (k_run<TEAM = 2>): long calls on one-word rows with at most one environment per CU - the CUs of
    // fires that go out (C3: three quarters of them over 1000 updates) join the fires that are left.  SF_TUNE_RUN_JOIN.
    const int join_knob = tn.v[SF_TUNE_RUN_JOIN];
    const int join_min = join_knob > 1 ? join_knob : (join_knob < -1 ? -join_knob : 192);
    // (Measured on C3 over 1000 updates with 256 / 192 / 128 / 96 / 64 environments: 10.8 -> 10.0, 10.5 -> 9.4, 9.8 -> 8.8, 9.6 -> 8.7, 9.5 -> 8.6 us per update -
    // 32 / 16 / 8 / 2 environments: 8.6 -> 8.1, 8.2 -> 7.6, 7.8 -> 7.2, 7.3 -> 7.1 - from 64 down against the teams sized by cost between segments, which
    // this replaces wherever it applies (they remain for calls with control lines inside the launch: C5);
    // ONE environment - FireSimulation.run(), C2 - keeps the plain kernel: its fire is young for hundreds of updates, and this kernel has no window
    // phase - measured on C2, 300 updates after 20: 5.1 against 6.0 us per update.  The knob set by hand wins.)
    sg.join = !p.win_first && join_knob != 0 && !p.team_forced && !p.team_wide && ((g.E >= 2 && !tn.set[SF_TUNE_RUN_TEAM]) || tn.set[SF_TUNE_RUN_JOIN]) && !p.balance && !lines && p.bsz == 64 && done == 0 &&
              n_steps >= join_min && !tn.set[SF_TUNE_RUN_WAVES] && !tn.set[SF_TUNE_RUN_VCAP] && p.jgeo.ok;
    if (sg.join) { sg.n = n_steps; sg.recut = seg_knob >= 4 ? seg_knob / 2 : 2; sg.team_max = kTeamMax; }
    sg.team = !p.win_first && !sg.join && p.team_any && !p.balance && (p.team_forced || p.team_wide || (s->cost_steps > 0 && n_steps - done >= seg_knob / 2));
    if (sg.team) {
        sg.team_max = p.team_forced ? tk : (kTeamMax < g.TY ? kTeamMax : g.TY);
        // Windows of rows (two-word rows): a fire that is small enough runs in ONE workgroup with the window around it, the largest ones
        // get up to four; whoever was given too small a team for its fire (known only on the device) is left untouched, noted in
        // todo[] and done by the second launch - two members, half the grid each, which always fits.
        // (Only with SF_TUNE_RUN_TEAM = -1: measured on C4's share, 128 x 2048^2, the cost-sized teams lose to two members for every
        // environment - 55 against 37 us per step around step 1000 - because teams of different sizes do not pack into the slots of one
        // XCD and their step boundaries then go through memory, 16 k instead of 12 k clocks each.)
        sg.windows = tgeo.rcap > 0 && !p.team_forced && tk == -1;
        sg.t_min = young ? 1 : (p.team_forced ? tk : (sg.windows ? 1 : tgeo.t_min));
        sg.t_max = young ? 1 : (team_fixed && !p.team_forced ? tgeo.t_min : sg.team_max);
    }
    return sg;
}

// ----------------------------------------------------------------------------- running the plan
// The fields of StepArgs every launch of a handle's kernels takes from the handle as it stands (a launch sets the rest).
static StepArgs handle_args(const sf_sim *s)
{
    StepArgs a;
    memset(&a, 0, sizeof a);
    a.g = s->g; a.status = s->status; a.age = s->age; a.cells = s->cells; a.burn = s->burn; a.rt = s->rt;
    a.commit = s->commit; a.tmp = s->tmp; a.flags = s->flags; a.tflags = s->tflags; a.tile_list = s->tile_list;
    a.n_active = s->n_active; a.seam = s->seam; a.settled = s->settled; a.tdirty = s->tdirty; a.thist = s->thist; a.vbits = s->vbits;
    a.launch = 0; a.from_commit = 1; a.ring = s->ring;
    return a;
}

// The resident rollout: k_win in front (p.win_first), then the segment loop.
static int run_resident(sf_sim *s, const StepPlan &p, StepArgs &a, int n_steps, bool row_was_fresh)
{
    const Geo &g = s->g;
    const int32_t *mit_dev = a.mit;
    const int mit_k = a.mit_k;
    if (p.result) {
        if (s->tdirty_all) HIPCHK(hipMemsetAsync(s->tdirty, 1, s->n_tiles_max, s->stream));
        s->tdirty_all = false;
    }
    a.cost = s->run_cost;
    s->last_team_max = 0;
    if (p.win_first) {
        // k_win: every environment's updates inside its window; what is left goes to s->todo
        const size_t wlds = (win_lds_bytes(16) + 15) / 16 * 16 + kRunCtl * 4;
        a.todo_out = s->todo; a.order = nullptr;
        a.row_valid = (row_was_fresh && p.result) ? 1 : 0;
        // (two counts that take turns, both zero to begin with: every k_win clears the one its successor appends to)
        if (!s->todo_cnt) { int rc0 = dev_alloc(s, &s->todo_cnt, (size_t)16); if (rc0) return rc0; HIPCHK(hipMemsetAsync(s->todo_cnt, 0, 16 * sizeof(uint32_t), s->stream)); }
        a.todo_cnt = s->todo_cnt + (s->win_seq & 1); a.todo_cnt_next = s->todo_cnt + ((s->win_seq + 1) & 1); a.todo_list = s->run_order;      // (the order array: no ordered segments in a call k_win goes in front of)
        s->win_seq++;
        if (p.result) { a.res_block = s->status_block; a.res_elapsed = s->elapsed_dev; a.res_sink = s->sink; }
        const void *wk = g.att ? reinterpret_cast<const void *>(k_win<1>) : reinterpret_cast<const void *>(k_win<0>);
        void *args[] = {&a, &n_steps};
        { int rc0 = launch_resident(s, wk, (unsigned)g.E, 1024, wlds, args); if (rc0) return rc0; }
        a.todo_out = nullptr; a.res_block = nullptr; a.res_elapsed = nullptr; a.res_sink = nullptr;
        s->last_launches++;
        a.todo = s->todo; a.todo_skip = 1;
    }
    for (int done = 0; done < n_steps && !p.win_only;) {
        const Segment sg = plan_segment(s, p, n_steps, done, mit_dev != nullptr);
        a.team_recut = sg.recut;
        if (p.balance) {
            hipLaunchKernelGGL(k_order, dim3(1), dim3(1024), 0, s->stream, g.E, (const uint32_t *)s->run_cost, s->run_order);
            a.order = s->run_order;
        }
        a.mit = mit_dev ? mit_dev + (size_t)done * g.E * mit_k * 3 : nullptr;
        if (p.result && done + sg.n == n_steps) { a.res_block = s->status_block; a.res_elapsed = s->elapsed_dev; a.res_sink = s->sink; }
        // (the block is current for the call's FIRST launch only if it was when the call started - and only that launch may go by it: the
        // launches before the last one of a call do not write it)
        a.row_valid = (row_was_fresh && done == 0 && !p.win_first && p.result) ? 1 : 0;
        if (sg.join) {
            int rc0 = launch_k_run_join(s, a, sg.n, p.jgeo, s->tune.v[SF_TUNE_RUN_JOIN] < 0);
            if (rc0) return rc0;
        } else if (sg.team) {
            a.todo = nullptr; a.todo_out = sg.windows ? s->todo : nullptr;
            int rc0 = launch_k_run_team(s, a, sg.n, p.tgeo, sg.t_min, sg.t_max, s->cost_steps);
            if (rc0) return rc0;
            if (sg.windows) {
                a.todo = s->todo; a.todo_out = nullptr; a.row_valid = 0;      // (the launch in front may have changed what the block counts)
                rc0 = launch_k_run_team(s, a, sg.n, p.tgeo, p.tgeo.t_min, p.tgeo.t_min, 0, true);
                if (rc0) return rc0;
                a.todo = nullptr;
            }
            a.cost = s->run_cost;
        } else {
            int rc0 = launch_run(s, run_key(g, kRunPlain, run_words(g.H, p.nw, g.VW), a.mit != nullptr), (unsigned)g.E, (unsigned)p.nw * 64, p.lds, a,
                                 sg.n, p.vcap, p.bsz);
            if (rc0) return rc0;
            if (g.VW > 1) s->vbits_fl_valid = false;
        }
        if (sg.join || sg.team) s->last_team_max = sg.team_max;
        s->cost_steps = sg.n;
        done += sg.n;
        s->last_launches++;
    }
    if (p.win_only) s->cost_steps = n_steps;
    s->status_fresh = p.result;
    s->tiles_valid = false;                // the tile activity map / seam planes are not kept by k_run
    s->last_kind = p.win_first ? 4 : 2;
    return SF_OK;
}

// Updates as planned (enqueue layer): the buffers their launches need, then the resident rollout or the per-step loop.  mit_dev / mit_k:
// control lines inside the resident launch (p planned with lines).  t0 (may be null): an event recorded in front of the step launches,
// behind the buffers' rebuilds - where a timed call's GPU time starts.
static int enqueue_steps(sf_sim *s, StepPlan p, int n_steps, const int32_t *mit_dev, int mit_k, hipEvent_t t0)
{
    const Geo &g = s->g;
    const Tuning &tn = s->tune;
    const bool row_was_fresh = s->status_fresh;      // the result block on the device is current as this call starts
    s->status_fresh = false;
    s->last_launches = 0;
    const int n_requested = n_steps;
    if (n_steps != 1 || mit_dev || s->last_was_step1) s->step1_polls = 0;       // (another kind of call, or nobody looked at the last update's result)
    if (p.nw) {
        int rc0 = ensure_commit(s);            // k_run starts from commit[] and leaves the new states there
        if (rc0) return rc0;
        // (a team launch reads all three planes of the vector bitmap; a launch of the plain kernel on rows of several words has kept only the first)
        if ((p.team_forced || p.team_wide || p.team_auto) && !s->vbits_fl_valid) s->vbits_valid = false;
        rc0 = ensure_vbits(s);
        if (rc0) return rc0;
        rc0 = ensure_bl(s);
        if (rc0) return rc0;
        if (p.win) {                           // the window phase reads the cell-major copy of the R table
            rc0 = ensure_rtc(s);
            if (rc0 == SF_ENOTSUP) { p.win = 0; p.win_first = false; plan_modes(s, p, n_steps); }      // (no memory for the cell-major table: this call goes without the window phase)
            else if (rc0) return rc0;
        }
    } else if (!p.generic) {
        int rc0 = ensure_tiles(s);
        if (rc0) return rc0;
    }
    if (!p.nw) { int rc0 = ensure_rm(s); if (rc0) return rc0; }
    StepArgs a = handle_args(s);
    a.counters = s->counters_on ? s->counters : nullptr;
    a.parents = s->graph_on ? s->parents : nullptr;
    // (0 ms: a team whose members do not all arrive at its start in the same instant starts as one at once - tests of that path)
    a.team_timeout = 100000ull * (unsigned long long)(tn.v[SF_TUNE_TEAM_TIMEOUT_MS] == 0 ? 2000 : (tn.v[SF_TUNE_TEAM_TIMEOUT_MS] < 1 ? 1 : tn.v[SF_TUNE_TEAM_TIMEOUT_MS]));
    a.team_start_timeout = tn.v[SF_TUNE_TEAM_TIMEOUT_MS] == 0 ? 0ull : a.team_timeout;
    a.mit = mit_dev; a.mit_k = mit_k;
    a.win = p.win;
    if (p.nw && p.win) { a.rtc = s->rtc; a.win_hint = s->win_hint; }
    if (t0) HIPCHK(hipEventRecord(t0, s->stream));
    if (p.nw) {
        int rc0 = run_resident(s, p, a, n_steps, row_was_fresh);
        if (rc0) return rc0;
        n_steps = 0;                           // nothing left for the per-step loop
    } else if (n_steps > 0) {
        s->vbits_valid = false;                // the per-step kernels do not keep the vector bitmap
        if (p.generic) s->tiles_valid = false; // nor does the per-cell kernel keep the tile maps
        s->last_kind = p.generic ? 3 : (p.fused ? 1 : 0);
    }
    const long long n_wave_tiles = (long long)g.E * g.TY * g.TX;
    const dim3 sel_grid((unsigned)((n_wave_tiles + kSelectThreads - 1) / kSelectThreads));
    const int waves_per_cu = tn.v[SF_TUNE_WAVES_PER_CU];   // persistent grid of k_step
    long long want = p.fused ? (n_wave_tiles + kWaves - 1) / kWaves : (long long)s->n_cu * waves_per_cu / kWaves;
    if (!p.fused && want * kWaves > n_wave_tiles) want = (n_wave_tiles + kWaves - 1) / kWaves;
    const dim3 step_grid((unsigned)(want < 1 ? 1 : want));
    const StepKernel kern = pick_step_kernel(g.RB, p.fused);
    const dim3 cell_grid((unsigned)((g.W + 255) / 256), (unsigned)g.H, (unsigned)g.E);
    for (int i = 0; i < n_steps; ++i) {
        a.launch = s->seq;
        a.from_commit = s->committed ? 1 : 0;
        a.ring = s->ring;
        if (p.generic) {
            if (g.ab == 1) hipLaunchKernelGGL(k_step_cells<uint8_t>, cell_grid, dim3(256), 0, s->stream, a);
            else if (g.ab == 2) hipLaunchKernelGGL(k_step_cells<uint16_t>, cell_grid, dim3(256), 0, s->stream, a);
            else hipLaunchKernelGGL(k_step_cells<uint32_t>, cell_grid, dim3(256), 0, s->stream, a);
        } else {
            if (!p.fused) hipLaunchKernelGGL(k_select, sel_grid, dim3(kSelectThreads), 0, s->stream, a);
            hipLaunchKernelGGL(kern, step_grid, dim3(kWaves * 64), (size_t)kWaves * g.lds_wave_bytes, s->stream, a);
            s->ring ^= 1;
        }
        if (a.parents) {
            if (p.generic || p.fused) hipLaunchKernelGGL(k_graph_pass, cell_grid, dim3(256), 0, s->stream, a);
            else hipLaunchKernelGGL(k_graph_pass_tiles, dim3((unsigned)(s->n_cu * 8)), dim3(256), 0, s->stream, a);
        }
        if (s->history) hipLaunchKernelGGL(k_record, cell_grid, dim3(256), 0, s->stream, g, (const uint8_t *)s->status,
                                           (const EnvState *)(s->tmp + (size_t)(a.launch & 1) * g.E), s->history, s->history_cap);
        s->seq = (s->seq + 1) % 6;
        s->committed = false;
    }
    if (s->fire_rows > 0) { const long long fr = (long long)s->fire_rows + 2LL * n_requested; s->fire_rows = fr > g.H ? g.H : (int)fr; }
    s->last_was_step1 = n_requested == 1 && !mit_dev;
    // no commit here: the states stay in the rings until something asks for them (ensure_commit)
    return SF_OK;
}

// What the updates of every stepping call go through (enqueue layer).  Recording off (sf_enable_arrival): as planned, nothing else.
// Recording on: in pieces of at most max_fire_duration - of even length, each planned as a call of its length would be (a piece of the
// point block with it) and followed by the arrival pass -, so that every sprite is still in the masks when a pass looks (DESIGN.md
// section 17).  hold: the caller makes the closing pass itself (the scatter + step pairs of enqueue_pair): a pass every
// max_fire_duration updates only.  t0 then stands in front of all the pieces.
static int enqueue_call(sf_sim *s, const StepPlan &p, int n_steps, const int32_t *mit_dev, int mit_k, bool hold, hipEvent_t t0)
{
    if (!s->wind_sched.empty()) {          // a wind schedule is set: the tables that are due, in front of the call's first piece
        int rc0 = wind_sched_pass(s);
        if (rc0) return rc0;
    }
    if (!s->arrival1) return enqueue_steps(s, p, n_steps, mit_dev, mit_k, t0);
    const Geo &g = s->g;
    int rc = SF_OK, launches = 0;
    if (t0 && hipEventRecord(t0, s->stream) != hipSuccess) rc = fail(SF_EHIP, "sf_step: hipEventRecord failed");
    for (int done = 0; done < n_steps && !rc;) {
        if (s->arr_pending >= g.md) { rc = arrival_pass(s); continue; }      // (a call that failed half way left them behind)
        const int room = g.md - s->arr_pending;
        const int pieces = (n_steps - done + room - 1) / room;
        const int c = hold ? std::min(n_steps - done, room) : (n_steps - done + pieces - 1) / pieces;
        const StepPlan pc = c == n_steps ? p : plan_step(s, c, mit_dev != nullptr);
        if (mit_dev && !pc.nw) { rc = fail(SF_EHIP, "sf_step_mitigated: a piece of %d updates was not planned as a resident launch", c); break; }
        rc = enqueue_steps(s, pc, c, mit_dev ? mit_dev + (size_t)done * g.E * mit_k * 3 : nullptr, mit_k, nullptr);
        launches += s->last_launches;
        s->arr_pending += c;
        done += c;
        if (!rc && (!hold || s->arr_pending >= g.md)) rc = arrival_pass(s);      // behind every piece; a caller that holds: every md updates
    }
    s->last_launches = launches;
    s->last_was_step1 = n_steps == 1 && !mit_dev;
    return rc;
}

// Plan + enqueue: n plain updates (enqueue layer; none: nothing).
static int step_impl(sf_sim *s, int n_steps, bool hold, hipEvent_t t0)
{
    return n_steps == 0 ? SF_OK : enqueue_call(s, plan_step(s, n_steps, false), n_steps, nullptr, 0, hold, t0);
}

// sf_step / sf_step_timed / sf_step_mitigated without points (call layer behind their argument checks).  No updates: the handle's
// readiness is still looked at, and nothing else happens - a closed loop keeps running.
static int step_call(sf_sim *s, const char *who, int n_steps, float *ms)
{
    if (n_steps < 0) return fail(SF_EINVAL, "%s: n_steps must be >= 0", who);
    if (ms) *ms = 0.f;
    if (n_steps == 0) return check_ready(s, who, kNeedRt | kNeedReset);
    { int rc = begin_call(s, who, kNeedRt | kNeedReset); if (rc) return rc; }
    { int rc = step_impl(s, n_steps, false, ms ? s->ev0 : nullptr); if (rc) return rc; }
    return finish_call(s, who, !s->async, ms);
}

// The per-update history FireSimulation._save_data appends to fire_map.npy (simulation.py:548-549,
// 887-959: int8 [T, H, W], one map after every executed update), recorded on the device.
extern "C" int sf_enable_history(sf_sim *s, int32_t capacity)
{
    if (!s) return fail(SF_EINVAL, "sf_enable_history: null handle");
    if (capacity < 0) return fail(SF_EINVAL, "sf_enable_history: capacity must be >= 0");
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    HIPCHK(hipStreamSynchronize(s->stream));
    const size_t per = (size_t)s->g.E * s->g.H * s->g.W;
    if (s->history) { HIPCHK(hipFree(s->history)); s->bytes -= (int64_t)(per * s->history_cap); }
    s->history = nullptr; s->history_cap = 0;
    if (capacity == 0) return SF_OK;
    HIPCHK(hipMalloc((void **)&s->history, per * capacity));
    s->bytes += (int64_t)(per * capacity);
    s->history_cap = capacity;
    HIPCHK(hipMemsetAsync(s->history, 0, per * capacity, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return SF_OK;
}

extern "C" int sf_get_history(sf_sim *s, int32_t env, int32_t first, int32_t count, int8_t *out)
{
    if (!s || !out) return fail(SF_EINVAL, "sf_get_history: null argument");
    if (!s->history) return fail(SF_ESTATE, "sf_get_history: call sf_enable_history first");
    if (env < 0 || env >= s->g.E) return fail(SF_EINVAL, "sf_get_history: environment %d out of range", env);
    if (first < 0 || count < 0 || count > s->history_cap)
        return fail(SF_EINVAL, "sf_get_history: %d updates from %d do not fit the capacity %d", count, first, s->history_cap);
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    const size_t map = (size_t)s->g.H * s->g.W;
    const int8_t *base = s->history + (size_t)env * s->history_cap * map;
    const int slot = first % s->history_cap;
    const int n1 = count < s->history_cap - slot ? count : s->history_cap - slot;    // up to the end of the ring
    if (n1) HIPCHK(hipMemcpyAsync(out, base + (size_t)slot * map, (size_t)n1 * map, hipMemcpyDeviceToHost, s->stream));
    if (count > n1) HIPCHK(hipMemcpyAsync(out + (size_t)n1 * map, base, (size_t)(count - n1) * map, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return SF_OK;
}

extern "C" int sf_history_device(sf_sim *s, void **ptr, int32_t *capacity)
{
    if (!s || !ptr || !capacity) return fail(SF_EINVAL, "sf_history_device: null argument");
    *ptr = s->history; *capacity = s->history_cap;
    return SF_OK;
}

// Arrival times: which update created the first sprite of a cell (fire.py:571-587), kept by a pass behind the
// step launches (arrival_pass; enqueue_call cuts a call into pieces of at most max_fire_duration updates while this is on).
extern "C" int sf_enable_arrival(sf_sim *s, int32_t on)
{
    if (!s) return fail(SF_EINVAL, "sf_enable_arrival: null handle");
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    const size_t n = (size_t)s->g.E * s->g.plane_env;
    if (!on) {
        if (!s->arrival1) return SF_OK;
        if (s->val_plane) return fail(SF_ESTATE, "sf_enable_arrival: a value plane is set and needs the arrival plane: switch it off first (sf_values_set with NULL)");
        HIPCHK(hipStreamSynchronize(s->stream));
        HIPCHK(hipFree(s->arrival1));
        s->arrival1 = nullptr;
        s->bytes -= (int64_t)(n * sizeof(uint32_t));
        return SF_OK;
    }
    if (s->arrival1) return SF_OK;
    { int rc = dev_alloc(s, &s->arrival1, n); if (rc) return rc; }
    HIPCHK(hipMemsetAsync(s->arrival1, 0, n * sizeof(uint32_t), s->stream));
    s->arr_pending = 0;
    if (s->was_reset) { int rc = arrival_pass(s); if (rc) return rc; }      // the sprites that are live now carry their true updates
    return finish_call(s, nullptr, !s->async, nullptr);
}

extern "C" int sf_get_arrival(sf_sim *s, int32_t env, int32_t *out)
{
    if (!s || !out) return fail(SF_EINVAL, "sf_get_arrival: null argument");
    if (!s->arrival1) return fail(SF_ESTATE, "sf_get_arrival: call sf_enable_arrival first");
    const Geo &g = s->g;
    if (env < 0 || env >= g.E) return fail(SF_EINVAL, "sf_get_arrival: environment %d out of range", env);
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    HIPCHK(hipMemcpy2DAsync(out, (size_t)g.W * 4, s->arrival1 + (size_t)env * g.plane_env, (size_t)g.P * 4, (size_t)g.W * 4, (size_t)g.H,
                            hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    { int rc = check_team_error(s, "sf_get_arrival"); if (rc) return rc; }
    for (size_t i = 0, n = (size_t)g.H * g.W; i < n; ++i) out[i] -= 1;      // stored: update + 1, 0 = never
    return SF_OK;
}

extern "C" int sf_arrival_device(sf_sim *s, void **ptr, int64_t *row_pitch, int64_t *env_stride)
{
    if (!s || !ptr || !row_pitch || !env_stride) return fail(SF_EINVAL, "sf_arrival_device: null argument");
    if (!s->arrival1) return fail(SF_ESTATE, "sf_arrival_device: call sf_enable_arrival first");
    *ptr = s->arrival1; *row_pitch = (int64_t)s->g.P * 4; *env_stride = (int64_t)s->g.plane_env * 4;
    return SF_OK;
}

extern "C" int sf_set_arrival_dense(sf_sim *s, int32_t on)
{
    if (!s) return fail(SF_EINVAL, "sf_set_arrival_dense: null handle");
    s->arr_dense = on != 0;
    return SF_OK;
}

extern "C" int sf_time_arrival_pass(sf_sim *s, float *ms_out)
{
    if (!s || !ms_out) return fail(SF_EINVAL, "sf_time_arrival_pass: null argument");
    if (!s->arrival1) return fail(SF_ESTATE, "sf_time_arrival_pass: call sf_enable_arrival first");
    { int rc = begin_call(s, "sf_time_arrival_pass", kCommit); if (rc) return rc; }      // (the commit is not part of the pass's time)
    HIPCHK(hipEventRecord(s->ev0, s->stream));
    { int rc = arrival_pass(s); if (rc) return rc; }
    return finish_call(s, nullptr, true, ms_out);
}

extern "C" int sf_get_arrival_passes(sf_sim *s, int64_t *out)
{
    if (!s || !out) return fail(SF_EINVAL, "sf_get_arrival_passes: null argument");
    out[0] = s->arr_passes[0]; out[1] = s->arr_passes[1];
    return SF_OK;
}

#ifdef SF_PHASES
// development build only: arm / read the per-wave timeline of k_step (see profiles/phase_profile.py)
extern "C" int sf_debug_wave_log(int32_t arm, unsigned long long *out)
{
    if (arm) { int v = -2; return hipMemcpyToSymbol(HIP_SYMBOL(g_wave_log_launch), &v, sizeof v) == hipSuccess ? 0 : -1; }
    int v = -1;
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_wave_log_launch), &v, sizeof v);
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wave_log), sizeof(unsigned long long) * 16384 * 4) == hipSuccess ? 0 : -1;
}
#endif

#ifdef SF_PHASES
// development build only: log the marks of one step (index inside the next resident launch) of one environment / read the log
extern "C" int sf_debug_timeline(int32_t env, int32_t step, unsigned long long *out /* [16][64] or null */)
{
    if (out) return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_timeline), sizeof(unsigned long long) * 16 * 64) == hipSuccess ? 0 : -1;
    unsigned long long z[16 * 64] = {};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_timeline), z, sizeof z);
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_timeline_step), &step, sizeof step);
    return hipMemcpyToSymbol(HIP_SYMBOL(g_timeline_env), &env, sizeof env) == hipSuccess ? 0 : -1;
}
#endif

#ifdef SF_WIN_PROF
extern "C" int sf_debug_win_prof(unsigned long long *out /* [1024][16][8] */)
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_win_prof), sizeof(unsigned long long) * 1024 * 16 * 8) == hipSuccess ? 0 : -1;
}
#endif

#ifdef SF_PHASES
extern "C" int sf_debug_phases(unsigned long long *out16)
{
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_phase), sizeof(unsigned long long) * 16) != hipSuccess) return -1;
    unsigned long long z[16] = {};
    return hipMemcpyToSymbol(HIP_SYMBOL(g_phase), z, sizeof z) == hipSuccess ? 0 : -1;
}
#endif

extern "C" int sf_step(sf_sim *s, int32_t n_steps)
{
    if (!s) return fail(SF_EINVAL, "sf_step: null handle");
    return step_call(s, "sf_step", n_steps, nullptr);
}
extern "C" int sf_step_timed(sf_sim *s, int32_t n_steps, float *ms_out)
{
    if (!s || !ms_out) return fail(SF_EINVAL, "sf_step_timed: null argument");
    return step_call(s, "sf_step_timed", n_steps, ms_out);
}

// rows (env, column, row, type) of one step out of a point block [n_steps][E][k][3]
__global__ void k_expand_pts(int E, int k, const int32_t *blk, int32_t *rows)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= E * k) return;
    rows[4 * i] = i / k; rows[4 * i + 1] = blk[3 * i]; rows[4 * i + 2] = blk[3 * i + 1]; rows[4 * i + 3] = blk[3 * i + 2];
}

// The point block of a sf_step_mitigated call on the device (enqueue layer; a host block is copied behind the rows [E * k][4] of one step, which
// the pairs expand into at the head of mit_stage).  Growing the staging buffer waits for the stream: enqueued kernels may read it.
static int stage_lines(sf_sim *s, int n_steps, const int32_t *pts, int k, int device_pointer, const int32_t **blk)
{
    const Geo &g = s->g;
    const size_t rows_bytes = (size_t)g.E * k * 4 * sizeof(int32_t);
    const size_t blk_bytes = device_pointer ? 0 : (size_t)n_steps * g.E * k * 3 * sizeof(int32_t);
    if (blk_bytes + rows_bytes > s->mit_stage_bytes) {
        HIPCHK(hipStreamSynchronize(s->stream));
        if (s->mit_stage) HIPCHK(hipFree(s->mit_stage));
        s->mit_stage = nullptr; s->mit_stage_bytes = 0;
        HIPCHK(hipMalloc(reinterpret_cast<void **>(&s->mit_stage), blk_bytes + rows_bytes));
        s->mit_stage_bytes = blk_bytes + rows_bytes;
    }
    *blk = pts;
    if (!device_pointer) {
        int32_t *d = s->mit_stage + (size_t)g.E * k * 4;
        HIPCHK(hipMemcpyAsync(d, pts, blk_bytes, hipMemcpyHostToDevice, s->stream));
        *blk = d;
    }
    return SF_OK;
}
// Step i of a call with control lines that the resident launch cannot take (enqueue layer): scatter the step's points, then one update.
// The bookkeeping is that of a call with control lines, whichever way it runs: its single updates are not a run(1) loop.  Arrival
// recording: a pass every max_fire_duration pairs; the one behind the last pair is the caller's (arr_pending != 0).
static int enqueue_pair(sf_sim *s, const int32_t *blk, int k, int i, hipEvent_t t0)
{
    const Geo &g = s->g;
    if (i == 0) { s->status_fresh = false; s->last_launches = 0; s->step1_polls = 0; }
    hipLaunchKernelGGL(k_expand_pts, dim3((unsigned)((g.E * k + 255) / 256)), dim3(256), 0, s->stream, g.E, k,
                       blk + (size_t)i * g.E * k * 3, s->mit_stage);
    const int rc = scatter_points(s, s->mit_stage, g.E * k);
    return rc ? rc : step_impl(s, 1, /*hold=*/true, t0);
}

/* A rollout in which control lines are drawn before every update - the loop
 *     for s in range(n_steps): sim.update_mitigation(points[s]); sim.run(1)
 * of an RL harness whose agents' moves are known in advance (BASELINE config C5: 64 agents per environment writing one
 * line cell per step) - as ONE call.  pts: int32 [n_steps][n_envs][k][3] = (column, row, type) per environment and step;
 * entries whose type is not a control line (3, 4, 5) or whose position is off the grid are skipped (padding).
 * Where the environment-resident launch can run it applies an environment's points inside the kernel, right before that
 * environment's update; otherwise the call enqueues n_steps scatter + step pairs.  ms_out (may be null): GPU milliseconds. */
extern "C" int sf_step_mitigated(sf_sim *s, int32_t n_steps, const int32_t *pts, int32_t k, int32_t device_pointer, float *ms_out)
{
    const char *who = "sf_step_mitigated";
    if (!s) return fail(SF_EINVAL, "sf_step_mitigated: null handle");
    if (n_steps < 0 || k < 0 || (n_steps > 0 && k > 0 && !pts)) return fail(SF_EINVAL, "sf_step_mitigated: bad arguments");
    if (ms_out) *ms_out = 0.f;
    if (n_steps == 0) return SF_OK;
    if (k == 0) return step_call(s, who, n_steps, ms_out);
    { int rc = begin_call(s, who, kNeedRt | kNeedReset); if (rc) return rc; }
    const StepPlan plan = plan_step(s, n_steps, true);       // can the resident launch take the lines?  Otherwise scatter + step pairs
    const int32_t *blk = nullptr;
    { int rc = stage_lines(s, n_steps, pts, k, device_pointer, &blk); if (rc) return rc; }
    if (plan.nw) {
        const int rc = enqueue_call(s, plan, n_steps, blk, k, false, ms_out ? s->ev0 : nullptr);
        return rc ? rc : finish_call(s, who, !s->async, ms_out);
    }
    for (int i = 0; i < n_steps; ++i) {      // (timed: the GPU time of the updates alone, so every pair is waited for)
        float ms1 = 0.f;
        int rc = enqueue_pair(s, blk, k, i, ms_out ? s->ev0 : nullptr);
        if (!rc && ms_out) rc = finish_call(s, who, true, &ms1);
        if (rc) return rc;
        if (ms_out) *ms_out += ms1;
    }
    if (s->arr_pending) { int rc = arrival_pass(s); if (rc) return rc; }
    return finish_call(s, who, !s->async, nullptr);
}

// ---------------------------------------------------------------------------------------------------- closed loop
// FireSimulation.update_mitigation(actions) + run(1) with actions that depend on the last observation (simulation.py:449-478,
// 501-553), without a launch per step: sf_loop_start leaves k_run resident, sf_loop_step posts one step's points into
// host-mapped memory, rings the doorbell and waits for every environment's "done" number; the result block arrives with it.
static int loop_launch(sf_sim *s)
{
    const Geo &g = s->g;
    StepArgs a = handle_args(s);
    a.mit = s->loop_pts_mem; a.mit_k = s->loop_k;
    a.res_block = s->status_block; a.res_elapsed = s->elapsed_dev; a.res_sink = s->sink;
    a.cost = s->run_cost;
    a.loop_db = s->loop_db_dev; a.loop_pts_host = s->loop_pts_dev; a.loop_res_host = s->loop_res_dev;
    a.loop_seq = s->loop_mem; a.loop_done = s->loop_mem + 32; a.loop_pts = s->loop_pts_mem;
    a.loop_timeout = 400000000ull;             // ~0.2 s without a ring: the workgroups leave, the next sf_loop_step starts them again
    HIPCHK(hipMemsetAsync(s->loop_mem, 0, sizeof(uint32_t), s->stream));       // nothing forwarded yet (the word may hold the stop of the launch before)
    // one 16-wave workgroup per environment - or the light loop's 8-wave one (SF_TUNE_LOOP_LIGHT)
    const int nw_cap = s->loop_light ? 8 : 16;
    const int nw = (g.H + 63) / 64 < nw_cap ? (g.H + 63) / 64 : nw_cap;
    long long all_vec = (long long)g.H * g.PV;
    int vcap = s->loop_light ? 1024 : 4096;
    if (vcap > all_vec) vcap = (int)((all_vec + 63) / 64 * 64);
    const size_t lds = run_lds_bytes(g, nw, vcap);
    // (8 waves on up to 1024 rows: two bitmap rows per thread, k_run<2, ...>)
    return launch_run(s, run_key(g, kRunLoop, run_words(g.H, nw, 1), true), (unsigned)g.E, (unsigned)nw * 64, lds, a, 0x7FFFFFFF, vcap, 64);
}

extern "C" int sf_loop_start(sf_sim *s, int32_t k)
{
    if (!s) return fail(SF_EINVAL, "sf_loop_start: null handle");
    if (k < 0 || k > 64) return fail(SF_EINVAL, "sf_loop_start: 0 .. 64 points per environment and step (got %d)", k);
    { int rc0 = check_ready(s, "sf_loop_start", kNeedRt | kNeedReset); if (rc0) return rc0; }
    HIPCHK(hipSetDevice(s->p.device));
    const Geo &g = s->g;
    // the resident launch with one workgroup per environment, every environment resident at once
    // SF_TUNE_LOOP_LIGHT = 1: the loop runs 8-wave workgroups with a short vector list - half of every CU's wave slots and more than half of
    // its LDS stay free, so the harness's own kernels (a policy network that shares the GPU) run on every CU beside the resident, mostly
    // sleeping loop.  (A stream with a CU mask - hipExtStreamCreateWithCUMask - was tried first: such a stream is a BLOCKING one, a kernel
    // on torch's default stream then waits for the resident loop to leave; profiles/cu_mask_probe.hip has the mask's numbering.)
    const int light = s->tune.v[SF_TUNE_LOOP_LIGHT] > 0 ? 1 : 0;
    if (!s->wind_sched.empty()) return fail(SF_ENOTSUP, "sf_loop_start: not while a wind schedule is set (sf_set_wind_schedule): a closed loop has no call boundary for the wind to change at");
    if (s->arrival1) return fail(SF_ENOTSUP, "sf_loop_start: not while arrival times are recorded (sf_enable_arrival): a closed loop has no launch boundary for the pass");
    if (g.ab != 1 || s->generic || g.VW != 1 || s->graph_on || s->history || g.dense || g.H > 16 * 64 || g.E > s->n_cu ||
        (s->fused_mode >= 0 && s->fused_mode != 2))
        return fail(SF_ENOTSUP, "sf_loop_start: needs the environment-resident launch with every environment resident at once "
                                "(grids up to 1024 x 1024, max_fire_duration <= 5, no more environments than CUs, no spread graph / history)");
    LOOP_QUIESCE(s);                   // (a refused call leaves a running loop running)
    s->loop_light = light;
    { int rc0 = ensure_commit(s); if (rc0) return rc0; }
    { int rc0 = ensure_vbits(s); if (rc0) return rc0; }
    { int rc0 = ensure_bl(s); if (rc0) return rc0; }
    auto pin = [&](void **host, void **dev, size_t bytes) -> int {
        HIPCHK(hipHostMalloc(host, bytes, hipHostMallocMapped | hipHostMallocCoherent));      // fine-grained: no GPU cache may hold these lines
        HIPCHK(hipHostGetDevicePointer(dev, *host, 0));
        memset(*host, 0, bytes);
        return SF_OK;
    };
    if (!s->loop_db) {
        int rc = pin((void **)&s->loop_db, (void **)&s->loop_db_dev, sizeof(uint32_t) * 64); if (rc) return rc;
        rc = pin((void **)&s->loop_res, (void **)&s->loop_res_dev, (size_t)64 * g.E); if (rc) return rc;
        HIPCHK(hipMalloc(reinterpret_cast<void **>(&s->loop_mem), sizeof(uint32_t) * (32 + (size_t)g.E)));
    }
    s->loop_slot_ints = (size_t)g.E * k * 4;        // a slot of the points ring: 16-byte pieces (column, row, type, the step's number)
    const size_t pts_bytes = sizeof(int32_t) * 2 * (s->loop_slot_ints ? s->loop_slot_ints : 4);
    if (pts_bytes > s->loop_pts_cap) {
        if (s->loop_pts) HIPCHK(hipHostFree(s->loop_pts));
        if (s->loop_pts_mem) HIPCHK(hipFree(s->loop_pts_mem));
        s->loop_pts = nullptr; s->loop_pts_mem = nullptr; s->loop_pts_cap = 0;
        int rc = pin((void **)&s->loop_pts, (void **)&s->loop_pts_dev, pts_bytes); if (rc) return rc;
        HIPCHK(hipMalloc(reinterpret_cast<void **>(&s->loop_pts_mem), pts_bytes));
        s->loop_pts_cap = pts_bytes;
    }
    s->loop_k = k; s->loop_seq = 0; s->loop_restarts = 0;
    volatile uint32_t *db = s->loop_db;
    for (int i = 0; i < 64; ++i) db[i] = 0;
    memset(s->loop_res, 0, (size_t)64 * g.E);
    memset(s->loop_pts, 0, pts_bytes);             // (pieces of an earlier loop carry ITS step numbers)
    __sync_synchronize();
    HIPCHK(hipMemsetAsync(s->loop_mem, 0, sizeof(uint32_t) * (32 + (size_t)g.E), s->stream));
    HIPCHK(hipMemsetAsync(s->loop_pts_mem, 0, pts_bytes, s->stream));
    if (s->tdirty_all) HIPCHK(hipMemsetAsync(s->tdirty, 1, s->n_tiles_max, s->stream));
    s->tdirty_all = false;
    s->status_fresh = false;
    { int rc0 = loop_launch(s); if (rc0) return rc0; }
    HIPCHK(hipGetLastError());
    s->loop_on = true;
    s->tiles_valid = false;
    s->last_kind = 2;
    return SF_OK;
}

/* pts: int32 [n_envs][k][3] = (column, row, type) of this step (k as given to sf_loop_start; entries with a type outside 3..5 are
 * padding), or null = no points.  status_out: int32 [n_envs][8] (like sf_get_status) or null; elapsed_out: double [n_envs] or null. */
extern "C" int sf_loop_step(sf_sim *s, const int32_t *pts, int32_t *status_out, double *elapsed_out)
{
    if (!s) return fail(SF_EINVAL, "sf_loop_step: null handle");
    if (!s->loop_on) return fail(SF_ESTATE, "sf_loop_step: call sf_loop_start first");
    const Geo &g = s->g;
    const uint32_t seq = s->loop_seq + 1;
    if (seq >= 0x7FFFFFF0u) return fail(SF_ESTATE, "sf_loop_step: sequence numbers exhausted; sf_loop_stop and start again");
    if (s->loop_k > 0) {
        // the points are their own doorbell: 16-byte pieces that carry the step's number, each written by ONE 16-byte store (the relay takes a
        // piece when it carries the number it waits for)
        __m128i *slot = reinterpret_cast<__m128i *>(s->loop_pts + (size_t)(seq & 1u) * s->loop_slot_ints);
        const size_t n = (size_t)g.E * s->loop_k;
        if (pts) for (size_t i = 0; i < n; ++i) _mm_store_si128(slot + i, _mm_set_epi32((int)seq, pts[3 * i + 2], pts[3 * i + 1], pts[3 * i]));
        else for (size_t i = 0; i < n; ++i) _mm_store_si128(slot + i, _mm_set_epi32((int)seq, 0, 0, 0));
    }
    volatile uint32_t *db = s->loop_db;
    __sync_synchronize();                                    // the points are in memory before the number that announces them
    db[0] = seq;
    s->loop_seq = seq;
    if (s->fire_rows > 0 && s->fire_rows < g.H) s->fire_rows = s->fire_rows + 2 > g.H ? g.H : s->fire_rows + 2;
    // wait for the "done" number; should the launch have left by itself (no ring for loop_timeout clocks), start it again: every
    // workgroup resumes from its own "done" number, the points of this step are still in their slot
    const volatile uint32_t *res = reinterpret_cast<const volatile uint32_t *>(s->loop_res);
    auto arrived = [&](int q) { const volatile uint32_t *l = res + (size_t)q * 16; return l[3] == seq && l[7] == seq && l[11] == seq && l[15] == seq; };
    // (a row is taken out of its line as soon as the line is there: nothing is left to do behind the last arrival)
    auto take = [&](int q) {
        const volatile uint32_t *l = res + (size_t)q * 16;
        if (status_out) {
            int32_t *o = status_out + (size_t)q * 8;
            o[0] = (int32_t)l[0]; o[1] = (int32_t)l[1]; o[2] = (int32_t)l[2]; o[3] = (int32_t)l[4]; o[4] = (int32_t)l[5]; o[5] = (int32_t)l[6];
            o[6] = (int32_t)l[8]; o[7] = (int32_t)l[9];
        }
        if (elapsed_out) {
            const unsigned long long el = (unsigned long long)l[10] | ((unsigned long long)l[12] << 32);
            memcpy(elapsed_out + q, &el, sizeof el);
        }
    };
    int e = 0;
    for (unsigned long long spins = 0;; ++spins) {
        while (e < g.E && arrived(e)) { take(e); ++e; }
        if (e == g.E) break;
        if ((spins & 0x3FFF) == 0x3FFF && hipStreamQuery(s->stream) == hipSuccess) {
            bool all = true;
            for (int q = 0; q < g.E; ++q) all = all && arrived(q);
            if (all) { for (int q = e; q < g.E; ++q) take(q); break; }
            if (s->xerr_pinned && *s->xerr_pinned) return fail(SF_EHIP, "sf_loop_step: the resident launch failed");
            HIPCHK(hipSetDevice(s->p.device));
            s->loop_restarts++;
            { int rc0 = loop_launch(s); if (rc0) return rc0; }
            HIPCHK(hipGetLastError());
        }
    }
    return SF_OK;
}

extern "C" int sf_loop_stop(sf_sim *s) { return s ? loop_stop(s) : fail(SF_EINVAL, "sf_loop_stop: null handle"); }
static int loop_stop(sf_sim *s)
{
    if (!s->loop_on) return SF_OK;
    HIPCHK(hipSetDevice(s->p.device));
    volatile uint32_t *db = s->loop_db;
    __sync_synchronize();
    db[0] = s->loop_seq | kLoopStop;
    __sync_synchronize();
    s->loop_on = false;
    HIPCHK(hipStreamSynchronize(s->stream));      // the workgroups commit their environments and leave the result block behind
    s->status_fresh = true;
    return SF_OK;
}

extern "C" int sf_loop_restarts(sf_sim *s, int32_t *out)
{
    if (!s || !out) return fail(SF_EINVAL, "sf_loop_restarts: null argument");
    *out = s->loop_restarts;
    return SF_OK;
}

static int get_maps(sf_sim *s, int env0, int n, uint8_t *out)
{
    const Geo &g = s->g;
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    if (s->last_was_step1) { s->last_was_step1 = false; s->step1_polls = 0; }      // (a loop that looks at the maps after every update: per-step kernels)
    const size_t bytes = (size_t)n * g.H * g.W;
    int rc = ensure_stage(s, bytes);
    if (rc) return rc;
    dim3 blk(256), grd((g.W + 255) / 256, g.H, n);
    hipLaunchKernelGGL(k_unpack_status, grd, blk, 0, s->stream, g, (const uint8_t *)s->status, (const uint8_t *)(s->bl_cur ? s->cells : nullptr), env0, (uint8_t *)s->stage, (uint8_t *)nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, s->stage, bytes, hipMemcpyDeviceToHost, s->stream));
    return finish_call(s, "sf_get_fire_map(s)", true, nullptr);
}

extern "C" int sf_get_fire_map(sf_sim *s, int32_t env, uint8_t *out)
{
    if (!s || !out) return fail(SF_EINVAL, "sf_get_fire_map: null argument");
    if (env < 0 || env >= s->g.E) return fail(SF_EINVAL, "sf_get_fire_map: environment %d out of range", env);
    return get_maps(s, env, 1, out);
}

extern "C" int sf_get_fire_maps(sf_sim *s, uint8_t *out)
{
    if (!s || !out) return fail(SF_EINVAL, "sf_get_fire_maps: null argument");
    const int chunk = 64;   // bound the staging buffer
    for (int e = 0; e < s->g.E; e += chunk) {
        const int n = s->g.E - e < chunk ? s->g.E - e : chunk;
        int rc = get_maps(s, e, n, out + (size_t)e * s->g.H * s->g.W);
        if (rc) return rc;
    }
    return SF_OK;
}

/* The cells of environment env whose BurnStatus differs from the reference point - the map as it was when THIS function was last called for the
 * environment, or the all-UNBURNED map of sf_reset (the ignition cell is reported) -: cells_out[i] = (y * W + x) << 3 | BurnStatus, *n_out of
 * them, in no particular order.  *n_out = -1: there is no reference point (first call for this environment, or sf_load_fire_map came in between)
 * or more than cap cells changed - fetch the whole map with sf_get_fire_map before anything steps; either way the current map is the reference
 * point from now on.  (sf_get_fire_map itself never moves the reference point: a look at the map for another purpose does not make a mirror
 * kept from the deltas miss a cell.)
 * The host-side counterpart of the reference's in-place mutation of ONE fire_map array (fire.py:140, 587, 719; simulation.py:546-553). */
// the buffers of the delta query; the launch of k_map_delta (or, without a reference point, of the snapshot) on the handle's stream.  *mode: 0 = the list
// is on its way into delta_pinned, 1 = no reference point (the current map has become it): the caller fetches the whole map
static int delta_enqueue(sf_sim *s, int env, int cap, int *mode, bool with_row = false)
{
    const Geo &g = s->g;
    constexpr int kInline = 1024;      // entries that travel with the count (one copy, one wait)
    if (!s->snap) {
        int rc = dev_alloc(s, &s->snap, (size_t)g.E * g.plane_env);
        if (rc) return rc;
        s->snap_valid.assign((size_t)g.E, 0);
    }
    if (cap > s->delta_cap || !s->delta_dev) {
        HIPCHK(hipStreamSynchronize(s->stream));
        if (s->delta_dev) { HIPCHK(hipFree(s->delta_dev)); s->delta_dev = nullptr; }
        if (s->delta_pinned) { HIPCHK(hipHostFree(s->delta_pinned)); s->delta_pinned = nullptr; }
        const int c = cap > kInline ? cap : kInline;
        HIPCHK(hipMalloc(reinterpret_cast<void **>(&s->delta_dev), ((size_t)c + kDeltaHead) * sizeof(uint32_t)));
        HIPCHK(hipHostMalloc(reinterpret_cast<void **>(&s->delta_pinned), ((size_t)c + kDeltaHead + 16) * sizeof(uint32_t), hipHostMallocDefault));      // (+ 16: a row that could not travel with a list, sf_run_delta)
        HIPCHK(hipMemsetAsync(s->delta_dev, 0, sizeof(uint32_t), s->stream));
        s->delta_cap = c;
        s->delta_base = 0;
    }
    if (!s->snap_valid[env]) {
        // no reference point: the current map becomes it, the caller fetches the whole map
        dim3 blk(256), grd((g.W + 255) / 256, g.H, 1);
        int rc = ensure_stage(s, (size_t)g.H * g.W);
        if (rc) return rc;
        hipLaunchKernelGGL(k_unpack_status, grd, blk, 0, s->stream, g, (const uint8_t *)s->status, (const uint8_t *)(s->bl_cur ? s->cells : nullptr), env, (uint8_t *)s->stage, s->snap);
        HIPCHK(hipGetLastError());
        s->snap_valid[env] = 1;
        *mode = 1;
        return SF_OK;
    }
    hipLaunchKernelGGL(k_map_delta, dim3((g.PV + 255) / 256, g.H), dim3(256), 0, s->stream, g, (const uint8_t *)s->status, (const uint8_t *)(s->bl_cur ? s->cells : nullptr), env,
                       s->snap + (size_t)env * g.plane_env, s->delta_dev, cap, s->delta_base,
                       with_row ? (const int32_t *)(s->status_block + (size_t)env * 8) : nullptr, (const double *)(s->elapsed_dev + env));
    HIPCHK(hipGetLastError());
    const int first = cap < kInline ? cap : kInline;
    HIPCHK(hipMemcpyAsync(s->delta_pinned, s->delta_dev, ((size_t)first + kDeltaHead) * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    *mode = 0;
    return SF_OK;
}
// behind the wait for the stream: the list out of the landing zone (a second copy if it is longer than what travelled with the count)
static int delta_finish(sf_sim *s, int cap, uint32_t *cells_out, int32_t *n_out)
{
    constexpr int kInline = 1024;
    const int first = cap < kInline ? cap : kInline;
    const uint32_t n = s->delta_pinned[0] - s->delta_base;
    s->delta_base = s->delta_pinned[0];
    if (n > (uint32_t)cap) { *n_out = -1; return SF_OK; }      // (the reference point is current: the caller fetches the whole map)
    if (n > (uint32_t)first) {
        HIPCHK(hipMemcpyAsync(s->delta_pinned + kDeltaHead + first, s->delta_dev + kDeltaHead + first, ((size_t)n - first) * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));
    }
    if (n) memcpy(cells_out, s->delta_pinned + kDeltaHead, (size_t)n * sizeof(uint32_t));
    *n_out = (int32_t)n;
    return SF_OK;
}

extern "C" int sf_get_fire_map_delta(sf_sim *s, int32_t env, uint32_t *cells_out, int32_t cap, int32_t *n_out)
{
    if (!s || !n_out || cap < 0 || (cap > 0 && !cells_out)) return fail(SF_EINVAL, "sf_get_fire_map_delta: bad argument");
    const Geo &g = s->g;
    if (env < 0 || env >= g.E) return fail(SF_EINVAL, "sf_get_fire_map_delta: environment %d out of range", env);
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    note_result_look(s);               // (like a status query)
    int mode = 0;
    { int rc = delta_enqueue(s, env, cap, &mode); if (rc) return rc; }
    { int rc = finish_call(s, "sf_get_fire_map_delta", true, nullptr); if (rc) return rc; }
    if (mode == 1) { *n_out = -1; return SF_OK; }
    return delta_finish(s, cap, cells_out, n_out);
}

static int refresh_status(sf_sim *s, int32_t *copy_to);
/* FireSimulation.run(n) as ONE call and ONE wait (simulation.py:501-553: the loop of update() calls, then the attributes a caller reads - fire_map,
 * elapsed_steps, elapsed_time, active): sf_step(n_steps) on every environment of the handle, then environment env's row of the result block
 * (sf_get_status), its elapsed_time and the cells of its fire_map that changed (sf_get_fire_map_delta) - three calls' worth of launches and copies
 * enqueued behind each other, waited for once.  *n_out as for sf_get_fire_map_delta (-1: fetch the whole map). */
extern "C" int sf_run_delta(sf_sim *s, int32_t n_steps, int32_t env, int32_t *status_row, double *elapsed, uint32_t *cells_out, int32_t cap, int32_t *n_out)
{
    if (!s || !status_row || !n_out || cap < 0 || (cap > 0 && !cells_out) || n_steps < 0) return fail(SF_EINVAL, "sf_run_delta: bad argument");
    const Geo &g = s->g;
    if (env < 0 || env >= g.E) return fail(SF_EINVAL, "sf_run_delta: environment %d out of range", env);
    int rc = begin_call(s, "sf_run_delta", kNeedRt | kNeedReset);
    if (!rc) rc = step_impl(s, n_steps, false, nullptr);
    if (rc) return rc;
    note_result_look(s);
    rc = refresh_status(s, nullptr);               // (nothing to launch behind a resident launch: it has left the block behind itself)
    if (rc) return rc;
    int mode = 0;
    rc = delta_enqueue(s, env, cap, &mode, true);
    if (rc) return rc;
    uint32_t *land = s->delta_pinned + 1;          // the row and its elapsed_time have travelled with the list's count ...
    if (mode == 1) {                               // ... unless there was no list
        land = s->delta_pinned + s->delta_cap + kDeltaHead;
        HIPCHK(hipMemcpyAsync(land, s->status_block + (size_t)env * 8, 8 * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
        HIPCHK(hipMemcpyAsync(land + 8, s->elapsed_dev + env, sizeof(double), hipMemcpyDeviceToHost, s->stream));
    }
    rc = finish_call(s, "sf_run_delta", true, nullptr);
    if (rc) return rc;
    memcpy(status_row, land, 8 * sizeof(int32_t));
    if (elapsed) memcpy(elapsed, land + 8, sizeof(double));
    if (mode == 1) *n_out = -1;
    else rc = delta_finish(s, cap, cells_out, n_out);
    return rc;
}

extern "C" int sf_get_burn(sf_sim *s, int32_t env, double *out)
{
    if (!s || !out) return fail(SF_EINVAL, "sf_get_burn: null argument");
    const Geo &g = s->g;
    if (env < 0 || env >= g.E) return fail(SF_EINVAL, "sf_get_burn: environment %d out of range", env);
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    const size_t bytes = (size_t)g.H * g.W * sizeof(double);
    int rc = ensure_stage(s, bytes);
    if (rc) return rc;
    dim3 blk(256), grd((g.W + 255) / 256, g.H);
    rc = ensure_commit(s);
    if (rc) return rc;
    rc = ensure_rm(s);
    if (rc) return rc;
    hipLaunchKernelGGL(k_unpack_burn, grd, blk, 0, s->stream, g, (const uint8_t *)s->status, (const uint32_t *)s->settled,
                       (const double *)s->burn, (const EnvState *)s->commit, env, (double *)s->stage);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, s->stage, bytes, hipMemcpyDeviceToHost, s->stream));
    return finish_call(s, "sf_get_burn", true, nullptr);
}

extern "C" int sf_set_burn(sf_sim *s, int32_t env, const double *burn)
{
    if (!s || !burn) return fail(SF_EINVAL, "sf_set_burn: null argument");
    const Geo &g = s->g;
    if (env < 0 || env >= g.E) return fail(SF_EINVAL, "sf_set_burn: environment %d out of range", env);
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    const size_t bytes = (size_t)g.H * g.W * sizeof(double);
    int rc = ensure_stage(s, bytes);
    if (rc) return rc;
    dim3 blk(256), grd((g.W + 255) / 256, g.H);
    rc = ensure_commit(s);
    if (rc) return rc;
    rc = ensure_rm(s);
    if (rc) return rc;
    if (g.att)   // the caller's values are the truth now: nothing is owed any more
        hipLaunchKernelGGL(k_settle_env, grd, blk, 0, s->stream, g, (const uint8_t *)s->status, s->settled, s->burn,
                           (const EnvState *)s->commit, env, 0);
    HIPCHK(hipMemcpyAsync(s->stage, burn, bytes, hipMemcpyHostToDevice, s->stream));
    hipLaunchKernelGGL(k_pack_burn, grd, blk, 0, s->stream, g, s->burn, env, (const double *)s->stage);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s->stream));
    return SF_OK;
}

// ----------------------------------------------------------------------------- environment state
// Every state call begins as begin_call(kStateCall): the closed loop ended, a reset insisted on, a voided handle refused, the step
// rings folded into commit[].

extern "C" int sf_copy_envs(sf_sim *s, const int32_t *src, const int32_t *dst, int32_t n, int32_t flags)
{
    if (!s) return fail(SF_EINVAL, "sf_copy_envs: null handle");
    if (n < 0 || (n > 0 && (!src || !dst))) return fail(SF_EINVAL, "sf_copy_envs: bad environment lists");
    if (flags & ~SF_COPY_TERRAIN) return fail(SF_EINVAL, "sf_copy_envs: unknown flags 0x%x", flags);
    const Geo &g = s->g;
    std::vector<char> role((size_t)g.E, 0);       // bit 0: a source, bit 1: a destination
    { int rc = check_envs(s, "sf_copy_envs", n, src); if (!rc) rc = check_envs(s, "sf_copy_envs", n, dst); if (rc) return rc; }
    for (int i = 0; i < n; ++i) {
        if (role[dst[i]] & 2) return fail(SF_EINVAL, "sf_copy_envs: environment %d is a destination twice", dst[i]);
        role[dst[i]] |= 2;
    }
    for (int i = 0; i < n; ++i) role[src[i]] |= 1;
    for (int e = 0; e < g.E; ++e)
        if (role[e] == 3) return fail(SF_EINVAL, "sf_copy_envs: environment %d is both a source and a destination", e);
    if (n == 0) return SF_OK;
    { int rc = begin_call(s, "sf_copy_envs", kStateCall); if (rc) return rc; }
    // Every per-environment slice of the current layout and of the structures derived from it: a handle-wide "rebuild" flag would make
    // the next step rebuild them for every environment.
    CopyList L;
    const bool terrain = (flags & SF_COPY_TERRAIN) && s->rt_set.size() > 1;      // (a stale rtc copy stays marked stale below)
    // (section 20: the record travels with the arrival plane it was summed over - under ONE plane for all environments.  Planes per
    // environment stay where they are, like the terrain without SF_COPY_TERRAIN: dst's damage is its own plane over src's arrival,
    // recounted below)
    L.n_seg = arrival_seg(s, L.seg, env_segs(s, terrain ? kForkKinds : kForkKinds & ~kSegTerrain, L.seg));
    if (!s->val_per_env) L.n_seg = value_seg(s, L.seg, L.n_seg);
    const unsigned gx = seg_grid_x(L.seg, L.n_seg);
    // with the terrain go the slices of section 18, where they exist: the table's part of the wind cache, the environment's schedule
    // and the segment its table stands for (a launch of their own: the slice table of env_segs is full)
    CopyList Wl;
    Wl.n_seg = 0;
    if (terrain && s->wterms) Wl.seg[Wl.n_seg++] = {reinterpret_cast<uint8_t *>(s->wterms), (long long)kWindPlanes * g.H * g.W * 4, (long long)kWindPlanes * g.H * g.W * 4};
    if (terrain && s->wsched) Wl.seg[Wl.n_seg++] = {reinterpret_cast<uint8_t *>(s->wsched), (long long)sizeof(WindSched), (long long)sizeof(WindSched)};
    for (int i0 = 0; i0 < n; i0 += kCopyPairs) {
        const int cnt = std::min(kCopyPairs, n - i0);
        for (int i = 0; i < cnt; ++i) { L.src[i] = Wl.src[i] = src[i0 + i]; L.dst[i] = Wl.dst[i] = dst[i0 + i]; }
        hipLaunchKernelGGL(k_env_copy, dim3(gx, (unsigned)cnt), dim3(256), 0, s->stream, L);
        if (Wl.n_seg) hipLaunchKernelGGL(k_env_copy, dim3(seg_grid_x(Wl.seg, Wl.n_seg), (unsigned)cnt), dim3(256), 0, s->stream, Wl);
        HIPCHK(hipGetLastError());
    }
    for (int i = 0; i < n; ++i) {
        if (s->snap) s->snap_valid[dst[i]] = 0;      // (sf_get_fire_map_delta: the next query for dst hands back the whole map once)
        if (terrain) {
            s->rd_lay[dst[i]] = s->rd_lay[src[i]]; s->rd_fbfm[dst[i]] = s->rd_fbfm[src[i]]; s->rd_stale[dst[i]] = 1;
            if (s->rd_fuel_ix && s->rd_fbfm[src[i]] && dst[i] != src[i]) {
                const size_t cells = (size_t)g.H * g.W;
                HIPCHK(hipMemcpyAsync(s->rd_fuel_ix + (size_t)dst[i] * cells, s->rd_fuel_ix + (size_t)src[i] * cells, cells,
                                      hipMemcpyDeviceToDevice, s->stream));
            }
            s->rt_set[dst[i]] = s->rt_set[src[i]];
            if (s->rtc_stale.size() == s->rt_set.size()) s->rtc_stale[dst[i]] = s->rtc_stale[src[i]];
            if (!s->rtc || s->rtc_stale.size() != s->rt_set.size() || s->rtc_stale[dst[i]]) s->rtc_valid = false;
            if (!s->wt_stale.empty()) s->wt_stale[dst[i]] = s->wt_stale[src[i]];
            if (s->wsched) s->wind_K[dst[i]] = s->wind_K[src[i]];
        }
    }
    if (terrain) { s->have_rt = true; for (char c : s->rt_set) if (!c) s->have_rt = false; }
    if (terrain && s->wsched) wind_sched_count(s);
    if (s->val_per_env) { int rc = value_recount(s); if (rc) return rc; }
    // (fire_rows bounds every environment's fire, dst's copy included; status_fresh: dst's row is src's current row)
    return finish_call(s, nullptr, !s->async, nullptr);
}

static StateHeader state_header(const sf_sim *s)
{
    const Geo &g = s->g;
    StateHeader h;
    memset(&h, 0, sizeof h);
    h.magic = kStateMagic; h.version = kStateVersion;
    h.bytes = state_layout(g, s->parents != nullptr, s->arrival1 != nullptr).bytes;
    h.H = g.H; h.W = g.W; h.md = g.md; h.ab = g.ab;
    h.diag = g.diag; h.att = g.att; h.has_max_time = g.has_max_time; h.prune_after_quit = g.prune_after_quit;
    h.has_parents = s->parents != nullptr; h.fire_rows = s->fire_rows; h.has_arrival = s->arrival1 != nullptr;
    h.max_time = g.has_max_time ? g.max_time : 0.0; h.update_rate = g.update_rate; h.pixel_scale = g.pixel_scale;
    return h;
}

// a blob this handle can take: every value its state depends on matches (the first one that does not is named)
static int header_check(const sf_sim *s, const StateHeader &b, int i)
{
    const StateHeader h = state_header(s);
    const char *what = nullptr;
    if (b.magic != h.magic) what = "magic number (not a state blob)";
    else if (b.version != h.version) what = "format version";
    else if (b.H != h.H || b.W != h.W) what = "grid size";
    else if (b.md != h.md || b.ab != h.ab) what = "max_fire_duration";
    else if (b.diag != h.diag) what = "diagonal spread";
    else if (b.att != h.att) what = "line attenuation";
    else if (b.has_max_time != h.has_max_time || b.max_time != h.max_time) what = "max_time";
    else if (b.update_rate != h.update_rate) what = "update_rate";
    else if (b.pixel_scale != h.pixel_scale) what = "pixel_scale threshold";
    else if (b.prune_after_quit != h.prune_after_quit) what = "prune_after_quit";
    else if (b.has_parents != h.has_parents) what = "spread graph";
    else if (b.has_arrival != h.has_arrival) what = "arrival recording";
    else if (b.bytes != h.bytes) what = "size";
    if (what) return fail(SF_EINVAL, "sf_load_state: blob %d does not match this handle: %s", i, what);
    return SF_OK;
}

static int state_list(const sf_sim *s, int32_t n, const int32_t *envs, const void *buf, int32_t device_pointer, const char *who, bool distinct)
{
    if (n < 0 || (n > 0 && (!envs || !buf))) return fail(SF_EINVAL, "%s: bad argument", who);
    if (device_pointer && ((uintptr_t)buf & 15))      // (the kernels read / write the f64 and u32 sections in place)
        return fail(SF_EINVAL, "%s: a device buffer must be 16-byte aligned", who);
    return check_envs(s, who, n, envs, distinct ? "is listed twice" : nullptr);
}

static StateArgs state_args(sf_sim *s)
{
    StateArgs a;
    memset(&a, 0, sizeof a);
    a.g = s->g;
    a.status = s->status; a.age = s->age; a.cells = s->bl_cur ? s->cells : nullptr;
    a.burn = s->burn; a.settled = s->settled; a.parents = s->parents; a.arrival = s->arrival1; a.vbits = s->vbits;
    a.commit = s->commit; a.res_block = s->status_block; a.res_sink = s->sink; a.res_elapsed = s->elapsed_dev;
    a.lay = state_layout(s->g, s->parents != nullptr, s->arrival1 != nullptr);
    a.stride = a.lay.bytes;
    return a;
}
// environments per launch, and per pass through the staging buffer of a host-pointer call (<= 64 MB of blobs unless one is larger)
static int state_chunk(const StateArgs &a, bool device)
{
    if (device) return kStateEnvs;
    return (int)std::max<long long>(1, std::min<long long>(kStateEnvs, (64LL << 20) / a.stride));
}

// ----------------------------------------------------------------------------- resets
// A call's environment list / host ignitions -> device memory through the pinned buffer, one copy; *dev is where they are.
static int reset_stage(sf_sim *s, const void *a, size_t na, const void *b, size_t nb, uint8_t **dev)
{
    CallBlock &blk = s->rs_blk;
    { int rc = block_reserve(s, blk, na + nb); if (rc) return rc; }
    if (na) memcpy(blk.pinned, a, na);
    if (nb) memcpy(blk.pinned + na, b, nb);
    *dev = blk.dev;
    return block_send(s, blk, na + nb);
}

// The two launches of a reset, the one way an environment gets a new episode: every environment taken is written in the layout that is
// current.  envs_dev: the list form's environments (distinct), else the mask form over all of them.  full: the list names every
// environment (sf_reset), so the handle-wide bookkeeping starts afresh too.
static int reset_launch(sf_sim *s, const int32_t *envs_dev, const uint8_t *mask, const int32_t *xy_dev, int n, bool full = false)
{
    const Geo &g = s->g;
    ResetArgs a;
    memset(&a, 0, sizeof a);
    a.g = g;
    const bool seams = !s->bl_cur && g.ab == 1;       // (the tile bookkeeping is not kept while the blocked plane is current: tiles_valid is false)
    // the tile histograms of a reset environment are known (all UNBURNED, the ignition's tile to be recounted); a partial reset leaves
    // it at that while every histogram of the handle is marked stale anyway
    const bool hist_known = g.ab == 1 && !s->generic && (full || !s->tdirty_all);
    if (full) { s->status_fresh = true; s->cost_steps = 0; }      // every result row is written; the old episodes' costs (run_cost, zeroed) say nothing
    a.n_seg = value_seg(s, a.seg, arrival_seg(s, a.seg, env_segs(s, (kResetKinds & ~(seams ? 0u : kSegSeam) & ~(hist_known ? 0u : kSegHist)) | (full ? kSegCost : 0u), a.seg)));
    a.envs = envs_dev; a.mask = mask; a.xy = xy_dev; a.n = n;
    a.status = s->status; a.age = s->age; a.cells = s->bl_cur ? s->cells : nullptr;
    a.commit = s->commit; a.tflags = s->tflags; a.ring = s->ring; a.vbits = s->vbits; a.win_hint = s->win_hint;
    a.seam = seams ? s->seam : nullptr;
    a.tdirty = hist_known ? s->tdirty : nullptr;
    a.res_block = s->status_block; a.res_sink = s->sink; a.res_elapsed = s->elapsed_dev;
    const unsigned gx = seg_grid_x(a.seg, a.n_seg);
    if (s->rs_timed) HIPCHK(hipEventRecord(s->ev0, s->stream));
    // Whole buffers of a large batch: a memset per slice.  Each costs a few microseconds to enqueue and clears ~14 % faster than the
    // kernel - C3's 2.7 GB in 0.46 ms against 0.50, 1 x 64 x 64 in 59 us against 30 (profiles/reset_paths_ab.txt): even at ~1 GB
    long long bytes = 0;
    for (int k = 0; k < a.n_seg; ++k) bytes += g.E * a.seg[k].len;
    if (full && bytes >= (1LL << 30)) {
        for (int k = 0; k < a.n_seg; ++k) {
            assert(a.seg[k].stride == a.seg[k].len);
            HIPCHK(hipMemsetAsync(a.seg[k].base, 0, (size_t)(g.E * a.seg[k].len), s->stream));
        }
    } else {
        hipLaunchKernelGGL(k_reset_envs, dim3(gx, (unsigned)n), dim3(256), 0, s->stream, a);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_reset_ignite, dim3((n + 255) / 256), dim3(256), 0, s->stream, a);
    HIPCHK(hipGetLastError());
    if (s->rs_timed) { HIPCHK(hipEventRecord(s->ev1, s->stream)); s->rs_have_ms = true; }
    s->tdirty_all = !hist_known;
    return arrival_pass(s);             // the ignitions are the sprites of update 0 (recording off: nothing)
}
// Host ignitions: every one on the grid, or SF_EINVAL in the words of the entry `who` (envs: whose they are, null = 0 .. n - 1).
static int check_ignitions(const sf_sim *s, const char *who, int n, const int32_t *envs, const int32_t *xy)
{
    const Geo &g = s->g;
    for (int i = 0; i < n; ++i)
        if (xy[2 * i] < 0 || xy[2 * i] >= g.W || xy[2 * i + 1] < 0 || xy[2 * i + 1] >= g.H)
            return fail(SF_EINVAL, "%s: ignition (%d, %d) of environment %d is outside the %dx%d grid", who, xy[2 * i], xy[2 * i + 1],
                        envs ? envs[i] : i, g.H, g.W);
    return SF_OK;
}
// The list form from host memory: m distinct environments and their ignitions through the call block, then the launches.
// (sf_get_fire_map_delta: a reset map is all UNBURNED - the caller zeroes its mirror, the next delta reports the ignition)
static int reset_list(sf_sim *s, const int32_t *envs, const int32_t *xy, int m, bool full = false)
{
    uint8_t *dev = nullptr;
    { int rc = reset_stage(s, envs, (size_t)m * 4, xy, (size_t)m * 8, &dev); if (rc) return rc; }
    { int rc = reset_launch(s, reinterpret_cast<const int32_t *>(dev), nullptr, reinterpret_cast<const int32_t *>(dev + (size_t)m * 4), m, full); if (rc) return rc; }
    if (s->snap) for (int i = 0; i < m; ++i) s->snap_valid[envs[i]] = 1;
    return SF_OK;
}

// Every environment, as the list 0 .. E - 1 (without a mask the mask form takes only those that are not running).  Allowed before any
// reset and on a handle a failed team launch has voided; waits whatever `async` says.
extern "C" int sf_reset(sf_sim *s, const int32_t *init_xy)
{
    if (!s || !init_xy) return fail(SF_EINVAL, "sf_reset: null argument");
    const int E = s->g.E;
    { int rc = check_ignitions(s, "reset", E, nullptr, init_xy); if (rc) return rc; }
    { int rc = begin_call(s, "sf_reset", kCommit); if (rc) return rc; }
    // everything is rewritten, nothing to convert: into the blocked plane if the resident launch is what steps this handle
    // (it did last, or nothing has stepped yet and it is the automatic choice), else into the row-major planes
    const bool bl = prefers_bl(s) && (s->bl_cur || s->last_kind == 2 || s->last_kind == -1);
    if (bl) { int rc = alloc_bl(s); if (rc) return rc; }
    s->bl_cur = bl;
    std::vector<int32_t> all((size_t)E);
    for (int e = 0; e < E; ++e) all[e] = e;
    { int rc = reset_list(s, all.data(), init_xy, E, true); if (rc) return rc; }
    { int rc = finish_call(s, nullptr, true, nullptr); if (rc) return rc; }
    s->last_ign.assign(init_xy, init_xy + (size_t)2 * E);      // (where a new episode ignites when sf_episodes_set draws no ignition)
    s->was_reset = true; s->vbits_valid = true; s->vbits_fl_valid = true; s->tiles_valid = !s->bl_cur; s->fire_rows = 1;     // every environment freshly written
    if (s->xerr_pinned) *s->xerr_pinned = 0;      // (cells, bitmaps, states of every environment are new: what a failed team launch left is gone)
    return SF_OK;
}

// One environment: a list of one.  Never refused on a voided handle, and it waits whatever `async` says.
extern "C" int sf_reset_env(sf_sim *s, int32_t env, int32_t x, int32_t y)
{
    if (!s) return fail(SF_EINVAL, "sf_reset_env: null handle");
    if (env < 0 || env >= s->g.E) return fail(SF_EINVAL, "sf_reset_env: environment %d out of range", env);
    if (!s->was_reset) return fail(SF_ESTATE, "sf_reset_env: call sf_reset once first");
    const int32_t xy[2] = {x, y};
    { int rc = check_ignitions(s, "reset", 1, &env, xy); if (rc) return rc; }
    { int rc = begin_call(s, "sf_reset_env", kCommit); if (rc) return rc; }
    { int rc = reset_list(s, &env, xy, 1); if (rc) return rc; }
    return finish_call(s, nullptr, true, nullptr);
}

extern "C" int sf_time_resets(sf_sim *s, int32_t on)
{
    if (!s) return fail(SF_EINVAL, "sf_time_resets: null handle");
    s->rs_timed = on != 0;
    s->rs_have_ms = false;
    return SF_OK;
}

extern "C" int sf_get_reset_ms(sf_sim *s, float *ms_out)
{
    if (!s || !ms_out) return fail(SF_EINVAL, "sf_get_reset_ms: null argument");
    if (!s->rs_have_ms) return fail(SF_ESTATE, "sf_get_reset_ms: no batched reset has been timed (sf_time_resets)");
    HIPCHK(hipSetDevice(s->p.device));
    HIPCHK(hipEventSynchronize(s->ev1));
    HIPCHK(hipEventElapsedTime(ms_out, s->ev0, s->ev1));
    return SF_OK;
}

extern "C" int sf_reset_envs(sf_sim *s, int32_t n, const int32_t *envs, const int32_t *xy)
{
    if (!s) return fail(SF_EINVAL, "sf_reset_envs: null handle");
    if (n < 0 || (n > 0 && (!envs || !xy))) return fail(SF_EINVAL, "sf_reset_envs: bad environment list");
    { int rc = check_envs(s, "sf_reset_envs", n, envs); if (rc) return rc; }      // (a repeated environment is accepted: below)
    { int rc = check_ignitions(s, "sf_reset_envs", n, envs, xy); if (rc) return rc; }
    if (n == 0) return SF_OK;
    { int rc = begin_call(s, "sf_reset_envs", kStateCall); if (rc) return rc; }
    // an environment named twice keeps the last ignition given for it: no two entries of the launch write one environment
    std::vector<int32_t> last((size_t)s->g.E, -1), le, lxy;
    for (int i = 0; i < n; ++i) last[envs[i]] = i;
    for (int i = 0; i < n; ++i)
        if (last[envs[i]] == i) { le.push_back(envs[i]); lxy.push_back(xy[2 * i]); lxy.push_back(xy[2 * i + 1]); }
    { int rc = reset_list(s, le.data(), lxy.data(), (int)le.size()); if (rc) return rc; }
    return finish_call(s, nullptr, !s->async, nullptr);
}

extern "C" int sf_reset_where(sf_sim *s, const uint8_t *device_mask, const int32_t *xy, int32_t xy_device_pointer)
{
    if (!s) return fail(SF_EINVAL, "sf_reset_where: null handle");
    if (!xy) return fail(SF_EINVAL, "sf_reset_where: null ignitions");
    const Geo &g = s->g;
    { int rc = begin_call(s, "sf_reset_where", kStateCall); if (rc) return rc; }
    const int32_t *xy_dev = xy;
    if (!xy_device_pointer) {
        uint8_t *dev = nullptr;
        int rc = reset_stage(s, xy, (size_t)g.E * 8, nullptr, 0, &dev);
        if (rc) return rc;
        xy_dev = reinterpret_cast<const int32_t *>(dev);
    }
    { int rc = reset_launch(s, nullptr, device_mask, xy_dev, g.E); if (rc) return rc; }
    // which environments were taken is known on the device only: no host mirror of a map can be told to zero itself, so the next
    // delta query of every environment hands back the whole map once
    if (s->snap) std::fill(s->snap_valid.begin(), s->snap_valid.end(), 0);
    return finish_call(s, nullptr, !s->async, nullptr);
}

// ----------------------------------------------------------------------------- agents
static int agents_free(sf_sim *s)
{
    if (s->ag_mem) {
        HIPCHK(hipStreamSynchronize(s->stream));      // (enqueued ticks may still use the buffers)
        HIPCHK(hipFree(s->ag_mem));
        s->bytes -= (int64_t)s->ag_bytes;
    }
    s->ag_mem = nullptr; s->ag_bytes = 0;
    s->ag_xyid = s->ag_start = s->ag_points = s->ag_prev = s->ag_terms = s->ag_len = s->ag_ign = nullptr;
    s->ag_ret = nullptr; s->ag_done = nullptr;
    s->ag_has_ign = false;
    s->val_w_on = false;                              // (the fifth weight belongs to the agent state: set again behind sf_agents_create)
    memset(&s->ag, 0, sizeof s->ag);
    return SF_OK;
}

extern "C" int sf_agents_create(sf_sim *s, const sf_agent_params *p, const int32_t *ignitions_xy)
{
    if (!s || !p) return fail(SF_EINVAL, "sf_agents_create: null argument");
    const Geo &g = s->g;
    if (p->k < 0 || p->k > kAgentsMax) return fail(SF_EINVAL, "sf_agents_create: %d agents per environment (1..%d; 0 frees)", p->k, kAgentsMax);
    if (p->k > 0) {
        if (p->n_updates < 1) return fail(SF_EINVAL, "sf_agents_create: n_updates = %d must be >= 1", p->n_updates);
        if (p->max_ticks < 0) return fail(SF_EINVAL, "sf_agents_create: max_ticks = %d must be >= 0", p->max_ticks);
        if (p->auto_reset && !ignitions_xy) return fail(SF_EINVAL, "sf_agents_create: auto_reset needs the ignitions");
        for (int e = 0; ignitions_xy && e < g.E; ++e)
            if (ignitions_xy[2 * e] < 0 || ignitions_xy[2 * e] >= g.W || ignitions_xy[2 * e + 1] < 0 || ignitions_xy[2 * e + 1] >= g.H)
                return fail(SF_EINVAL, "sf_agents_create: ignition (%d, %d) of environment %d is outside the %dx%d grid", ignitions_xy[2 * e],
                            ignitions_xy[2 * e + 1], e, g.H, g.W);
    }
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    { int rc = agents_free(s); if (rc) return rc; }
    if (p->k == 0) return SF_OK;
    // one allocation, every buffer on a 16-byte boundary: xyid | start | points | prev | terms | len | ign | ret | done
    const size_t E = (size_t)g.E, K = (size_t)p->k;
    const size_t sizes[9] = {E * K * 12, E * K * 8, E * K * 12, E * 4, E * 16, E * 4, E * 8, E * 8, E};
    size_t off[9], total = 0;
    for (int i = 0; i < 9; ++i) { off[i] = total; total += (sizes[i] + 15) / 16 * 16; }
    HIPCHK(hipMalloc(reinterpret_cast<void **>(&s->ag_mem), total));
    s->ag_bytes = total; s->bytes += (int64_t)total;
    int32_t **ip[7] = {&s->ag_xyid, &s->ag_start, &s->ag_points, &s->ag_prev, &s->ag_terms, &s->ag_len, &s->ag_ign};
    for (int i = 0; i < 7; ++i) *ip[i] = reinterpret_cast<int32_t *>(s->ag_mem + off[i]);
    s->ag_ret = reinterpret_cast<double *>(s->ag_mem + off[7]);
    s->ag_done = s->ag_mem + off[8];
    std::vector<uint8_t> h(total, 0);
    int32_t *xyid = reinterpret_cast<int32_t *>(h.data() + off[0]);
    for (size_t i = 0; i < E * K; ++i) xyid[3 * i + 2] = (int32_t)(i % K) + 1;
    if (ignitions_xy) memcpy(h.data() + off[6], ignitions_xy, E * 8);
    HIPCHK(hipMemcpyAsync(s->ag_mem, h.data(), total, hipMemcpyHostToDevice, s->stream));
    // (section 19: episodes that draw no ignition re-ignite where these agents' environments do)
    if (ignitions_xy && s->ep_on && !(s->ep.flags & SF_EP_IGNITION)) HIPCHK(hipMemcpyAsync(s->ep_ign, ignitions_xy, E * 8, hipMemcpyHostToDevice, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));          // (h is pageable and leaves scope)
    s->ag = *p;
    s->ag_has_ign = ignitions_xy != nullptr;
    return SF_OK;
}

extern "C" int sf_agents_place(sf_sim *s, int32_t n, const int32_t *envs, const int32_t *xy, int32_t also_start)
{
    if (!s) return fail(SF_EINVAL, "sf_agents_place: null handle");
    if (!s->ag.k) return fail(SF_ESTATE, "sf_agents_place: call sf_agents_create first");
    if (n < 0 || (n > 0 && (!envs || !xy))) return fail(SF_EINVAL, "sf_agents_place: bad environment list");
    const Geo &g = s->g;
    const int K = s->ag.k;
    { int rc = check_envs(s, "sf_agents_place", n, envs); if (rc) return rc; }
    for (long long i = 0; i < (long long)n * K; ++i)
        if (xy[2 * i] < 0 || xy[2 * i] >= g.W || xy[2 * i + 1] < 0 || xy[2 * i + 1] >= g.H)
            return fail(SF_EINVAL, "sf_agents_place: cell (%d, %d) of agent %d of environment %d is outside the %dx%d grid", xy[2 * i],
                        xy[2 * i + 1], (int)(i % K), envs[i / K], g.H, g.W);
    if (n == 0) return SF_OK;
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    // an environment named twice keeps its last entry: no two threads of the launch write one agent
    std::vector<int32_t> last((size_t)g.E, -1), keep;
    for (int i = 0; i < n; ++i) last[envs[i]] = i;
    for (int i = 0; i < n; ++i) if (last[envs[i]] == i) keep.push_back(i);
    const int m = (int)keep.size();
    // the call block: envs [m] | xy [m][K][2]
    const size_t o_xy = ((size_t)m * 4 + 15) / 16 * 16, bytes = o_xy + (size_t)m * K * 8;
    CallBlock &blk = s->ag_blk;
    { int rc = block_reserve(s, blk, bytes); if (rc) return rc; }
    for (int i = 0; i < m; ++i) {
        reinterpret_cast<int32_t *>(blk.pinned)[i] = envs[keep[i]];
        memcpy(blk.pinned + o_xy + (size_t)i * K * 8, xy + (size_t)keep[i] * K * 2, (size_t)K * 8);
    }
    { int rc = block_send(s, blk, bytes); if (rc) return rc; }
    hipLaunchKernelGGL(k_agents_place, dim3((unsigned)((m * K + 255) / 256)), dim3(256), 0, s->stream, m, K,
                       reinterpret_cast<const int32_t *>(blk.dev), reinterpret_cast<const int32_t *>(blk.dev + o_xy), also_start != 0 ? 1 : 0,
                       s->ag_xyid, s->ag_start, s->ag_len, s->ag_ret);
    HIPCHK(hipGetLastError());
    return finish_call(s, nullptr, !s->async, nullptr);
}

extern "C" int sf_agents_device(sf_sim *s, void **xyid)
{
    if (!s || !xyid) return fail(SF_EINVAL, "sf_agents_device: null argument");
    if (!s->ag.k) return fail(SF_ESTATE, "sf_agents_device: call sf_agents_create first");
    *xyid = s->ag_xyid;
    return SF_OK;
}


// ----------------------------------------------------------------------------- drawn episodes
static int episodes_free(sf_sim *s)
{
    if (s->ep_mem) {
        HIPCHK(hipStreamSynchronize(s->stream));      // (enqueued ticks may still use the buffers)
        HIPCHK(hipFree(s->ep_mem));
        s->bytes -= (int64_t)s->ep_bytes;
    }
    s->ep_mem = s->ep_ones = nullptr; s->ep_bytes = 0;
    s->ep_index = s->ep_due_cnt = nullptr;
    s->ep_ign = s->ep_due = nullptr;
    s->ep_wind = s->ep_due_U = s->ep_due_D = nullptr;
    memset(&s->ep, 0, sizeof s->ep);
    s->ep_on = false;
    return SF_OK;
}

// New episodes in the environments the mask takes (null: those that are not running), their parameters drawn first (enqueue layer):
// the draw, the batched reset with the drawn ignitions, then - SF_EP_WIND - the tables of the drawn winds, so that the episode runs
// under its own wind from its first update.  Nothing is read back.
static int episode_begin(sf_sim *s, const uint8_t *mask)
{
    const Geo &g = s->g;
    const sf_episode_params &p = s->ep;
    const bool wind = (p.flags & SF_EP_WIND) != 0;
    bool cached = false;
    if (wind) {
        // the cache of wind-independent terms current for EVERY table (which ones restart is known on the device only), again after
        // anything staled a part of it (mark_tables); without a cache the tables are built from the layers
        const int n_tab = (int)s->rt_set.size();
        bool stale = !s->wterms || s->wt_off;
        for (int t = 0; t < n_tab && !stale; ++t) stale = s->wt_stale[t] != 0;
        cached = !stale;
        if (stale && !s->ep_nocache) {
            std::vector<int32_t> tabs((size_t)n_tab);
            for (int t = 0; t < n_tab; ++t) tabs[t] = t;
            const int rc = ensure_wterms(s, tabs.data(), n_tab);
            if (rc && rc != SF_ENOTSUP) return rc;
            cached = rc == SF_OK;
            s->ep_nocache = !cached;
        }
    }
    EpisodeArgs a;
    memset(&a, 0, sizeof a);
    a.H = g.H; a.W = g.W; a.P = g.P; a.E = g.E;
    a.mask = mask; a.commit = s->commit;
    a.seed = p.seed; a.flags = p.flags;
    for (int i = 0; i < 4; ++i) { a.ign_box[i] = p.ign_box[i]; a.agent_box[i] = p.agent_box[i]; }
    for (int i = 0; i < 2; ++i) { a.U[i] = p.U[i]; a.U_dir[i] = p.U_dir[i]; }
    a.rt = s->rt; a.tab_stride = s->rt_set.size() > 1 ? (long long)8 * g.plane_env : 0;
    a.index = s->ep_index; a.ign = s->ep_ign; a.wind = s->ep_wind;
    a.K = (p.flags & SF_EP_AGENTS) ? s->ag.k : 0;
    a.start = s->ag_start; a.xyid = s->ag_xyid;
    a.due_cnt = s->ep_due_cnt; a.due = s->ep_due; a.due_U = s->ep_due_U; a.due_D = s->ep_due_D;
    if (wind) HIPCHK(hipMemsetAsync(s->ep_due_cnt, 0, sizeof(uint32_t), s->stream));
    hipLaunchKernelGGL(k_episode_draw, dim3((unsigned)g.E), dim3(kEpAttempts), 0, s->stream, a);
    HIPCHK(hipGetLastError());
    { int rc = reset_launch(s, nullptr, mask, s->ep_ign, g.E); if (rc) return rc; }
    // (section 15's bookkeeping of the mask form: which environments were taken is known on the device only)
    if (s->snap) std::fill(s->snap_valid.begin(), s->snap_valid.end(), 0);
    if (wind) {
        int rc = wind_launch(s, s->ep_due, s->ep_due_cnt, 0, g.E, s->ep_due_U, s->ep_due_D, 0, cached);
        if (rc) return rc;
        // rtc_stale as in sf_set_wind: where the cell-major buffer exists the pass has written the listed tables' copies too (a copy
        // that was stale is no worse for it); where it does not, every table is marked stale when it is allocated (ensure_rtc)
    }
    return SF_OK;
}

extern "C" int sf_episodes_set(sf_sim *s, const sf_episode_params *p)
{
    const char *who = "sf_episodes_set";
    if (!s) return fail(SF_EINVAL, "%s: null handle", who);
    const Geo &g = s->g;
    if (p) {
        if (p->flags & ~(SF_EP_IGNITION | SF_EP_LIVE_CELL | SF_EP_WIND | SF_EP_AGENTS)) return fail(SF_EINVAL, "%s: unknown flags 0x%x", who, p->flags);
        if (p->reserved != 0) return fail(SF_EINVAL, "%s: reserved must be 0", who);
        if ((p->flags & SF_EP_LIVE_CELL) && !(p->flags & SF_EP_IGNITION)) return fail(SF_EINVAL, "%s: SF_EP_LIVE_CELL needs SF_EP_IGNITION", who);
        const struct { int flag; const int32_t *box; const char *name; } boxes[2] = {{SF_EP_IGNITION, p->ign_box, "ign_box"}, {SF_EP_AGENTS, p->agent_box, "agent_box"}};
        for (const auto &b : boxes)
            if ((p->flags & b.flag) && (b.box[0] < 0 || b.box[1] < 0 || b.box[2] >= g.W || b.box[3] >= g.H || b.box[0] > b.box[2] || b.box[1] > b.box[3]))
                return fail(SF_EINVAL, "%s: %s (%d, %d, %d, %d) is not x0 <= x1, y0 <= y1 on the %dx%d grid", who, b.name, b.box[0], b.box[1], b.box[2], b.box[3], g.H, g.W);
        if (p->flags & SF_EP_WIND) {
            const bool ok = std::isfinite(p->U[0]) && std::isfinite(p->U[1]) && std::isfinite(p->U_dir[0]) && std::isfinite(p->U_dir[1]) &&
                            p->U[0] >= 0.0 && p->U[0] <= p->U[1] && p->U_dir[0] <= p->U_dir[1];
            if (!ok) return fail(SF_EINVAL, "%s: wind ranges U [%g, %g], U_dir [%g, %g] must be finite with lo <= hi and U >= 0", who, p->U[0], p->U[1], p->U_dir[0], p->U_dir[1]);
            if (!s->p.per_env_terrain) return fail(SF_ESTATE, "%s: SF_EP_WIND: this handle shares one terrain between all environments (create it with per_env_terrain = 1)", who);
            for (size_t t = 0; t < s->rd_lay.size(); ++t)
                if (!s->rd_lay[t]) return fail(SF_ESTATE, "%s: SF_EP_WIND: table %d has no layers (sf_set_layers*, sf_generate_layers)", who, (int)t);
            if (!s->wind_sched.empty()) return fail(SF_ESTATE, "%s: SF_EP_WIND while a wind schedule is set (sf_set_wind_schedule): the two would fight over the table", who);
        }
        if (!(p->flags & SF_EP_IGNITION) && !(s->ag.k && s->ag_has_ign) && s->last_ign.empty())
            return fail(SF_ESTATE, "%s: without SF_EP_IGNITION new episodes ignite where the environment last did: call sf_reset or sf_agents_create (with ignitions) first", who);
    }
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    { int rc = episodes_free(s); if (rc) return rc; }
    if (!p) return SF_OK;
    // one allocation, every buffer on a 16-byte boundary: index | ign | wind | due | due_cnt | due_U | due_D | ones
    const size_t E = (size_t)g.E;
    const size_t sizes[8] = {E * 4, E * 8, E * 16, E * 4, 4, E * 8, E * 8, E};
    size_t off[8], total = 0;
    for (int i = 0; i < 8; ++i) { off[i] = total; total += (sizes[i] + 15) / 16 * 16; }
    HIPCHK(hipMalloc(reinterpret_cast<void **>(&s->ep_mem), total));
    s->ep_bytes = total; s->bytes += (int64_t)total;
    s->ep_index = reinterpret_cast<uint32_t *>(s->ep_mem + off[0]);
    s->ep_ign = reinterpret_cast<int32_t *>(s->ep_mem + off[1]);
    s->ep_wind = reinterpret_cast<double *>(s->ep_mem + off[2]);
    s->ep_due = reinterpret_cast<int32_t *>(s->ep_mem + off[3]);
    s->ep_due_cnt = reinterpret_cast<uint32_t *>(s->ep_mem + off[4]);
    s->ep_due_U = reinterpret_cast<double *>(s->ep_mem + off[5]);
    s->ep_due_D = reinterpret_cast<double *>(s->ep_mem + off[6]);
    s->ep_ones = s->ep_mem + off[7];
    std::vector<uint8_t> h(total, 0);
    memset(h.data() + off[7], 1, E);
    const bool from_agents = s->ag.k && s->ag_has_ign;
    if (!(p->flags & SF_EP_IGNITION) && !from_agents) memcpy(h.data() + off[1], s->last_ign.data(), E * 8);
    HIPCHK(hipMemcpyAsync(s->ep_mem, h.data(), total, hipMemcpyHostToDevice, s->stream));
    if (!(p->flags & SF_EP_IGNITION) && from_agents) HIPCHK(hipMemcpyAsync(s->ep_ign, s->ag_ign, E * 8, hipMemcpyDeviceToDevice, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));          // (h is pageable and leaves scope)
    s->ep = *p;
    s->ep_on = true;
    s->ep_nocache = false;
    return SF_OK;
}

extern "C" int sf_episodes_begin(sf_sim *s, const uint8_t *device_mask, int32_t all)
{
    const char *who = "sf_episodes_begin";
    if (!s) return fail(SF_EINVAL, "%s: null handle", who);
    if (!s->ep_on) return fail(SF_ESTATE, "%s: call sf_episodes_set first", who);
    const bool tables = (s->ep.flags & (SF_EP_LIVE_CELL | SF_EP_WIND)) != 0;      // the draw reads, or the wind pass rebuilds, R tables
    { int rc = begin_call(s, who, kStateCall | (tables ? kNeedRt : 0)); if (rc) return rc; }
    { int rc = episode_begin(s, all ? s->ep_ones : device_mask); if (rc) return rc; }
    return finish_call(s, nullptr, !s->async, nullptr);
}

extern "C" int sf_episodes_device(sf_sim *s, void **index, void **ignition, void **wind)
{
    if (!s) return fail(SF_EINVAL, "sf_episodes_device: null handle");
    if (!index || !ignition || !wind) return fail(SF_EINVAL, "sf_episodes_device: null argument");
    if (!s->ep_on) return fail(SF_ESTATE, "sf_episodes_device: call sf_episodes_set first");
    *index = s->ep_index; *ignition = s->ep_ign; *wind = s->ep_wind;
    return SF_OK;
}

static AgentArgs agent_args(const sf_sim *s, const int32_t *actions, const sf_agent_out *out)
{
    AgentArgs a;
    memset(&a, 0, sizeof a);
    a.g = s->g;
    a.status = s->status;
    a.cells = s->bl_cur ? s->cells : nullptr;        // (whichever plane is current NOW: the step between the two kernels may change it)
    a.rows = s->status_block;
    a.actions = actions;
    a.xyid = s->ag_xyid; a.start = s->ag_start; a.points = s->ag_points; a.prev_cnt = s->ag_prev; a.terms = s->ag_terms;
    a.ep_len = s->ag_len; a.ep_ret = s->ag_ret; a.done = s->ag_done;
    a.K = s->ag.k; a.only_unburned = s->ag.only_unburned != 0; a.done_on_burn = s->ag.done_on_burn != 0;
    a.max_ticks = s->ag.max_ticks; a.auto_reset = s->ag.auto_reset != 0;
    for (int i = 0; i < 4; ++i) a.w[i] = (double)s->ag.w[i];
    if (s->val_plane) {
        a.damage = s->val_aux; a.damage_stride = (long long)sizeof(ValueRec);
        a.tick_base = s->val_tick(0); a.tick_loss = s->val_tick(1);
        a.wv = (double)s->val_w; a.wv_on = s->val_w_on ? 1 : 0;
    }
    if (out) { a.o_reward = out->reward; a.o_done = out->done; a.o_terms = out->terms; a.o_len = out->final_len; a.o_ret = out->final_ret; }
    return a;
}

// One tick for every environment, nothing read back, every piece from the enqueue layer: result rows -> k_agents_act -> one update
// with the device points, then the plain updates -> result rows -> k_agents_finish -> the batched reset with the done mask.
extern "C" int sf_agents_step(sf_sim *s, const int32_t *device_actions, const sf_agent_out *out)
{
    if (!s) return fail(SF_EINVAL, "sf_agents_step: null handle");
    if (!s->ag.k) return fail(SF_ESTATE, "sf_agents_step: call sf_agents_create first");
    if (!device_actions) return fail(SF_EINVAL, "sf_agents_step: null actions");
    const Geo &g = s->g;
    { int rc = begin_call(s, "sf_agents_step", kNeedRt | kStateCall); if (rc) return rc; }
    note_result_look(s);
    int rc = refresh_status(s, nullptr);             // r0: the rows as a status query leaves them
    const int32_t *pts = nullptr;
    if (!rc) rc = stage_lines(s, 1, s->ag_points, s->ag.k, 1, &pts);
    if (!rc) {
        hipLaunchKernelGGL(k_agents_act, dim3((unsigned)g.E), dim3(kAgentsMax), 0, s->stream, agent_args(s, device_actions, out));
        const StepPlan plan = plan_step(s, 1, true);         // one update with the device points: inside the resident launch, or a pair
        rc = plan.nw ? enqueue_call(s, plan, 1, pts, s->ag.k, false, nullptr) : enqueue_pair(s, pts, s->ag.k, 0, nullptr);
        if (!rc && s->arr_pending) rc = arrival_pass(s);
    }
    if (!rc) rc = step_impl(s, s->ag.n_updates - 1, false, nullptr);
    if (!rc) { note_result_look(s); rc = refresh_status(s, nullptr); }      // r1 (commits the step rings too)
    if (!rc) {
        hipLaunchKernelGGL(k_agents_finish, dim3((unsigned)g.E), dim3(kAgentsMax), 0, s->stream, agent_args(s, device_actions, out));
        if (s->ag.auto_reset && s->ep_on) rc = episode_begin(s, s->ag_done);      // section 19: the new episodes are drawn
        else if (s->ag.auto_reset) {
            rc = reset_launch(s, nullptr, s->ag_done, s->ag_ign, g.E);
            // (section 15's bookkeeping of the mask form: which environments were taken is known on the device only)
            if (!rc && s->snap) std::fill(s->snap_valid.begin(), s->snap_valid.end(), 0);
        }
    }
    return rc ? rc : finish_call(s, "sf_agents_step", !s->async, nullptr);
}

extern "C" int sf_state_bytes(sf_sim *s, int64_t *bytes_out)
{
    if (!s || !bytes_out) return fail(SF_EINVAL, "sf_state_bytes: null argument");
    *bytes_out = state_layout(s->g, s->parents != nullptr, s->arrival1 != nullptr).bytes;
    return SF_OK;
}

extern "C" int sf_save_state(sf_sim *s, int32_t n, const int32_t *envs, void *out, int32_t device_pointer)
{
    if (!s) return fail(SF_EINVAL, "sf_save_state: null handle");
    { int rc = state_list(s, n, envs, out, device_pointer, "sf_save_state", false); if (rc) return rc; }
    if (n == 0) return SF_OK;
    { int rc = begin_call(s, "sf_save_state", kStateCall); if (rc) return rc; }
    // the result rows travel with the state: made current as a status query would, but a snapshot is not a look at the result of a
    // single update (no note_result_look: the run(1)-loop heuristic stays as it was)
    { int rc = refresh_status(s, nullptr); if (rc) return rc; }
    StateArgs a = state_args(s);
    a.hdr = state_header(s);
    const int chunk = state_chunk(a, device_pointer != 0);
    if (!device_pointer) { int rc = ensure_stage(s, (size_t)chunk * a.stride); if (rc) return rc; }
    for (int i0 = 0; i0 < n; i0 += chunk) {
        const int cnt = std::min(chunk, n - i0);
        a.n = cnt;
        for (int i = 0; i < cnt; ++i) a.env[i] = envs[i0 + i];
        uint8_t *dst = device_pointer ? static_cast<uint8_t *>(out) + (size_t)i0 * a.stride : static_cast<uint8_t *>(s->stage);
        a.blob = dst;
        hipLaunchKernelGGL(k_state_pack, dim3((unsigned)((a.g.W + 255) / 256), (unsigned)a.g.H, (unsigned)cnt), dim3(256), 0, s->stream, a);
        HIPCHK(hipGetLastError());
        if (!device_pointer) {
            HIPCHK(hipMemcpyAsync(static_cast<uint8_t *>(out) + (size_t)i0 * a.stride, s->stage, (size_t)cnt * a.stride, hipMemcpyDeviceToHost, s->stream));
            HIPCHK(hipStreamSynchronize(s->stream));
        }
    }
    if (device_pointer && !s->async) HIPCHK(hipStreamSynchronize(s->stream));
    return check_team_error(s, "sf_save_state");
}

extern "C" int sf_load_state(sf_sim *s, int32_t n, const int32_t *envs, const void *in, int32_t device_pointer)
{
    if (!s) return fail(SF_EINVAL, "sf_load_state: null handle");
    { int rc = state_list(s, n, envs, in, device_pointer, "sf_load_state", true); if (rc) return rc; }
    if (n == 0) return SF_OK;
    HIPCHK(hipSetDevice(s->p.device));
    const long long bytes = state_layout(s->g, s->parents != nullptr, s->arrival1 != nullptr).bytes;
    // every header is looked at before anything changes (a refused call leaves the handle as it was)
    std::vector<StateHeader> hdr((size_t)n);
    if (device_pointer) {
        LOOP_QUIESCE(s);
        HIPCHK(hipMemcpy2DAsync(hdr.data(), sizeof(StateHeader), in, (size_t)bytes, sizeof(StateHeader), (size_t)n, hipMemcpyDeviceToHost, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));      // (the blobs may come from a save enqueued in front)
    } else {
        for (int i = 0; i < n; ++i) memcpy(&hdr[i], static_cast<const uint8_t *>(in) + (size_t)i * bytes, sizeof(StateHeader));
    }
    int fire_rows = 0;
    for (int i = 0; i < n; ++i) {
        int rc = header_check(s, hdr[i], i);
        if (rc) return rc;
        fire_rows = std::max(fire_rows, hdr[i].fire_rows > 0 ? hdr[i].fire_rows : INT32_MAX);
    }
    { int rc = begin_call(s, "sf_load_state", kStateCall); if (rc) return rc; }
    const Geo &g = s->g;
    StateArgs a = state_args(s);
    const int chunk = state_chunk(a, device_pointer != 0);
    if (!device_pointer) { int rc = ensure_stage(s, (size_t)chunk * a.stride); if (rc) return rc; }
    const bool per_env_tiles = !s->bl_cur && s->tiles_valid;      // the tile maps / seams are kept: rebuild this environment's
    const bool recount = g.ab == 1 && !s->generic && !s->tdirty_all;
    EnvSeg seg[kEnvSegs];
    const int n_seg = env_segs(s, kSegCells | kSegHint, seg);
    for (int i0 = 0; i0 < n; i0 += chunk) {
        const int cnt = std::min(chunk, n - i0);
        a.n = cnt;
        for (int i = 0; i < cnt; ++i) a.env[i] = envs[i0 + i];
        if (device_pointer) a.blob = const_cast<uint8_t *>(static_cast<const uint8_t *>(in)) + (size_t)i0 * a.stride;
        else {
            HIPCHK(hipMemcpyAsync(s->stage, static_cast<const uint8_t *>(in) + (size_t)i0 * a.stride, (size_t)cnt * a.stride, hipMemcpyHostToDevice, s->stream));
            a.blob = static_cast<uint8_t *>(s->stage);
        }
        for (int i = 0; i < cnt; ++i) {      // the cell planes start from zero: guard rows / quads and the pitch padding stay zero; so does the window advice (about a fire that is not there)
            const int e = a.env[i];
            for (int k = 0; k < n_seg; ++k) HIPCHK(hipMemsetAsync(seg[k].base + e * seg[k].stride, 0, (size_t)seg[k].len, s->stream));
            if (recount) HIPCHK(hipMemsetAsync(s->tdirty + (size_t)e * g.TY * g.TX, 1, (size_t)g.TY * g.TX, s->stream));
        }
        hipLaunchKernelGGL(k_state_unpack, dim3((unsigned)((g.P + 255) / 256), (unsigned)g.H, (unsigned)cnt), dim3(256), 0, s->stream, a);
        hipLaunchKernelGGL(k_state_vbits, dim3((unsigned)g.VW, (unsigned)g.H, (unsigned)cnt), dim3(64), 0, s->stream, a);
        HIPCHK(hipGetLastError());
        if (per_env_tiles)
            for (int i = 0; i < cnt; ++i) {
                int rc = rebuild_tflags(s, a.env[i], 1);
                if (!rc) rc = rebuild_seams(s, a.env[i], 1);
                if (rc) return rc;
            }
        if (!device_pointer) HIPCHK(hipStreamSynchronize(s->stream));      // (the staging buffer is reused by the next pass)
    }
    if (s->bl_cur) s->tiles_valid = false;
    { int rc = wind_forget(s, envs, n); if (rc) return rc; }      // (a scheduled environment's table stands for the update count it had: decided anew)
    for (int i = 0; i < n; ++i) if (s->snap) s->snap_valid[envs[i]] = 0;
    // fire_rows bounds every environment's fire: the saving handle's bound covers a loaded one (a blob without one makes it unknown)
    s->fire_rows = (s->fire_rows > 0 && fire_rows != INT32_MAX) ? std::max(s->fire_rows, fire_rows) : 0;
    { int rc = value_recount(s); if (rc) return rc; }      // section 20: the restored planes say what counts
    if (device_pointer && !s->async) HIPCHK(hipStreamSynchronize(s->stream));
    return SF_OK;
}

// The result block made current on the device (enqueue layer), also written to copy_to (may be null) and the registered sink.
static int refresh_status(sf_sim *s, int32_t *copy_to)
{
    const Geo &g = s->g;
    { int rc0 = ensure_commit(s); if (rc0) return rc0; }
    if (s->status_fresh) {
        // the resident launch has left the block (and the registered sink's copy) behind: nothing to count
        if (copy_to && copy_to != s->sink)
            HIPCHK(hipMemcpyAsync(copy_to, s->status_block, sizeof(int32_t) * 8 * g.E, hipMemcpyDeviceToDevice, s->stream));
        return SF_OK;
    }
    int32_t *sink2 = s->sink && s->sink != copy_to ? s->sink : nullptr;       // the registered sink follows every refresh
    if (g.ab == 1 && !s->generic) {
        // per-tile histograms: only the tiles touched since the last query are recounted; one launch writes the whole block
        if (s->tdirty_all) HIPCHK(hipMemsetAsync(s->tdirty, 1, s->n_tiles_max, s->stream));
        s->tdirty_all = false;
        hipLaunchKernelGGL(k_counts_tiles, dim3((unsigned)g.E), dim3(1024), 0, s->stream, g, (const uint8_t *)s->status, (const uint8_t *)(s->bl_cur ? s->cells : nullptr), s->tdirty, s->thist,
                           (const EnvState *)s->commit, s->status_block, s->elapsed_dev, copy_to ? copy_to : sink2);
        if (copy_to && sink2) HIPCHK(hipMemcpyAsync(sink2, s->status_block, sizeof(int32_t) * 8 * g.E, hipMemcpyDeviceToDevice, s->stream));
        s->status_fresh = true;            // (the block - and the registered sink's copy - is current until something changes a status byte)
    } else {
        { int rc0 = ensure_rm(s); if (rc0) return rc0; }
        HIPCHK(hipMemsetAsync(s->status_block, 0, sizeof(int32_t) * 8 * g.E, s->stream));
        int bx = g.H < 64 ? g.H : 64;
        hipLaunchKernelGGL(k_counts, dim3(bx, g.E), dim3(256), 0, s->stream, g, (const uint8_t *)s->status,
                           (const EnvState *)s->commit, s->status_block);
        s->tdirty_all = true;
        hipLaunchKernelGGL(k_elapsed, dim3((g.E + 255) / 256), dim3(256), 0, s->stream, g.E, (const EnvState *)s->commit,
                           s->elapsed_dev);
        if (copy_to) HIPCHK(hipMemcpyAsync(copy_to, s->status_block, sizeof(int32_t) * 8 * g.E, hipMemcpyDeviceToDevice, s->stream));
        if (sink2) HIPCHK(hipMemcpyAsync(sink2, s->status_block, sizeof(int32_t) * 8 * g.E, hipMemcpyDeviceToDevice, s->stream));
    }
    HIPCHK(hipGetLastError());
    return SF_OK;
}
// What a status query does first (call layer): the prologue, the note of the look, the refresh.
static int status_query(sf_sim *s, const char *who, int32_t *copy_to)
{
    { int rc = begin_call(s, who, 0); if (rc) return rc; }
    note_result_look(s);
    return refresh_status(s, copy_to);
}

extern "C" int sf_update_status_device(sf_sim *s)
{
    if (!s) return fail(SF_EINVAL, "sf_update_status_device: null handle");
    const int rc = status_query(s, "sf_update_status_device", nullptr);
    return rc ? rc : finish_call(s, nullptr, true, nullptr);
}

extern "C" int sf_get_status(sf_sim *s, int32_t *status, double *elapsed)
{
    if (!s || !status) return fail(SF_EINVAL, "sf_get_status: null argument");
    int rc = status_query(s, "sf_get_status", nullptr);
    if (rc) return rc;
    const size_t nb_st = sizeof(int32_t) * 8 * s->g.E, nb_el = sizeof(double) * s->g.E;
    if (!s->status_pinned) HIPCHK(hipHostMalloc(&s->status_pinned, nb_st + nb_el, hipHostMallocDefault));
    char *pin = (char *)s->status_pinned;
    HIPCHK(hipMemcpyAsync(pin, s->status_block, nb_st, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipMemcpyAsync(pin + nb_st, s->elapsed_dev, nb_el, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    memcpy(status, pin, nb_st);
    if (elapsed) memcpy(elapsed, pin + nb_st, nb_el);
    return check_team_error(s, "sf_get_status");
}

extern "C" int sf_enable_counters(sf_sim *s, int32_t on)
{
    if (!s) return fail(SF_EINVAL, "sf_enable_counters: null handle");
    s->counters_on = on != 0;
    return SF_OK;
}

extern "C" int sf_get_counters(sf_sim *s, int64_t *out, int32_t reset)
{
    if (!s || !out) return fail(SF_EINVAL, "sf_get_counters: null argument");
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    HIPCHK(hipStreamSynchronize(s->stream));
    std::vector<unsigned long long> h((size_t)kCounterShards * kCounterRow);
    HIPCHK(hipMemcpy(h.data(), s->counters, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (int k = 0; k < kCounterRow; ++k) out[k] = 0;
    for (int i = 0; i < kCounterShards; ++i)
        for (int k = 0; k < kCounterRow; ++k) out[k] += (int64_t)h[(size_t)i * kCounterRow + k];
    if (reset) HIPCHK(hipMemset(s->counters, 0, h.size() * sizeof(unsigned long long)));
    return SF_OK;
}

extern "C" int sf_copy_status_to(sf_sim *s, void *device_dst)
{
    if (!s || !device_dst) return fail(SF_EINVAL, "sf_copy_status_to: null argument");
    int rc = status_query(s, "sf_copy_status_to", static_cast<int32_t *>(device_dst));       // (the counting kernel writes the copy too)
    return rc ? rc : finish_call(s, "sf_copy_status_to", true, nullptr);       // (one wait for steps still in flight and the count)
}

extern "C" int sf_rollout(sf_sim *s, int32_t n_steps, void *device_dst)
{
    if (!s || !device_dst) return fail(SF_EINVAL, "sf_rollout: null argument");
    if (n_steps < 0) return fail(SF_EINVAL, "sf_rollout: n_steps must be >= 0");
    int rc = begin_call(s, "sf_rollout", kNeedRt | kNeedReset);
    if (!rc) rc = step_impl(s, n_steps, false, nullptr);
    if (rc) return rc;
    note_result_look(s);
    rc = refresh_status(s, static_cast<int32_t *>(device_dst));
    return rc ? rc : finish_call(s, "sf_rollout", !s->async, nullptr);      // (asynchronous mode: enqueued, not waited for - sf_sync / the caller's device synchronisation)
}

extern "C" int sf_set_result_sink(sf_sim *s, void *device_dst)
{
    if (!s) return fail(SF_EINVAL, "sf_set_result_sink: null handle");
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    HIPCHK(hipStreamSynchronize(s->stream));       // nothing in flight may still write the old sink
    s->sink = static_cast<int32_t *>(device_dst);
    s->status_fresh = false;                       // the new sink is filled by the next refresh
    return SF_OK;
}

// ---- the one collective: RCCL through dlopen, so that a one-GPU host needs no librccl
namespace {
struct RcclApi {
    void *lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
};
RcclApi g_rccl;
int rccl_load()
{
    if (g_rccl.lib) return SF_OK;
    // (SIMFIRE_RCCL_LIB: another library with the same five entry points - the tests' single-process stand-in, tests/fake_rccl.cpp,
    // which lets 8 handles on ONE GPU play the 8 ranks of a node; never set in production)
    const char *names[] = {getenv("SIMFIRE_RCCL_LIB"), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void *lib = nullptr;
    for (const char *n : names) if (n && *n && (lib = dlopen(n, RTLD_NOW | RTLD_LOCAL))) break;
    if (!lib) return fail(SF_ERCCL, "librccl.so could not be loaded: %s", dlerror());
    RcclApi a;
    a.lib = lib;
    a.GetUniqueId = reinterpret_cast<decltype(a.GetUniqueId)>(dlsym(lib, "ncclGetUniqueId"));
    a.CommInitRank = reinterpret_cast<decltype(a.CommInitRank)>(dlsym(lib, "ncclCommInitRank"));
    a.AllGather = reinterpret_cast<decltype(a.AllGather)>(dlsym(lib, "ncclAllGather"));
    a.CommDestroy = reinterpret_cast<decltype(a.CommDestroy)>(dlsym(lib, "ncclCommDestroy"));
    a.GetErrorString = reinterpret_cast<decltype(a.GetErrorString)>(dlsym(lib, "ncclGetErrorString"));
    if (!a.GetUniqueId || !a.CommInitRank || !a.AllGather || !a.CommDestroy || !a.GetErrorString) {
        dlclose(lib);
        return fail(SF_ERCCL, "librccl.so lacks one of ncclGetUniqueId / ncclCommInitRank / ncclAllGather / ncclCommDestroy / ncclGetErrorString");
    }
    g_rccl = a;
    return SF_OK;
}
#define RCCLCHK(x) do { ncclResult_t _r = (x); if (_r != ncclSuccess) return fail(SF_ERCCL, "%s failed: %s", #x, g_rccl.GetErrorString(_r)); } while (0)
}  // namespace

extern "C" int sf_comm_unique_id(void *id_out)
{
    if (!id_out) return fail(SF_EINVAL, "sf_comm_unique_id: null argument");
    static_assert(sizeof(ncclUniqueId) == 128, "the header promises 128 bytes");
    { int rc = rccl_load(); if (rc) return rc; }
    ncclUniqueId id;
    RCCLCHK(g_rccl.GetUniqueId(&id));
    std::memcpy(id_out, &id, sizeof id);
    return SF_OK;
}

extern "C" int sf_comm_destroy(sf_sim *s) { return s ? comm_close(s) : fail(SF_EINVAL, "sf_comm_destroy: null handle"); }
static int comm_close(sf_sim *s)
{
    if (!s->comm) return SF_OK;
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    HIPCHK(hipStreamSynchronize(s->stream));
    ncclComm_t c = s->comm;
    s->comm = nullptr; s->comm_world = 0;
    RCCLCHK(g_rccl.CommDestroy(c));
    return SF_OK;
}

extern "C" int sf_comm_init(sf_sim *s, int32_t rank, int32_t world_size, const void *unique_id)
{
    if (!s || !unique_id) return fail(SF_EINVAL, "sf_comm_init: null argument");
    if (world_size < 1 || rank < 0 || rank >= world_size) return fail(SF_EINVAL, "sf_comm_init: rank %d of %d", rank, world_size);
    { int rc = rccl_load(); if (rc) return rc; }
    { int rc = comm_close(s); if (rc) return rc; }
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    ncclUniqueId id;
    std::memcpy(&id, unique_id, sizeof id);
    RCCLCHK(g_rccl.CommInitRank(&s->comm, world_size, id, rank));
    s->comm_world = world_size;
    return SF_OK;
}

extern "C" int sf_allgather_status(sf_sim *s, void *device_out)
{
    if (!s || !device_out) return fail(SF_EINVAL, "sf_allgather_status: null argument");
    if (!s->comm) return fail(SF_ESTATE, "sf_allgather_status: call sf_comm_init first");
    int rc = status_query(s, "sf_allgather_status", nullptr);      // the block of this rank's shard (fresh already after a resident launch)
    if (rc) return rc;
    // on the handle's stream: behind the steps in flight and the refresh, no host wait in between
    RCCLCHK(g_rccl.AllGather(s->status_block, device_out, (size_t)8 * s->g.E, ncclInt32, s->comm, s->stream));
    return finish_call(s, "sf_allgather_status", true, nullptr);
}

extern "C" int sf_status_device(sf_sim *s, void **ptr)
{
    if (!s || !ptr) return fail(SF_EINVAL, "sf_status_device: null argument");
    *ptr = s->status_block;
    return SF_OK;
}

extern "C" int sf_fire_map_device(sf_sim *s, void **ptr, int64_t *row_pitch, int64_t *env_stride)
{
    if (!s || !ptr || !row_pitch || !env_stride) return fail(SF_EINVAL, "sf_fire_map_device: null argument");
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    if (s->bl_cur) {
        // the resident launch keeps the cells in its blocked plane: the row-major status plane is refreshed from it (one sweep) and
        // is a snapshot until the next call - the blocked plane stays the current one, nothing is converted back
        const Geo &g = s->g;
        hipLaunchKernelGGL(k_bl_to_rm, dim3((g.PV + 63) / 64, g.H, g.E), dim3(64), 0, s->stream, g, (const uint8_t *)s->cells, s->status, (uint8_t *)nullptr);
        HIPCHK(hipGetLastError());
    } else { s->tdirty_all = true; s->status_fresh = false; }      // the caller holds a writable alias of the status plane: recount everything at the next query
    HIPCHK(hipStreamSynchronize(s->stream));
    *ptr = s->status; *row_pitch = s->g.P; *env_stride = s->g.plane_env;
    return SF_OK;
}

// ----------------------------------------------------------------------------- observations
extern "C" int sf_cell_layout(sf_sim *s, int32_t *blocked)
{
    if (!s || !blocked) return fail(SF_EINVAL, "sf_cell_layout: null argument");
    *blocked = s->bl_cur ? 1 : 0;
    return SF_OK;
}

// Output cells per k_observe workgroup (TX x TY) for pool factor f and output width ow, and the LDS row stride of its staged region:
// up to 256 outputs, fewer as f grows, so that the region (TY * f rows of whole vectors) fits kObsLds.
struct ObsTile { int TX, TY, stride; };
static ObsTile obs_tile(int f, int ow)
{
    int outs = kObsThreads;
    while (outs > 1 && (long long)outs * f * f > 16384) outs >>= 1;
    for (;;) {
        int tx = 1;
        while (tx * 2 <= outs && tx * 2 <= 64 && tx < ow) tx *= 2;
        ObsTile t{tx, outs / tx, (tx * f + 30) / 16 * 16};
        if ((long long)t.TY * f * t.stride <= kObsLds || outs == 1) return t;
        outs >>= 1;
    }
}

extern "C" int sf_observe(sf_sim *s, const sf_obs_params *p, int32_t n, const int32_t *envs, void *device_out)
{
    if (!s || !p) return fail(SF_EINVAL, "sf_observe: null argument");
    const Geo &g = s->g;
    if (n < 0 || (n > 0 && (!envs || !device_out))) return fail(SF_EINVAL, "sf_observe: bad environment list or output");
    const int C = p->n_channels;
    if (C < 1 || C > SF_OBS_MAX_CHANNELS) return fail(SF_EINVAL, "sf_observe: %d channels (1..%d)", C, SF_OBS_MAX_CHANNELS);
    bool attr = false, agents = false;
    for (int c = 0; c < C; ++c) {
        if (p->channels[c] < SF_OBS_FIRE_MAP || p->channels[c] > SF_OBS_AGENTS)
            return fail(SF_EINVAL, "sf_observe: channel %d has the unknown code %d", c, p->channels[c]);
        if (p->pool_mode[c] != 0 && p->pool_mode[c] != 1) return fail(SF_EINVAL, "sf_observe: channel %d has the pool mode %d (0 mean, 1 max)", c, p->pool_mode[c]);
        attr |= p->channels[c] >= SF_OBS_W_0 && p->channels[c] <= SF_OBS_WIND_DIRECTION;
        agents |= p->channels[c] == SF_OBS_AGENTS;
    }
    const int f = p->pool;
    if (f < 1 || f > SF_OBS_MAX_POOL) return fail(SF_EINVAL, "sf_observe: pool %d (1..%d)", f, SF_OBS_MAX_POOL);
    const bool crop = p->crop_h != 0 || p->crop_w != 0;
    if (crop && (p->crop_h < 1 || p->crop_w < 1 || p->crop_h > 65535 || p->crop_w > 65535))
        return fail(SF_EINVAL, "sf_observe: crop %d x %d", p->crop_h, p->crop_w);
    if (crop && !p->centers) return fail(SF_EINVAL, "sf_observe: a crop needs centers");
    const int eh = crop ? p->crop_h : g.H, ew = crop ? p->crop_w : g.W;
    if (eh % f || ew % f) return fail(SF_EINVAL, "sf_observe: the extent %d x %d is not divisible by pool %d", eh, ew, f);
    if (p->dtype != 0 && p->dtype != 1) return fail(SF_EINVAL, "sf_observe: dtype %d (0 float32, 1 bfloat16)", p->dtype);
    const int k = agents && p->agents ? p->agents_k : 0;
    if (agents && p->agents && (p->agents_k < 0 || p->agents_k > SF_OBS_MAX_AGENTS))
        return fail(SF_EINVAL, "sf_observe: %d agents per environment (0..%d)", p->agents_k, SF_OBS_MAX_AGENTS);
    if ((uintptr_t)device_out & (p->dtype ? 1 : 3)) return fail(SF_EINVAL, "sf_observe: the output is not aligned to its element");
    { int rc = check_envs(s, "sf_observe", n, envs); if (rc) return rc; }
    if (n == 0) return SF_OK;
    if (attr && !s->have_rt) return fail(SF_ESTATE, "sf_observe: attribute channels need the layers (sf_set_layers)");
    { int rc = begin_call(s, "sf_observe", kNotVoid); if (rc) return rc; }
    const int oh = eh / f, ow = ew / f;
    const ObsTile tl = obs_tile(f, ow);
    const long long tiles_x = (ow + tl.TX - 1) / tl.TX, tiles = tiles_x * ((oh + tl.TY - 1) / tl.TY);
    if ((long long)n * tiles > 0x7FFFFFFFLL) return fail(SF_ENOTSUP, "sf_observe: %d environments x %lld tiles exceed the launch grid", n, tiles);

    // the per-call block: ObsHead | envs [n] | centers [n][2] (host) | agents [n][k][3] (host)
    const size_t o_envs = (sizeof(ObsHead) + 15) / 16 * 16, o_cen = o_envs + ((size_t)n * 4 + 15) / 16 * 16;
    const bool cen_host = crop && !p->centers_device, ag_host = k > 0 && !p->agents_device;
    const size_t o_ag = o_cen + (cen_host ? ((size_t)n * 8 + 15) / 16 * 16 : 0);
    const size_t bytes = o_ag + (ag_host ? (size_t)n * k * 12 : 0);
    CallBlock &blk = s->obs_blk;
    { int rc = block_reserve(s, blk, bytes); if (rc) return rc; }
    ObsHead h;
    memset(&h, 0, sizeof h);
    for (int c = 0; c < C; ++c) { h.code[c] = p->channels[c]; h.mode[c] = p->pool_mode[c]; }
    // get_attribute_bounds (simulation.py:334-374; FuelConstants / ElevationConstants / WindConstants, enums.py:118-173) in the order of
    // supported_attributes (simulation.py:317-332)
    const double lo[7] = {0.0, 1.0, 0.2, 0.12, -282.0, 0.0, 0.0}, hi[7] = {1.0, 3500.0, 6.0, 1.0, 11000.0, 250.0, 360.0};
    for (int a = 0; a < 7; ++a) { h.lo[a] = lo[a]; h.span[a] = hi[a] - lo[a]; }
    memcpy(blk.pinned, &h, sizeof h);
    memcpy(blk.pinned + o_envs, envs, (size_t)n * 4);
    if (cen_host) memcpy(blk.pinned + o_cen, p->centers, (size_t)n * 8);
    if (ag_host) memcpy(blk.pinned + o_ag, p->agents, (size_t)n * k * 12);
    { int rc = block_send(s, blk, bytes); if (rc) return rc; }

    ObsArgs a;
    memset(&a, 0, sizeof a);
    a.g = g;
    a.status = s->status;
    a.cells = s->bl_cur ? s->cells : nullptr;
    a.lay = s->lay_all;
    a.lay_tab = s->rt_set.size() > 1 ? 7LL * g.H * g.W : 0;
    a.head = reinterpret_cast<const ObsHead *>(blk.dev);
    a.envs = reinterpret_cast<const int32_t *>(blk.dev + o_envs);
    a.centers = !crop ? nullptr : (cen_host ? reinterpret_cast<const int32_t *>(blk.dev + o_cen) : p->centers);
    a.agents = k == 0 ? nullptr : (ag_host ? reinterpret_cast<const int32_t *>(blk.dev + o_ag) : p->agents);
    a.out = device_out;
    a.n = n; a.C = C; a.f = f; a.ch = eh; a.cw = ew; a.oh = oh; a.ow = ow; a.k = k;
    a.TX = tl.TX; a.TY = tl.TY; a.tiles_x = (int)tiles_x; a.stride = tl.stride;
    a.norm = p->normalize != 0; a.bf16 = p->dtype == 1; a.pad = p->pad;
    hipLaunchKernelGGL(k_observe, dim3((unsigned)((long long)n * tiles)), dim3(kObsThreads), 0, s->stream, a);
    return finish_call(s, "sf_observe", !s->async, nullptr);
}

// ----------------------------------------------------------------------------- frames
// Output rows per k_render workgroup and its LDS bytes: the staged source rows (R * scale rows of P bytes) and the output bytes of the
// band (channels last: one segment of R * ow * 3 bytes, else three of R * ow), each segment with 16 bytes of alignment slack.
struct RenderTile { int R, st_bytes, out_seg, lds; };
static RenderTile render_tile(const Geo &g, int scale, int oh, int ow, bool cl)
{
    constexpr int kBudget = 32768, kMax = 65536 - 256;
    const auto make = [&](int R) {
        RenderTile t;
        t.R = R;
        t.st_bytes = (R * scale * g.P + 15) / 16 * 16;
        t.out_seg = cl ? (R * ow * 3 + 16 + 15) / 16 * 16 : (R * ow + 16 + 15) / 16 * 16;
        t.lds = t.st_bytes + (cl ? 1 : 3) * t.out_seg;
        return t;
    };
    int R = 1;
    while (R < oh && make(R + 1).lds <= kBudget) ++R;
    RenderTile t = make(R);
    if (t.lds > kMax) t.R = 0;
    return t;
}

extern "C" int sf_render(sf_sim *s, const sf_render_params *p, int32_t n, const int32_t *envs, void *device_out)
{
    if (!s || !p) return fail(SF_EINVAL, "sf_render: null argument");
    const Geo &g = s->g;
    if (n < 0 || (n > 0 && (!envs || !device_out))) return fail(SF_EINVAL, "sf_render: bad environment list or output");
    if (p->source != SF_RENDER_CURRENT && p->source != SF_RENDER_HISTORY)
        return fail(SF_EINVAL, "sf_render: source %d (0 current, 1 history)", p->source);
    const bool hist = p->source == SF_RENDER_HISTORY;
    if (hist && (p->first < 0 || p->count < 1)) return fail(SF_EINVAL, "sf_render: history frames %d from %d", p->count, p->first);
    if (p->scale < 1 || p->scale > SF_RENDER_MAX_SCALE) return fail(SF_EINVAL, "sf_render: scale %d (1..%d)", p->scale, SF_RENDER_MAX_SCALE);
    if (p->mode < SF_RENDER_NEAREST || p->mode > SF_RENDER_SPRITES) return fail(SF_EINVAL, "sf_render: mode %d (0 nearest, 1 mean, 2 sprites)", p->mode);
    if (p->background != SF_RENDER_FUEL && p->background != SF_RENDER_WHITE)
        return fail(SF_EINVAL, "sf_render: background %d (0 fuel, 1 white)", p->background);
    if (p->contours != 0 && p->contours != 1) return fail(SF_EINVAL, "sf_render: contours %d (0 or 1)", p->contours);
    if (p->channels_last != 0 && p->channels_last != 1) return fail(SF_EINVAL, "sf_render: channels_last %d (0 or 1)", p->channels_last);
    for (int c = 0; c < 3; ++c)
        if (p->terrain_rgb[c] < 0 || p->terrain_rgb[c] > 255) return fail(SF_EINVAL, "sf_render: terrain_rgb[%d] = %d (0..255)", c, p->terrain_rgb[c]);
    const int k = p->agents ? p->agents_k : 0;
    if (p->agents && (p->agents_k < 0 || p->agents_k > SF_RENDER_MAX_AGENTS))
        return fail(SF_EINVAL, "sf_render: %d agents per environment (0..%d)", p->agents_k, SF_RENDER_MAX_AGENTS);
    { int rc = check_envs(s, "sf_render", n, envs); if (rc) return rc; }
    const int s_ = p->scale, oh = (g.H + s_ - 1) / s_, ow = (g.W + s_ - 1) / s_;
    const bool cl = p->channels_last != 0;
    const RenderTile tl = render_tile(g, s_, oh, ow, cl);
    if (tl.R == 0) return fail(SF_ENOTSUP, "sf_render: a row of %d cells does not fit one workgroup's LDS", g.W);
    const int count = hist ? p->count : 1;
    const long long frames = (long long)n * count, bands = (oh + tl.R - 1) / tl.R;
    if (frames * bands > 0x7FFFFFFFLL) return fail(SF_ENOTSUP, "sf_render: %lld frames x %lld bands exceed the launch grid", frames, bands);
    if (hist && !s->history) return fail(SF_ESTATE, "sf_render: a history source needs sf_enable_history");
    if (hist && p->count > s->history_cap)
        return fail(SF_EINVAL, "sf_render: %d updates do not fit the history capacity %d", p->count, s->history_cap);
    const int n_tab = (int)s->rt_set.size();
    for (int i = 0; i < n; ++i)
        if (!s->rd_lay[n_tab == 1 ? 0 : envs[i]]) return fail(SF_ESTATE, "sf_render: environment %d has no layers (sf_set_layers)", envs[i]);
    if (n == 0) return SF_OK;
    { int rc = begin_call(s, "sf_render", kNotVoid); if (rc) return rc; }

    // which backgrounds to (re)build: the listed environments' stale tables; every functional one when the fuel colours were made
    // from another terrain_rgb (only the fuel background shows them)
    const int64_t rgb = p->terrain_rgb[0] | p->terrain_rgb[1] << 8 | p->terrain_rgb[2] << 16;
    if (p->background == SF_RENDER_FUEL && rgb != s->rd_rgb) {
        for (int t = 0; t < n_tab; ++t) if (!s->rd_fbfm[t]) s->rd_stale[t] = 1;
        s->rd_rgb = rgb;
    }
    std::vector<int32_t> tabs, fb;
    {
        std::vector<char> want(n_tab, 0);
        for (int i = 0; i < n; ++i) want[n_tab == 1 ? 0 : envs[i]] = 1;
        for (int t = 0; t < n_tab; ++t)
            if (want[t] && s->rd_stale[t]) { tabs.push_back(t); fb.push_back(s->rd_fbfm[t]); }
    }
    if (!s->rd_bg) HIPCHK(hipMalloc(reinterpret_cast<void **>(&s->rd_bg), (size_t)n_tab * g.H * g.W * sizeof(uint32_t)));

    // the per-call block: envs [n] | tabs [nt] | fbfm [nt] | min / max [nt][2] | agents [n][k][3] (host)
    const int nt = (int)tabs.size();
    const auto up16 = [](size_t b) { return (b + 15) / 16 * 16; };
    const bool ag_host = k > 0 && !p->agents_device;
    const size_t o_tabs = up16((size_t)n * 4), o_fb = o_tabs + up16((size_t)nt * 4), o_mm = o_fb + up16((size_t)nt * 4);
    const size_t o_ag = o_mm + (size_t)nt * 16, bytes = o_ag + (ag_host ? (size_t)n * k * 12 : 0);
    CallBlock &blk = s->rd_blk;
    { int rc = block_reserve(s, blk, bytes); if (rc) return rc; }
    memcpy(blk.pinned, envs, (size_t)n * 4);
    if (nt) { memcpy(blk.pinned + o_tabs, tabs.data(), (size_t)nt * 4); memcpy(blk.pinned + o_fb, fb.data(), (size_t)nt * 4); }
    if (ag_host) memcpy(blk.pinned + o_ag, p->agents, (size_t)n * k * 12);
    // (the lists, and the agents behind the min / max words: those are the kernels' to write)
    { int rc = block_send(s, blk, o_mm, o_ag, ag_host ? (size_t)n * k * 12 : 0); if (rc) return rc; }

    if (nt) {
        RenderBgArgs b;
        memset(&b, 0, sizeof b);
        b.H = g.H; b.W = g.W;
        b.lay = s->lay_all; b.lay_tab = 7LL * g.H * g.W;
        b.fuel_ix = s->rd_fuel_ix;
        b.tabs = reinterpret_cast<const int32_t *>(blk.dev + o_tabs);
        b.fbfm = reinterpret_cast<const int32_t *>(blk.dev + o_fb);
        b.mm = reinterpret_cast<double *>(blk.dev + o_mm);
        b.bg = s->rd_bg;
        b.base = (uint32_t)(s->rd_rgb < 0 ? rgb : s->rd_rgb);
        for (int c = 0; c < kRdFbfmColours; ++c) {
            uint32_t w = 0;
            for (int ch = 0; ch < 3; ++ch) w |= (uint32_t)(uint8_t)(kRdFbfmRgb[c][ch] * 255.0) << (8 * ch);     // astype(np.uint8)
            b.fbfm_rgb[c] = w;
        }
        hipLaunchKernelGGL(k_render_minmax, dim3((unsigned)nt), dim3(1024), 0, s->stream, b);
        hipLaunchKernelGGL(k_render_bg, dim3((unsigned)g.H, (unsigned)nt), dim3(kRdThreads), 0, s->stream, b);
        HIPCHK(hipGetLastError());
        for (int t : tabs) s->rd_stale[t] = 0;
    }

    RenderArgs a;
    memset(&a, 0, sizeof a);
    a.g = g;
    a.status = s->status;
    a.cells = !hist && s->bl_cur ? s->cells : nullptr;
    a.hist = hist ? s->history : nullptr;
    a.cap = s->history_cap; a.first = hist ? p->first : 0; a.count = count;
    a.bg = s->rd_bg;
    a.bg_tab = n_tab > 1 ? (long long)g.H * g.W : 0;
    a.envs = reinterpret_cast<const int32_t *>(blk.dev);
    a.agents = k == 0 ? nullptr : (ag_host ? reinterpret_cast<const int32_t *>(blk.dev + o_ag) : p->agents);
    a.out = static_cast<uint8_t *>(device_out);
    a.n_frames = (int)frames; a.k = k;
    a.s = s_; a.mode = p->mode; a.white = p->background == SF_RENDER_WHITE; a.contours = p->contours; a.cl = cl;
    a.oh = oh; a.ow = ow; a.R = tl.R; a.stride = g.P; a.st_bytes = tl.st_bytes; a.out_seg = tl.out_seg;
    hipLaunchKernelGGL(k_render, dim3((unsigned)(frames * bands)), dim3(kRdThreads), (unsigned)tl.lds, s->stream, a);
    return finish_call(s, "sf_render", !s->async, nullptr);
}

extern "C" int sf_compute_ros(int64_t n, const float *loc_x, const float *loc_y, const float *new_loc_x,
                              const float *new_loc_y, const float *w_0, const float *delta, const float *M_x,
                              const float *sigma, const float *h, const float *S_T, const float *S_e,
                              const float *p_p, const float *M_f, const float *U, const float *U_dir,
                              const float *slope_mag, const float *slope_dir, double *R_out, int32_t device)
{
    const float *in[17] = {loc_x, loc_y, new_loc_x, new_loc_y, w_0, delta, M_x, sigma, h, S_T, S_e, p_p, M_f, U, U_dir,
                           slope_mag, slope_dir};
    if (n < 0) return fail(SF_EINVAL, "sf_compute_ros: n must be >= 0");
    if (n == 0) return SF_OK;
    for (int i = 0; i < 17; ++i) if (!in[i]) return fail(SF_EINVAL, "sf_compute_ros: null input #%d", i);
    if (!R_out) return fail(SF_EINVAL, "sf_compute_ros: null output");
    HIPCHK(hipSetDevice(device));
    float *d_in = nullptr;
    double *d_out = nullptr;
    HIPCHK(hipMalloc(reinterpret_cast<void **>(&d_in), (size_t)17 * n * sizeof(float)));
    if (hipMalloc(reinterpret_cast<void **>(&d_out), (size_t)n * sizeof(double)) != hipSuccess) {
        hipFree(d_in);
        return fail(SF_EHIP, "sf_compute_ros: out of device memory");
    }
    int rc = SF_OK;
    for (int i = 0; i < 17 && rc == SF_OK; ++i)
        if (hipMemcpy(d_in + (size_t)i * n, in[i], (size_t)n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
            rc = fail(SF_EHIP, "sf_compute_ros: upload failed");
    if (rc == SF_OK) {
        const float *p = d_in;
        hipLaunchKernelGGL(k_compute_ros, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, (long long)n, p, p + n,
                           p + 2 * n, p + 3 * n, p + 4 * n, p + 5 * n, p + 6 * n, p + 7 * n, p + 8 * n, p + 9 * n,
                           p + 10 * n, p + 11 * n, p + 12 * n, p + 13 * n, p + 14 * n, p + 15 * n, p + 16 * n, d_out);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess)
            rc = fail(SF_EHIP, "sf_compute_ros: kernel failed");
        else if (hipMemcpy(R_out, d_out, (size_t)n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
            rc = fail(SF_EHIP, "sf_compute_ros: download failed");
    }
    hipFree(d_in);
    hipFree(d_out);
    return rc;
}
