// The handle (struct sf_sim), grouped by feature, and what every call starts and ends with.  Part of the single translation unit
// simfire_hip.hip (included there behind the kernel headers, in front of the host code: sf_host_*.h and the rest of simfire_hip.hip).
//
// Who owns device memory also frees it: each feature's state has ONE release() that frees its allocations and nulls the pointers.
// destroy() calls them all; a feature's early-free path (agents_free, episodes_free, value_free, sf_set_wind_lab) calls the same
// one and then makes its own adjustment of `bytes`.
#pragma once
#include "sf_tables.h"
#include "sf_planes.h"

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
// a call that returns SF_OK or a code whose message is already set: on a code, return it
#define SF_TRY(expr) do { const int _rc = (expr); if (_rc) return _rc; } while (0)

// hipFree / hipHostFree of a pointer that may be null, which is null afterwards (release() of the feature states)
template <typename T>
static hipError_t free_dev(T *&p)
{
    const hipError_t e = p ? hipFree(p) : hipSuccess;
    p = nullptr;
    return e;
}
template <typename T>
static hipError_t free_pinned(T *&p)
{
    const hipError_t e = p ? hipHostFree(p) : hipSuccess;
    p = nullptr;
    return e;
}
// the first error of several frees (all of them are made)
static hipError_t first_error(std::initializer_list<hipError_t> es)
{
    for (hipError_t e : es) if (e != hipSuccess) return e;
    return hipSuccess;
}

namespace {      // (the types the handle is made of: internal linkage, like the kernel arguments of sf_common.h)

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
    void release()
    {
        (void)free_dev(dev); (void)free_pinned(pinned);
        if (ev) (void)hipEventDestroy(ev);
        ev = nullptr; cap = 0;
    }
};

// The lab's timing of a feature's launches (sf_time_resets, sf_set_wind_lab): while `on`, ev0 / ev1 of the handle are recorded around
// them (lab_start / lab_stop); `have`: a pair has been recorded since the switch (lab_ms)
struct LabTimer { bool on = false, have = false; };

// k_run<TEAM>: an environment served by several workgroups (sf_run_kernels.h); allocated at the first team launch
struct TeamState {
    uint32_t *tab = nullptr, *size = nullptr, *xdone = nullptr;
    uint32_t *xj = nullptr;            // k_run<TEAM = 2> (teams that grow inside the launch): names put down / the board / counters (StepArgs::xj)
    unsigned long long *xcut = nullptr;
    uint32_t *jlog = nullptr;          // what happened to the teams in the last such launch (sf_get_join_log)
    bool jlog_valid = false;
    unsigned long long *xg = nullptr;
    uint8_t *xbuf = nullptr;
    uint32_t *xerr_pinned = nullptr, *xerr_mapped = nullptr;
    int slots = 0;                     // entries of tab
    long long plan_ones = 0;           // != 0: tab / size hold the plan "every environment one workgroup" for this (E, slots, placement) - k_team_plan need not run again for it
    hipError_t release()
    {
        xerr_mapped = nullptr;
        return first_error({free_pinned(xerr_pinned), free_dev(tab), free_dev(size), free_dev(xdone), free_dev(xg), free_dev(xbuf), free_dev(xj),
                            free_dev(xcut), free_dev(jlog)});
    }
};

// LOOP mode (sf_loop_start): the resident launch driven step by step through host-mapped memory
struct LoopState {
    bool on = false;
    int light = 0;                     // 1: the running closed loop is the light one (8-wave workgroups; SF_TUNE_LOOP_LIGHT)
    int k = 0;                         // points per environment and step
    uint32_t seq = 0;                  // sequence number of the last step posted
    uint32_t *db = nullptr, *db_dev = nullptr;         // (pinned, device-mapped) [0] doorbell, [64 ...] "done" numbers [E] (other cache lines)
    int32_t *res = nullptr, *res_dev = nullptr;        // u32 [E][16]: one 64-byte line per environment (pinned, device-mapped; k_run, loop_finish)
    int32_t *pts = nullptr, *pts_dev = nullptr;        // [2][slot] points ring (pinned, device-mapped)
    size_t pts_cap = 0, slot_ints = 0;
    uint32_t *mem = nullptr;                           // device: [0] forwarded sequence number, [32 ...] done [E]
    int32_t *pts_mem = nullptr;                        // device copy of the ring
    size_t pts_mem_cap = 0;
    int restarts = 0;                  // times the launch had left by itself (timeout) and was started again
    hipError_t release()
    {
        db_dev = nullptr; res_dev = pts_dev = nullptr;
        return first_error({free_pinned(db), free_pinned(res), free_pinned(pts), free_dev(mem), free_dev(pts_mem)});
    }
};

// sf_get_fire_map_delta: the fire maps as the host last saw them (u8 [E][H][P], allocated at the first call), per environment whether that
// reference point exists, the list of changed cells on the device ([0] = count) and its pinned landing zone
struct DeltaState {
    uint8_t *snap = nullptr;
    std::vector<char> snap_valid;
    uint32_t *dev = nullptr, *pinned = nullptr;
    int cap = 0;
    uint32_t base = 0;                 // what the list's count stood at after the last query (it counts on: nothing zeroes it)
    hipError_t release() { return first_error({free_dev(snap), free_dev(dev), free_pinned(pinned)}); }
};

// sf_enable_arrival: the plane u32 [E][H][P] (update that created a cell's first sprite + 1, 0 = never; null =
// recording off), updates made since the last pass (< md between the pieces of a call, 0 between calls), the lab's "always the
// dense pass" and its count of passes made in the sparse / the dense form
struct ArrivalState {
    uint32_t *plane = nullptr;
    int pending = 0;
    bool dense = false;
    int64_t passes[2] = {0, 0};
    hipError_t release() { return free_dev(plane); }
};

// sf_values_set: the handle's copy of the value plane, int32 [n][H][P] with n = E (per_env) or 1 and zeros
// in the pitch padding (null = the feature is off); ONE allocation for the records ValueRec [E], tick_base and tick_loss int64 [E]
// and the word the range check of a device plane leaves (sf_sim::val_rec / val_tick / val_bad); the lab's "always the dense pass" and
// its count of passes made in the sparse / the dense form; the fifth reward weight of sf_agents_step
struct ValueState {
    int32_t *plane = nullptr;
    bool per_env = false;
    uint8_t *aux = nullptr;
    bool dense = false;
    int64_t passes[2] = {0, 0};
    float w = 0.0f;
    bool w_on = false;
    hipError_t release() { return first_error({free_dev(plane), free_dev(aux)}); }
};

// sf_render (per table, layers present / FBFM-coded fuel / background stale: TableBook): the background words [tables][H * W], the FBFM
// colour index plane [tables][H * W] (allocated by the first sf_set_layers_fbfm), the terrain_rgb the fuel colours were made from
// (-1: none yet) and the per-call block (lists of environments and tables, the min / max words its kernels write, host agents)
struct RenderState {
    uint32_t *bg = nullptr;
    uint8_t *fuel_ix = nullptr;
    int64_t rgb = -1;
    CallBlock blk;
    hipError_t release() { return first_error({free_dev(bg), free_dev(fuel_ix)}); }
};

// wind changes: the cache plane of wind-independent terms, float [tables][kWindPlanes][H * W], allocated at the
// first wind change (per table whether its part is stale: TableBook; cache_off: the lab has switched the cache off); the
// schedules on the device [E] with their host mirror (segments per environment, the scheduled environments, whether the cache has been
// made current for them since the last change of either: TableBook::wind_sched_ready), the due list of a schedule pass and its winds;
// the call block (list, scalars, schedule rows); the lab's events around the launches
struct WindState {
    float *terms = nullptr;
    bool cache_off = false;
    WindSched *sched_dev = nullptr;
    std::vector<int32_t> K, sched;
    bool sched_cached = false;
    int32_t *due = nullptr;
    uint32_t *due_cnt = nullptr;       // (inside `due`)
    double *due_U = nullptr, *due_D = nullptr;      // (due_D: inside due_U)
    CallBlock blk;
    LabTimer timer;
    hipError_t release_cache() { return free_dev(terms); }
    hipError_t release()
    {
        due_cnt = nullptr; due_D = nullptr;
        return first_error({release_cache(), free_dev(sched_dev), free_dev(due), free_dev(due_U)});
    }
};

// sf_agents_* (DESIGN.md section 16): the parameters of sf_agents_create (p.k == 0: no agent state), ONE device allocation that
// holds every agent buffer - positions, start cells, this tick's points, the counts and episode statistics between the two
// kernels of a tick, the done mask, the ignitions of a new episode - and the call block of sf_agents_place.  Not slices of
// env_segs: fork, snapshot and restore do not carry agents.
struct AgentState {
    sf_agent_params p = {};
    uint8_t *mem = nullptr;
    size_t bytes = 0;
    int32_t *xyid = nullptr, *start = nullptr, *points = nullptr, *prev = nullptr, *terms = nullptr, *len = nullptr, *ign = nullptr;
    double *ret = nullptr;
    uint8_t *done = nullptr;
    CallBlock blk;
    bool has_ign = false;              // sf_agents_create was given ignitions
    hipError_t release()
    {
        xyid = start = points = prev = terms = len = ign = nullptr;
        ret = nullptr; done = nullptr;
        bytes = 0;
        return free_dev(mem);
    }
};

// sf_episodes_* (DESIGN.md section 19): the parameters of sf_episodes_set (on: randomisation is set) and ONE device allocation
// for the episode buffers - the next episode's index, the ignition a new episode takes (drawn, or the fixed one), the last wind
// drawn, the due list k_episode_draw leaves for k_wind_rtable (the list, its count, the winds) and a mask of ones (all = 1).
// The handle's like the agent buffers: not slices of env_segs.
// nocache: the cache of wind-independent terms could not be had (no memory, or the lab has it off): not asked for again
// until sf_episodes_set / sf_set_wind_lab.
struct EpisodeState {
    sf_episode_params p = {};
    bool on = false, nocache = false;
    uint8_t *mem = nullptr, *ones = nullptr;
    size_t bytes = 0;
    uint32_t *index = nullptr, *due_cnt = nullptr;
    int32_t *ign = nullptr, *due = nullptr;
    double *wind = nullptr, *due_U = nullptr, *due_D = nullptr;
    hipError_t release()
    {
        ones = nullptr; bytes = 0;
        index = due_cnt = nullptr;
        ign = due = nullptr;
        wind = due_U = due_D = nullptr;
        return free_dev(mem);
    }
};

// A query with scratch (sf_host_query.h; DESIGN.md section 22, "host frame of a query"): the scratch of the environments a call is
// working on - allocated at the first call, grown but never shrunk when a call's chunk needs more (scratch_reserve), freed with the
// handle -, its size in bytes, and the call block (the environment list of a call).  What lies in it, per listed environment of a
// chunk: sf_distance the plane g, u16 [H][P]; sf_reach two bit planes and the halo (reach_env_bytes); sf_walk three bit planes and
// two halos (walk_env_bytes); sf_escape those, the sorted cells and the buckets (escape_env_bytes); sf_travel the working array, float32 [H][W] dense (travel_env_bytes) - only when the call asks for no
// minutes plane, which is the working array otherwise; sf_perimeter the bit plane, the edge words and eight arrays of max_edges
// (perim_env_bytes) - only when the call asks for a traced output; sf_influence the parent codes, the child counters and the
// accumulators that are no output of the call (infl_env_bytes); sf_components the selected bits, the rows' root counts, the second plane
// and - unless the labels output is the label plane - the label plane (cc_env_bytes).
struct QueryState {
    uint8_t *mem = nullptr;
    size_t cap = 0;
    CallBlock blk;
    hipError_t release() { cap = 0; return free_dev(mem); }
};

// sf_behavior: the heat cache, float [tables][H * W] (per table whether its part is stale: TableBook) -
// allocated at the first call, freed with the handle -, the parts built so far (the lab's count) and the call block (the
// environment list of a call)
struct BehaviorState {
    float *hpa = nullptr;
    int64_t builds = 0;
    CallBlock blk;
    hipError_t release() { return free_dev(hpa); }
};

}  // namespace

// ----------------------------------------------------------------------------- handle
// The step path's buffers and knobs stand flat in the handle; which cell layout is current and which structures derived from it still
// match it - the step path's coherence state - is the PlaneBook's (planes, sf_planes.h), as the per-table flags are the TableBook's.
struct sf_sim {
    sf_params p;
    Geo g;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    uint8_t *status = nullptr, *age_alloc = nullptr, *age = nullptr;
    uint8_t *cells_alloc = nullptr, *cells = nullptr;      // blocked cell plane of the resident launch (allocated at its first use)
    double *burn = nullptr, *rt = nullptr;
    mutable std::map<std::tuple<const void *, unsigned, size_t>, int> occ_cache;      // k_run instantiations: workgroups per CU by hipOccupancyMaxActiveBlocksPerMultiprocessor (occupancy)
    double *rtc = nullptr;             // the R table(s) cell-major (k_rt_cellmajor): built when the resident launch first needs it, stale after every change of rt (TableBook)
    unsigned long long *win_hint = nullptr;      // k_run's window phase: where the fire stood and where the window was when the phase last ended, per environment; 0 = unknown.  ADVICE only (sf_win_kernels.h)
    double *lay_all = nullptr;         // [tables][7][H*W] dense: w0 delta Mx sigma elev U Udir (kept for the observation planes)
    double *layer(int table, int i) const { return lay_all + ((size_t)table * 7 + i) * (size_t)g.H * g.W; }
    TableBook tables;                  // per terrain table: what has been supplied, what is stale (sf_tables.h)
    PlaneBook planes;                  // which cell layout is current, what derived from it still matches it (sf_planes.h)
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
    int32_t *sink = nullptr;           // sf_set_result_sink: caller-owned device copy of the result block, written by every refresh
    int last_launches = 0;             // k_run launches of the last step call (sf_get_last_launches)
    // run(1) loops (one update per call, the result block looked at after each - FireSimulation.run(1) in a harness): after two such
    // pairs in a row the single update runs as the resident launch too, which leaves the block behind itself (measured, step(1) +
    // status() per call: 41 against 46 us on one environment, 47 against 58 on C3's 256; a loop that only enqueues step(1) calls, or
    // looks at the maps after each, is faster on the per-step kernels and keeps them)
    bool last_was_step1 = false;       // the last step call was one update and nothing has looked at its result yet
    int step1_polls = 0;               // step(1) + status pairs in a row
    unsigned long long *vbits = nullptr;   // vector bitmap of the resident launch (k_run)
    int32_t *todo = nullptr;           // team launches with windows of rows: the steps an environment's team could not make (the catch-up launch's) [E]
    ncclComm_t comm = nullptr;         // sf_comm_init: communicator of the result-block all-gather
    int comm_world = 0;
    int last_team_max = 0;             // upper bound of the team sizes in the last resident launch (0: it was not a team launch)
    int cost_steps = 0;                // steps the per-environment cost array covers (0: nothing recorded since the last reset)
    uint32_t *todo_cnt = nullptr;      // k_win: how many environments it left updates for (their numbers: run_order); two counts, by the parity of win_seq
    unsigned win_seq = 0;              // k_win launches so far
    uint32_t *run_cost = nullptr, *run_order = nullptr;   // k_run: clocks / 16 an environment's workgroup took in the last resident launch [E]; launch order built from it (k_order)
    mutable std::map<const void *, size_t> lds_allowed;       // dynamic LDS the resident kernels have been enabled for, by host handle (allow_lds)
    uint8_t *parents = nullptr;        // spread-graph parent masks, allocated by sf_enable_spread_graph
    bool graph_on = false;
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
    bool counters_on = false;
    int seq = 0;                       // index (mod 6) of the next step launch
    Tuning tune;                       // sf_set_tuning
    int64_t bytes = 0;
    std::vector<int32_t> last_ign;     // the ignitions of the last sf_reset (host copy; sf_episodes_set)
    // the features, each with its own state
    TeamState team;
    LoopState loop;
    DeltaState delta;
    ArrivalState arrival;
    ValueState values;
    RenderState render;
    WindState wind;
    AgentState agents;
    EpisodeState episodes;
    QueryState dist, reach, walk, escape, travel, perimeter, influence, components;      // one block and one scratch per feature (as for CallBlock: calls of different features do not wait for each other)
    BehaviorState behavior;
    CallBlock obs_blk;                 // sf_observe: ObsHead, environment list, host centers / agents
    CallBlock rs_blk;                  // sf_reset_envs / sf_reset_where: the environment list and host ignitions of a call
    LabTimer reset_timer;              // sf_time_resets: ev0 / ev1 recorded around the launches of every batched reset
    LabTimer components_timer;         // sf_time_components: the same around the memsets and launches of every sf_components
    LabTimer ignite_timer;             // sf_time_ignites: the same around the scatter launch of every sf_ignite / sf_ignite_device
    CallBlock gen_blk;                 // sf_generate_layers: its descriptors + environment list
    CallBlock ens_blk;                 // sf_ensemble_stats: the member list of a call
    size_t val_plane_bytes() const { return (size_t)(values.per_env ? g.E : 1) * g.plane_env * sizeof(int32_t); }
    size_t val_aux_bytes() const { return (size_t)g.E * (sizeof(ValueRec) + 16) + 16; }
    ValueRec *val_rec() const { return reinterpret_cast<ValueRec *>(values.aux); }
    long long *val_tick(int i) const { return reinterpret_cast<long long *>(values.aux + (size_t)g.E * (sizeof(ValueRec) + 8 * i)); }      // 0: base, 1: loss
    uint32_t *val_bad() const { return reinterpret_cast<uint32_t *>(values.aux + (size_t)g.E * (sizeof(ValueRec) + 16)); }
};

// the blocked plane if it is the current one, else null: what a kernel that reads whichever layout is current takes as `cells`
static uint8_t *cur_cells(const sf_sim *s) { return s->planes.blocked() ? s->cells : nullptr; }
// the status bytes as the kernels off the step path take them (sf_cells.h): to read, and to write
static CellPlanes cur_planes(const sf_sim *s) { return CellPlanes{s->status, cur_cells(s)}; }
static CellPlanesMut cur_planes_mut(const sf_sim *s) { return CellPlanesMut{s->status, cur_cells(s)}; }
// In front of a launch that looks after the per-tile histograms: while every one is stale, say so on the device.
static int mark_hist_dirty(sf_sim *s)
{
    if (s->planes.hist_all_stale()) HIPCHK(hipMemsetAsync(s->tdirty, 1, s->n_tiles_max, s->stream));
    s->planes.hist_marked();
    return SF_OK;
}

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
#define LOOP_QUIESCE(s) do { if ((s)->loop.on) { int _rq = loop_stop(s); if (_rq) return _rq; } } while (0)
static int ensure_rm(sf_sim *s);
static int value_pass(sf_sim *s);
static int wind_forget(sf_sim *s, const int32_t *envs, int n);
static hipError_t allow_lds(const sf_sim *s, const void *fn, size_t lds);

// Behind every wait for the handle's stream: has a workgroup of a team launch (k_run<TEAM>) given up waiting for a team member?
// Then what the launch left behind is void - say so wherever data is handed back, not only in sf_sync / a synchronous sf_step.
// (A reset of every environment rewrites all the state a team launch touches and clears the word: the handle recovers.)
static int check_team_error(const sf_sim *s, const char *where)
{
    if (s->team.xerr_pinned && *s->team.xerr_pinned)
        return fail(SF_EHIP, "%s: a workgroup of a team launch (k_run<TEAM>) gave up waiting for a team member; the state of this handle is void until every environment is reset", where);
    return SF_OK;
}

// The prologue of a call (call layer): what the handle must have been given (SF_ESTATE before anything else happens), the device, the
// end of a closed loop, then - where asked for - the refusal of a handle a failed team launch has voided and the step rings folded
// into commit[] (after which tmp / flags carry nothing: the next launch starts from commit).
enum { kNeedRt = 1, kNeedReset = 2, kNotVoid = 4, kCommit = 8, kStateCall = kNeedReset | kNotVoid | kCommit };
static int check_ready(const sf_sim *s, const char *who, int need)
{
    if ((need & kNeedRt) && !s->tables.have_rt()) return fail(SF_ESTATE, "%s: call sf_set_layers or sf_set_rtable first", who);
    if ((need & kNeedReset) && !s->planes.was_reset()) return fail(SF_ESTATE, "%s: call sf_reset first", who);
    return SF_OK;
}
static int begin_call(sf_sim *s, const char *who, int need)
{
    SF_TRY(check_ready(s, who, need));
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    if (need & kNotVoid) SF_TRY(check_team_error(s, who));
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
    b.cap = 0;
    HIPCHK(free_dev(b.dev));
    HIPCHK(free_pinned(b.pinned));
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
// A whole block of up to two host segments (an environment list and what travels with it): the `na` bytes at `a` and, right behind
// them, the `nc` bytes at `c` - room reserved, copied into the mirror, sent.  *dev: where `a` stands on the device (`c`: na bytes on).
template <typename T>
static int block_stage(sf_sim *s, CallBlock &b, const T **dev, const T *a, size_t na, const void *c = nullptr, size_t nc = 0)
{
    SF_TRY(block_reserve(s, b, na + nc));
    if (na) memcpy(b.pinned, a, na);
    if (nc) memcpy(b.pinned + na, c, nc);
    *dev = reinterpret_cast<const T *>(b.dev);
    return block_send(s, b, na + nc);
}

// Room for `bytes` in a query's scratch: grown, never shrunk.  Growing waits for the stream first (enqueued kernels may still use
// the scratch) and is counted in the handle's `bytes`.
static int scratch_reserve(sf_sim *s, QueryState &q, size_t bytes)
{
    if (bytes <= q.cap) return SF_OK;
    HIPCHK(hipStreamSynchronize(s->stream));
    s->bytes -= (int64_t)q.cap;
    HIPCHK(q.release());
    HIPCHK(hipMalloc(reinterpret_cast<void **>(&q.mem), bytes));
    q.cap = bytes;
    s->bytes += (int64_t)q.cap;
    return SF_OK;
}

// The lab's events around a feature's launches (enqueue layer), and what they measured: `why` says what has not happened yet
static int lab_start(sf_sim *s, const LabTimer &t)
{
    if (t.on) HIPCHK(hipEventRecord(s->ev0, s->stream));
    return SF_OK;
}
static int lab_stop(sf_sim *s, LabTimer &t)
{
    if (t.on) { HIPCHK(hipEventRecord(s->ev1, s->stream)); t.have = true; }
    return SF_OK;
}
static int lab_ms(sf_sim *s, const LabTimer &t, const char *who, const char *why, float *ms_out)
{
    if (!t.have) return fail(SF_ESTATE, "%s: %s", who, why);
    HIPCHK(hipSetDevice(s->p.device));
    HIPCHK(hipEventSynchronize(s->ev1));
    HIPCHK(hipEventElapsedTime(ms_out, s->ev0, s->ev1));
    return SF_OK;
}
