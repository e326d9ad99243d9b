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
//     steps, its vector bitmaps live in LDS, the cells in a blocked plane (sf_cells.h); the automatic choice for n >= 2 on
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
#include "sf_dist_kernels.h"
#include "sf_reach_kernels.h"
#include "sf_walk_kernels.h"
#include "sf_escape_kernels.h"
#include "sf_travel_kernels.h"
#include "sf_perimeter_kernels.h"
#include "sf_influence_kernels.h"
#include "sf_components_kernels.h"
#include "sf_behavior_kernels.h"
#include "sf_ignite_kernels.h"

// The host code: the handle and the prologue / epilogue of a call (sf_handle.h), then one fragment per feature (sf_host_*.h, included
// below where their functions stood while this was one file: kernel templates are instantiated in the order the host code names
// them).  This file keeps create / destroy, the setters, the resident launches, the launch plan and the step path, the closed loop,
// status, maps and delta.
#include "sf_handle.h"

extern "C" const char *sf_last_error(void) { return g_err.c_str(); }
// the other translation units report through the same per-thread message (simfire_hip_cfd.hip)
int sf_fail_message(int code, const char *msg)
{
    g_err = msg;
    return code;
}
extern "C" const char *sf_version(void) { return "simfire_hip 0.2 (gfx950)"; }      // 0.2: the knob numbers and the 16 counter slots of simfire_hip_lab.h as they stand since round 5; sf_get_fire_map_delta

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
    s->tables.init(p->per_env_terrain ? g.E : 1);
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
    g.cells_env = bl_env_bytes(g.H, g.PV);
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
    if (s->loop.on) (void)loop_stop(s);
    if (s->stream) hipStreamSynchronize(s->stream);
    (void)comm_close(s);
    // every feature frees what it owns; the step path's own buffers are listed here
    (void)s->team.release(); (void)s->loop.release(); (void)s->delta.release(); (void)s->arrival.release(); (void)s->values.release();
    (void)s->render.release(); (void)s->wind.release(); (void)s->agents.release(); (void)s->episodes.release();
    (void)s->dist.release(); (void)s->reach.release(); (void)s->walk.release(); (void)s->escape.release(); (void)s->travel.release(); (void)s->perimeter.release(); (void)s->influence.release(); (void)s->components.release(); (void)s->behavior.release();
    for (CallBlock *b : {&s->obs_blk, &s->render.blk, &s->rs_blk, &s->gen_blk, &s->agents.blk, &s->wind.blk, &s->ens_blk, &s->dist.blk, &s->reach.blk, &s->walk.blk, &s->escape.blk, &s->travel.blk, &s->perimeter.blk, &s->influence.blk, &s->components.blk, &s->behavior.blk}) b->release();
    void *ptrs[] = {s->status, s->age_alloc, s->cells_alloc, s->burn, s->rt, s->rtc, s->lay_all, s->history, s->smag, s->sdir, s->commit, s->tmp, s->flags, s->counters, s->tflags, s->tile_list, s->n_active, s->seam, s->settled, s->tdirty, s->thist, s->vbits, s->todo, s->run_cost, s->run_order, s->todo_cnt, s->win_hint, s->mit_stage,
                    s->status_block, s->elapsed_dev, s->stage, s->parents};
    for (void *p : ptrs) if (p) hipFree(p);
    if (s->status_pinned) (void)hipHostFree(s->status_pinned);
    for (int i = 0; i < sf_sim::kPtsRing; ++i) {
        if (s->pts_pinned[i]) (void)hipHostFree(s->pts_pinned[i]);
        if (s->ev_pts[i]) (void)hipEventDestroy(s->ev_pts[i]);
    }
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
    s->planes.geometry_changed();      // the tile activity map is laid out per wave tile: rebuilt for the new geometry before the next tiled step
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
    s->planes.family_switched();
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
    if (!s->last_team_max || !s->team.size) { for (int e = 0; e < s->g.E; ++e) out[e] = 0; return SF_OK; }
    HIPCHK(hipMemcpy(out, s->team.size, (size_t)s->g.E * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return SF_OK;
}
extern "C" int sf_get_join_log(sf_sim *s, uint32_t *out, int32_t cap, int32_t *n_out)
{
    if (!s || !n_out || cap < 0 || (cap > 0 && !out)) return fail(SF_EINVAL, "sf_get_join_log: bad argument");
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    HIPCHK(hipStreamSynchronize(s->stream));
    *n_out = 0;
    if (!s->team.jlog || !s->team.jlog_valid) return SF_OK;
    uint32_t n = 0;
    HIPCHK(hipMemcpy(&n, s->team.jlog, sizeof n, hipMemcpyDeviceToHost));
    if (n > (uint32_t)kJoinLog) n = kJoinLog;
    if (n > (uint32_t)cap) n = (uint32_t)cap;
    if (n) HIPCHK(hipMemcpy(out, s->team.jlog + 1, (size_t)n * 3 * sizeof(uint32_t), hipMemcpyDeviceToHost));
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
    if (!s->team.xdone) return SF_OK;                   // (no team launch yet)
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    HIPCHK(hipStreamSynchronize(s->stream));
    uint32_t v = 0;
    HIPCHK(hipMemcpy(&v, s->team.xdone + (size_t)2 * s->g.E, sizeof v, hipMemcpyDeviceToHost));
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

#include "sf_host_terrain.h"

#include "sf_host_wind.h"

// The environment states live in the tmp / flags rings while steps are being enqueued; they are folded
// into commit[] only when something needs them (status queries, resets, burn_amounts transfers).
static int ensure_commit(sf_sim *s)
{
    LOOP_QUIESCE(s);
    if (s->planes.committed()) return SF_OK;
    hipLaunchKernelGGL(k_commit, dim3((s->g.E + 255) / 256), dim3(256), 0, s->stream, s->g, s->commit,
                       (const EnvState *)s->tmp, s->flags, (s->seq + 5) % 6, s->n_active);
    HIPCHK(hipGetLastError());
    s->planes.rings_folded();
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
    if (s->planes.blocked()) add(kSegCells, s->cells_alloc, g.cells_env);
    else {
        add(kSegCells, s->status, g.plane_env);
        add(kSegCells, s->age_alloc, g.age_env * g.ab);      // (with its guard rows)
    }
    add(kSegBurn, s->burn, g.plane_env * 8);
    add(kSegSettled, s->settled, g.plane_env * 4);
    add(kSegParents, s->parents, g.plane_env);
    add(kSegSnap, s->delta.snap, g.plane_env);
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
    const CellPlanesMut pl = cur_planes_mut(s);
    s->planes.points_scattered();
    const dim3 grd((unsigned)((n + 255) / 256)), blk(256);
    hipLaunchKernelGGL(k_mitigate_clear, grd, blk, 0, s->stream, g, pl, (const uint32_t *)s->settled, s->burn,
                       (const EnvState *)s->commit, (const EnvState *)s->tmp, (const uint32_t *)s->flags, s->seq,
                       s->planes.committed() ? 1 : 0, pts_dev, n);
    hipLaunchKernelGGL(k_mitigate_write, grd, blk, 0, s->stream, g, pl, s->settled, s->tdirty,
                       (const EnvState *)s->commit, (const EnvState *)s->tmp, (const uint32_t *)s->flags, s->seq,
                       s->planes.committed() ? 1 : 0, pts_dev, n);
    HIPCHK(hipGetLastError());
    return SF_OK;
}

// n host rows of four int32 -> the next buffer of the pinned, device-mapped ring (sf_apply_mitigation, sf_ignite): *slot names it,
// s->pts_mapped[*slot] is what a kernel reads, and the caller records s->ev_pts[*slot] behind the kernels that do.
static int pts_stage(sf_sim *s, const int32_t *pts, int n, int *slot_out)
{
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
    *slot_out = slot;
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
    int slot = 0;
    SF_TRY(pts_stage(s, pts, n, &slot));
    SF_TRY(scatter_points(s, s->pts_mapped[slot], n));
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
    if (s->delta.snap) s->delta.snap_valid[env] = 0;      // (sf_get_fire_map_delta: no reference point any more)
    SF_TRY(ensure_stage(s, n));
    dim3 blk(256), grd((g.W + 255) / 256, g.H);
    SF_TRY(ensure_commit(s));
    SF_TRY(ensure_rm(s));
    s->planes.map_loaded();            // (from here on the environment's map is being replaced)
    if (g.att)
        hipLaunchKernelGGL(k_settle_env, grd, blk, 0, s->stream, g, (const uint8_t *)s->status, s->settled, s->burn,
                           (const EnvState *)s->commit, env, 1);
    HIPCHK(hipMemcpyAsync(s->stage, map, n, hipMemcpyHostToDevice, s->stream));
    hipLaunchKernelGGL(k_pack_status, grd, blk, 0, s->stream, g, s->status, s->settled, (const EnvState *)s->commit, env,
                       (const uint8_t *)s->stage);
    HIPCHK(hipGetLastError());
    SF_TRY(rebuild_tflags(s, env, 1));
    HIPCHK(hipStreamSynchronize(s->stream));
    return SF_OK;
}

// The resident launch works on the blocked cell plane (sf_cells.h), everything else on the row-major planes; the
// one that is current is converted when the other kind of work comes next (one sweep over the cell planes).
static int ensure_rm(sf_sim *s)
{
    if (!s->planes.blocked()) return SF_OK;
    const Geo &g = s->g;
    hipLaunchKernelGGL(k_bl_to_rm, dim3((g.PV + 63) / 64, g.H, g.E), dim3(64), 0, s->stream, g, (const uint8_t *)s->cells, s->status, s->age);
    HIPCHK(hipGetLastError());
    s->planes.converted_to_rm();
    return SF_OK;
}
static int alloc_bl(sf_sim *s)
{
    if (s->cells_alloc) return SF_OK;
    const Geo &g = s->g;
    const size_t bytes = (size_t)g.E * g.cells_env;
    SF_TRY(dev_alloc(s, &s->cells_alloc, bytes));
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
    if (s->tables.rtc_valid()) return SF_OK;
    const Geo &g = s->g;
    const size_t n_tab = (size_t)s->tables.size(), tab = (size_t)8 * g.plane_env;
    if (!s->rtc) {
        // (the copy doubles the handle's largest allocation with per-environment terrain; the window phase it serves is optional: a handle
        // that cannot have it runs without - the caller switches the phase off for the call, results never depend on it)
        if (hipMalloc(reinterpret_cast<void **>(&s->rtc), tab * n_tab * sizeof(double)) != hipSuccess) { (void)hipGetLastError(); s->rtc = nullptr; return SF_ENOTSUP; }
        s->bytes += (int64_t)(tab * n_tab * sizeof(double));
    }
    for (size_t i = 0; i < n_tab; ++i)
        if (s->tables[i].rtc_stale)
            hipLaunchKernelGGL(k_rt_cellmajor, dim3((g.P + 255) / 256, g.H), dim3(256), 0, s->stream, g.H, g.P, (const double *)(s->rt + i * tab), s->rtc + i * tab);
    HIPCHK(hipGetLastError());
    s->tables.rtc_built();
    return SF_OK;
}

static int ensure_bl(sf_sim *s)
{
    if (s->planes.blocked()) return SF_OK;
    const Geo &g = s->g;
    SF_TRY(alloc_bl(s));
    hipLaunchKernelGGL(k_rm_to_bl, dim3((g.PV + 63) / 64, g.H, g.E), dim3(64), 0, s->stream, g, (const uint8_t *)s->status, (const uint8_t *)s->age, s->cells);
    HIPCHK(hipGetLastError());
    s->planes.converted_to_bl();
    return SF_OK;
}

// The per-step tiled kernels keep the tile activity map and the seam planes, the resident launch keeps the vector
// bitmap; whichever a launch needs is rebuilt from the sprite-mask planes if the other kind ran in between.
static int ensure_tiles(sf_sim *s)
{
    if (s->planes.tiles_valid()) return SF_OK;
    { int rc0 = ensure_rm(s); if (rc0) return rc0; }
    HIPCHK(hipMemsetAsync(s->tflags, 0, s->tflags_bytes, s->stream));
    SF_TRY(rebuild_tflags(s, 0, s->g.E));
    SF_TRY(rebuild_seams(s, 0, s->g.E));
    s->planes.tiles_rebuilt();
    return SF_OK;
}
static int ensure_vbits(sf_sim *s)
{
    if (s->planes.bits_valid()) return SF_OK;
    { int rc0 = ensure_rm(s); if (rc0) return rc0; }
    const Geo &g = s->g;
    hipLaunchKernelGGL(k_rebuild_vbits, dim3(g.VW, g.H, g.E), dim3(64), 0, s->stream, g, (const uint8_t *)s->age, s->vbits, 0);
    HIPCHK(hipGetLastError());
    s->planes.bits_rebuilt();
    return SF_OK;
}

#include "sf_host_views.h"
#include "sf_host_query.h"

extern "C" int sf_last_step_launch(sf_sim *s, int32_t *kind)
{
    if (!s || !kind) return fail(SF_EINVAL, "sf_last_step_launch: null argument");
    *kind = s->planes.last_kind();
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
    case kRunJoin: return {1, att, 1, 0, 2};                      // (one-word rows, diagonal spread, no control lines inside the launch; launch_k_run_join: TEAM = 3 with the counters on)
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
    if (!s->team.tab || s->team.slots < t.slots) {
        if (s->team.tab) { HIPCHK(hipFree(s->team.tab)); s->team.tab = nullptr; }
        SF_TRY(dev_alloc(s, &s->team.tab, (size_t)t.slots));
        s->team.slots = t.slots;
        s->team.plan_ones = 0;
    }
    if (!s->team.xg) {
        SF_TRY(dev_alloc(s, &s->team.xg, (size_t)g.E * kTeamMax * 3));
        SF_TRY(dev_alloc(s, &s->team.xbuf, (size_t)g.E * kTeamMax * 4 * team_xrow(g)));
        SF_TRY(dev_alloc(s, &s->team.xdone, (size_t)2 * g.E + 1));       // members that have left [E] | the teams' start words [E] | teams that started as one
        HIPCHK(hipMemsetAsync(s->team.xdone, 0, sizeof(uint32_t) * ((size_t)2 * g.E + 1), s->stream));
        SF_TRY(dev_alloc(s, &s->team.size, (size_t)g.E));
        HIPCHK(hipHostMalloc(reinterpret_cast<void **>(&s->team.xerr_pinned), sizeof(uint32_t), hipHostMallocMapped));
        HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void **>(&s->team.xerr_mapped), s->team.xerr_pinned, 0));
        *s->team.xerr_pinned = 0;
        HIPCHK(hipMemsetAsync(s->team.xbuf, 0, (size_t)g.E * kTeamMax * 4 * team_xrow(g), s->stream));
    }
    return SF_OK;
}

// The fields of StepArgs every team launch (k_run<TEAM>) sets from the handle.  rcap: bitmap rows a member keeps (0 = all); cost: the cost array
// the launch reads and records, or null.
static void team_args(const sf_sim *s, StepArgs &a, int rcap, uint32_t *cost)
{
    a.cost = cost;
    a.team_tab = s->team.tab; a.xg = s->team.xg; a.xbuf = s->team.xbuf; a.xdone = s->team.xdone; a.xerr = s->team.xerr_mapped;
    a.xrow = team_xrow(s->g); a.team_rcap = rcap;
    // placement of the members: 0 (default) = the slots of one XCD, 1 = consecutive slots (eight XCDs in turn), 2 = as 0 but the
    // hand-off written through as if they were apart - results never depend on it (tests run all three)
    a.team_far = s->tune.v[SF_TUNE_TEAM_PLACEMENT] == 2;
    a.order = nullptr;
}

static int launch_k_run_join(sf_sim *s, StepArgs &a, int n_steps, const TeamGeo &t, bool eager)
{
    const Geo &g = s->g;
    SF_TRY(team_buffers(s, t));
    if (!s->team.xj) {
        SF_TRY(dev_alloc(s, &s->team.xj, (size_t)3 * g.E + 2));
        SF_TRY(dev_alloc(s, &s->team.xcut, (size_t)g.E));
        SF_TRY(dev_alloc(s, &s->team.jlog, (size_t)1 + 3 * kJoinLog));
    }
    HIPCHK(hipMemsetAsync(s->team.jlog, 0, sizeof(uint32_t), s->stream));
    s->team.jlog_valid = true;
    hipLaunchKernelGGL(k_team_plan, dim3(1), dim3(1024), 0, s->stream, g.E, t.slots, 1, 1, 0u, 0u, 1, s->run_cost, s->team.tab, s->team.size, s->team.xg, s->team.xdone, 0,
                       s->team.xj, s->team.xcut);
    s->team.plan_ones = 0;             // (this plan spreads the environments over the XCDs: not the table a launch of fixed teams of one keeps)
    team_args(s, a, 0, s->run_cost);
    a.xj = s->team.xj; a.xcut = s->team.xcut; a.tsize = s->team.size; a.jlog = s->team.jlog;
    // (k_team_plan's model of a team: the chain no member's update gets shorter than, what belonging to a team costs per update; eager - tests -:
    // every workgroup that is free joins whatever runs)
    // Where the newcomers come from: the environment's own XCD (default: the team's step boundaries and cuts stay in one L2 - measured on C3, 1000 updates:
    // teams spread over the XCDs pay ~12 k clocks per update for belonging, and every cut writes back and invalidates a whole L2 under 31 other
    // environments; 10.9 -> 12.7 us per update); SF_TUNE_TEAM_PLACEMENT 1 = from anywhere, 2 = the own XCD but every hand-off as if they were apart
    const int place = s->tune.v[SF_TUNE_TEAM_PLACEMENT];
    a.join_local = place == 1 ? 0 : (place == 2 ? 2 : 1);
    a.join_floor = eager ? 0 : 12000; a.join_ovh = eager ? 0 : (a.join_local == 1 ? 3000 : 12000);
    // (counters on: the instantiation that keeps the statistics, TEAM = 3, where TEAM = 2 is built without them - sf_run_kernels.h)
    RunKey key = run_key(g, kRunJoin, 1, false), counted = key;
    counted.team = 3;
    if (a.counters && run_fn(counted)) key = counted;
    return launch_run(s, key, (unsigned)t.slots, (unsigned)t.waves * 64, t.lds, a, n_steps, t.vcap, 64);
}


// keep_cost: the launch neither reads nor records what the environments cost (the catch-up launch behind a windowed one)
static int launch_k_run_team(sf_sim *s, StepArgs &a, int n_steps, const TeamGeo &t, int t_min, int t_max, int steps_before, bool keep_cost = false)
{
    const Geo &g = s->g;
    SF_TRY(team_buffers(s, t));
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
    if (!ones_key || s->team.plan_ones != ones_key)
        hipLaunchKernelGGL(k_team_plan, dim3(1), dim3(1024), 0, s->stream, g.E, t.slots, t_min, t_max, ovh, floor_c, scatter,
                           s->run_cost, s->team.tab, s->team.size, s->team.xg, s->team.xdone, keep_cost ? 1 : 0, (uint32_t *)nullptr, (unsigned long long *)nullptr);
    s->team.plan_ones = ones_key;
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
        const int F = s->planes.fire_rows(), wv = (F + 14) / 16 + 1;
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
                      g.H >= 64 && g.H <= 1024 && g.PV >= 4 && !g.dense && s->planes.fire_rows() > 0 && s->planes.fire_rows() <= 62 && n_steps <= 64 && !tn.set[SF_TUNE_RUN_WAVES] &&
                      g.diag && (tn.v[SF_TUNE_RUN_TEAM] == 0 || tn.v[SF_TUNE_RUN_TEAM] == 1) && s->fused_mode != 2;
        // (the launch behind k_win: while every fire surely ends the call inside 64 rows, 16-wave workgroups - an environment whose fire reached the
        // ring of a window placed to the vector gets a new window of 64 rows around where the fire stands now, 2 us per update instead of the
        // general loop's 6 in an 8-wave workgroup; everybody else's workgroup returns at once)
        const bool all_young = tn.v[SF_TUNE_RUN_WINDOW] != 0 && s->planes.fire_rows() > 0 && s->planes.fire_rows() + 2LL * n_steps <= 60;
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
    if (p.team_wide && !p.team_forced && tk == 0 && tgeo.rcap > 0 && s->planes.fire_rows() > 0) {
        // (cut_bands: the fire's tile rows, + ceil((updates + 1) / tile height) + 1 tile rows either side)
        const long long room = (long long)tgeo.rcap - s->planes.fire_rows() - 2LL * done - 7LL * g.LR * g.RB - 2;
        const long long fit = room / 2;              // updates the window is sure to hold
        // (only where the whole call stays young - measured on C4's share: one member for the first ~ 380 of 1000 updates and two
        // for the rest loses to two members throughout, 23.5 against 21.9 us per step; the driver's 20 after 5: 7.0 against 8.7)
        // (C4's share, calls of 60 / 100 / 150 / 250 / 350 updates after 20: one member 7.8 / 8.3 / 9.6 / 11.9 / 15.8 us per step, two 9.1 / 9.3 / 10.8 / 12.1 / 14.1)
        if (done == 0 && fit >= n_steps && s->planes.fire_rows() + 2LL * n_steps <= 480) { young = true; sg.n = n_steps - done; sg.recut = 0; }
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
    if (p.result) SF_TRY(mark_hist_dirty(s));
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
            if (g.VW > 1) s->planes.plain_run_wide();
        }
        if (sg.join || sg.team) s->last_team_max = sg.team_max;
        s->cost_steps = sg.n;
        done += sg.n;
        s->last_launches++;
    }
    if (p.win_only) s->cost_steps = n_steps;
    s->planes.resident_done(p.result, p.win_first);
    return SF_OK;
}

// Updates as planned (enqueue layer): the buffers their launches need, then the resident rollout or the per-step loop.  mit_dev / mit_k:
// control lines inside the resident launch (p planned with lines).  t0 (may be null): an event recorded in front of the step launches,
// behind the buffers' rebuilds - where a timed call's GPU time starts.
static int enqueue_steps(sf_sim *s, StepPlan p, int n_steps, const int32_t *mit_dev, int mit_k, hipEvent_t t0)
{
    const Geo &g = s->g;
    const Tuning &tn = s->tune;
    const bool row_was_fresh = s->planes.call_begins();      // the result block on the device is current as this call starts
    s->last_launches = 0;
    const int n_requested = n_steps;
    if (n_steps != 1 || mit_dev || s->last_was_step1) s->step1_polls = 0;       // (another kind of call, or nobody looked at the last update's result)
    if (p.nw) {
        int rc0 = ensure_commit(s);            // k_run starts from commit[] and leaves the new states there
        if (rc0) return rc0;
        // (a team launch reads all three planes of the vector bitmap; a launch of the plain kernel on rows of several words has kept only the first)
        if (p.team_forced || p.team_wide || p.team_auto) s->planes.team_launch_next();
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
        a.from_commit = (i == 0 && s->planes.committed()) ? 1 : 0;      // (the first launch leaves the states in the rings)
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
    }
    s->planes.per_step_enqueued(p.generic, p.fused, n_steps);
    s->planes.updates_made(n_requested, g.H);
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
    if (!s->wind.sched.empty()) {          // a wind schedule is set: the tables that are due, in front of the call's first piece
        int rc0 = wind_sched_pass(s);
        if (rc0) return rc0;
    }
    if (!s->arrival.plane) return enqueue_steps(s, p, n_steps, mit_dev, mit_k, t0);
    const Geo &g = s->g;
    int rc = SF_OK, launches = 0;
    if (t0 && hipEventRecord(t0, s->stream) != hipSuccess) rc = fail(SF_EHIP, "sf_step: hipEventRecord failed");
    for (int done = 0; done < n_steps && !rc;) {
        if (s->arrival.pending >= g.md) { rc = arrival_pass(s); continue; }      // (a call that failed half way left them behind)
        const int room = g.md - s->arrival.pending;
        const int pieces = (n_steps - done + room - 1) / room;
        const int c = hold ? std::min(n_steps - done, room) : (n_steps - done + pieces - 1) / pieces;
        const StepPlan pc = c == n_steps ? p : plan_step(s, c, mit_dev != nullptr);
        if (mit_dev && !pc.nw) { rc = fail(SF_EHIP, "sf_step_mitigated: a piece of %d updates was not planned as a resident launch", c); break; }
        rc = enqueue_steps(s, pc, c, mit_dev ? mit_dev + (size_t)done * g.E * mit_k * 3 : nullptr, mit_k, nullptr);
        launches += s->last_launches;
        s->arrival.pending += c;
        done += c;
        if (!rc && (!hold || s->arrival.pending >= g.md)) rc = arrival_pass(s);      // behind every piece; a caller that holds: every md updates
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
    SF_TRY(begin_call(s, who, kNeedRt | kNeedReset));
    SF_TRY(step_impl(s, n_steps, false, ms ? s->ev0 : nullptr));
    return finish_call(s, who, !s->async, ms);
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
    if (i == 0) { (void)s->planes.call_begins(); s->last_launches = 0; s->step1_polls = 0; }
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
    SF_TRY(begin_call(s, who, kNeedRt | kNeedReset));
    const StepPlan plan = plan_step(s, n_steps, true);       // can the resident launch take the lines?  Otherwise scatter + step pairs
    const int32_t *blk = nullptr;
    SF_TRY(stage_lines(s, n_steps, pts, k, device_pointer, &blk));
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
    if (s->arrival.pending) SF_TRY(arrival_pass(s));
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
    a.mit = s->loop.pts_mem; a.mit_k = s->loop.k;
    a.res_block = s->status_block; a.res_elapsed = s->elapsed_dev; a.res_sink = s->sink;
    a.cost = s->run_cost;
    a.loop_db = s->loop.db_dev; a.loop_pts_host = s->loop.pts_dev; a.loop_res_host = s->loop.res_dev;
    a.loop_seq = s->loop.mem; a.loop_done = s->loop.mem + 32; a.loop_pts = s->loop.pts_mem;
    a.loop_timeout = 400000000ull;             // ~0.2 s without a ring: the workgroups leave, the next sf_loop_step starts them again
    HIPCHK(hipMemsetAsync(s->loop.mem, 0, sizeof(uint32_t), s->stream));       // nothing forwarded yet (the word may hold the stop of the launch before)
    // one 16-wave workgroup per environment - or the light loop's 8-wave one (SF_TUNE_LOOP_LIGHT)
    const int nw_cap = s->loop.light ? 8 : 16;
    const int nw = (g.H + 63) / 64 < nw_cap ? (g.H + 63) / 64 : nw_cap;
    long long all_vec = (long long)g.H * g.PV;
    int vcap = s->loop.light ? 1024 : 4096;
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
    if (!s->wind.sched.empty()) return fail(SF_ENOTSUP, "sf_loop_start: not while a wind schedule is set (sf_set_wind_schedule): a closed loop has no call boundary for the wind to change at");
    if (s->arrival.plane) return fail(SF_ENOTSUP, "sf_loop_start: not while arrival times are recorded (sf_enable_arrival): a closed loop has no launch boundary for the pass");
    if (g.ab != 1 || s->generic || g.VW != 1 || s->graph_on || s->history || g.dense || g.H > 16 * 64 || g.E > s->n_cu ||
        (s->fused_mode >= 0 && s->fused_mode != 2))
        return fail(SF_ENOTSUP, "sf_loop_start: needs the environment-resident launch with every environment resident at once "
                                "(grids up to 1024 x 1024, max_fire_duration <= 5, no more environments than CUs, no spread graph / history)");
    LOOP_QUIESCE(s);                   // (a refused call leaves a running loop running)
    s->loop.light = light;
    { int rc0 = ensure_commit(s); if (rc0) return rc0; }
    { int rc0 = ensure_vbits(s); if (rc0) return rc0; }
    { int rc0 = ensure_bl(s); if (rc0) return rc0; }
    auto pin = [&](void **host, void **dev, size_t bytes) -> int {
        HIPCHK(hipHostMalloc(host, bytes, hipHostMallocMapped | hipHostMallocCoherent));      // fine-grained: no GPU cache may hold these lines
        HIPCHK(hipHostGetDevicePointer(dev, *host, 0));
        memset(*host, 0, bytes);
        return SF_OK;
    };
    if (!s->loop.db) {
        SF_TRY(pin((void **)&s->loop.db, (void **)&s->loop.db_dev, sizeof(uint32_t) * 64));
        SF_TRY(pin((void **)&s->loop.res, (void **)&s->loop.res_dev, (size_t)64 * g.E));
        HIPCHK(hipMalloc(reinterpret_cast<void **>(&s->loop.mem), sizeof(uint32_t) * (32 + (size_t)g.E)));
    }
    s->loop.slot_ints = (size_t)g.E * k * 4;        // a slot of the points ring: 16-byte pieces (column, row, type, the step's number)
    const size_t pts_bytes = sizeof(int32_t) * 2 * (s->loop.slot_ints ? s->loop.slot_ints : 4);
    if (pts_bytes > s->loop.pts_cap) {
        if (s->loop.pts) HIPCHK(hipHostFree(s->loop.pts));
        if (s->loop.pts_mem) HIPCHK(hipFree(s->loop.pts_mem));
        s->loop.pts = nullptr; s->loop.pts_mem = nullptr; s->loop.pts_cap = 0;
        SF_TRY(pin((void **)&s->loop.pts, (void **)&s->loop.pts_dev, pts_bytes));
        HIPCHK(hipMalloc(reinterpret_cast<void **>(&s->loop.pts_mem), pts_bytes));
        s->loop.pts_cap = pts_bytes;
    }
    s->loop.k = k; s->loop.seq = 0; s->loop.restarts = 0;
    volatile uint32_t *db = s->loop.db;
    for (int i = 0; i < 64; ++i) db[i] = 0;
    memset(s->loop.res, 0, (size_t)64 * g.E);
    memset(s->loop.pts, 0, pts_bytes);             // (pieces of an earlier loop carry ITS step numbers)
    __sync_synchronize();
    HIPCHK(hipMemsetAsync(s->loop.mem, 0, sizeof(uint32_t) * (32 + (size_t)g.E), s->stream));
    HIPCHK(hipMemsetAsync(s->loop.pts_mem, 0, pts_bytes, s->stream));
    SF_TRY(mark_hist_dirty(s));
    s->planes.loop_started();
    SF_TRY(loop_launch(s));
    HIPCHK(hipGetLastError());
    s->loop.on = true;
    return SF_OK;
}

/* pts: int32 [n_envs][k][3] = (column, row, type) of this step (k as given to sf_loop_start; entries with a type outside 3..5 are
 * padding), or null = no points.  status_out: int32 [n_envs][8] (like sf_get_status) or null; elapsed_out: double [n_envs] or null. */
extern "C" int sf_loop_step(sf_sim *s, const int32_t *pts, int32_t *status_out, double *elapsed_out)
{
    if (!s) return fail(SF_EINVAL, "sf_loop_step: null handle");
    if (!s->loop.on) return fail(SF_ESTATE, "sf_loop_step: call sf_loop_start first");
    const Geo &g = s->g;
    const uint32_t seq = s->loop.seq + 1;
    if (seq >= 0x7FFFFFF0u) return fail(SF_ESTATE, "sf_loop_step: sequence numbers exhausted; sf_loop_stop and start again");
    if (s->loop.k > 0) {
        // the points are their own doorbell: 16-byte pieces that carry the step's number, each written by ONE 16-byte store (the relay takes a
        // piece when it carries the number it waits for)
        __m128i *slot = reinterpret_cast<__m128i *>(s->loop.pts + (size_t)(seq & 1u) * s->loop.slot_ints);
        const size_t n = (size_t)g.E * s->loop.k;
        if (pts) for (size_t i = 0; i < n; ++i) _mm_store_si128(slot + i, _mm_set_epi32((int)seq, pts[3 * i + 2], pts[3 * i + 1], pts[3 * i]));
        else for (size_t i = 0; i < n; ++i) _mm_store_si128(slot + i, _mm_set_epi32((int)seq, 0, 0, 0));
    }
    volatile uint32_t *db = s->loop.db;
    __sync_synchronize();                                    // the points are in memory before the number that announces them
    db[0] = seq;
    s->loop.seq = seq;
    s->planes.updates_made(1, g.H);
    // wait for the "done" number; should the launch have left by itself (no ring for loop_timeout clocks), start it again: every
    // workgroup resumes from its own "done" number, the points of this step are still in their slot
    const volatile uint32_t *res = reinterpret_cast<const volatile uint32_t *>(s->loop.res);
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
            if (s->team.xerr_pinned && *s->team.xerr_pinned) return fail(SF_EHIP, "sf_loop_step: the resident launch failed");
            HIPCHK(hipSetDevice(s->p.device));
            s->loop.restarts++;
            { int rc0 = loop_launch(s); if (rc0) return rc0; }
            HIPCHK(hipGetLastError());
        }
    }
    return SF_OK;
}

extern "C" int sf_loop_stop(sf_sim *s) { return s ? loop_stop(s) : fail(SF_EINVAL, "sf_loop_stop: null handle"); }
static int loop_stop(sf_sim *s)
{
    if (!s->loop.on) return SF_OK;
    HIPCHK(hipSetDevice(s->p.device));
    volatile uint32_t *db = s->loop.db;
    __sync_synchronize();
    db[0] = s->loop.seq | kLoopStop;
    __sync_synchronize();
    s->loop.on = false;
    HIPCHK(hipStreamSynchronize(s->stream));      // the workgroups commit their environments and leave the result block behind
    s->planes.loop_stopped();
    return SF_OK;
}

extern "C" int sf_loop_restarts(sf_sim *s, int32_t *out)
{
    if (!s || !out) return fail(SF_EINVAL, "sf_loop_restarts: null argument");
    *out = s->loop.restarts;
    return SF_OK;
}

static int get_maps(sf_sim *s, int env0, int n, uint8_t *out)
{
    const Geo &g = s->g;
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    if (s->last_was_step1) { s->last_was_step1 = false; s->step1_polls = 0; }      // (a loop that looks at the maps after every update: per-step kernels)
    const size_t bytes = (size_t)n * g.H * g.W;
    SF_TRY(ensure_stage(s, bytes));
    dim3 blk(256), grd((g.W + 255) / 256, g.H, n);
    hipLaunchKernelGGL(k_unpack_status, grd, blk, 0, s->stream, g, cur_planes(s), env0, (uint8_t *)s->stage, (uint8_t *)nullptr);
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
        SF_TRY(get_maps(s, e, n, out + (size_t)e * s->g.H * s->g.W));
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
    if (!s->delta.snap) {
        SF_TRY(dev_alloc(s, &s->delta.snap, (size_t)g.E * g.plane_env));
        s->delta.snap_valid.assign((size_t)g.E, 0);
    }
    if (cap > s->delta.cap || !s->delta.dev) {
        HIPCHK(hipStreamSynchronize(s->stream));
        if (s->delta.dev) { HIPCHK(hipFree(s->delta.dev)); s->delta.dev = nullptr; }
        if (s->delta.pinned) { HIPCHK(hipHostFree(s->delta.pinned)); s->delta.pinned = nullptr; }
        const int c = cap > kInline ? cap : kInline;
        HIPCHK(hipMalloc(reinterpret_cast<void **>(&s->delta.dev), ((size_t)c + kDeltaHead) * sizeof(uint32_t)));
        HIPCHK(hipHostMalloc(reinterpret_cast<void **>(&s->delta.pinned), ((size_t)c + kDeltaHead + 16) * sizeof(uint32_t), hipHostMallocDefault));      // (+ 16: a row that could not travel with a list, sf_run_delta)
        HIPCHK(hipMemsetAsync(s->delta.dev, 0, sizeof(uint32_t), s->stream));
        s->delta.cap = c;
        s->delta.base = 0;
    }
    if (!s->delta.snap_valid[env]) {
        // no reference point: the current map becomes it, the caller fetches the whole map
        dim3 blk(256), grd((g.W + 255) / 256, g.H, 1);
        SF_TRY(ensure_stage(s, (size_t)g.H * g.W));
        hipLaunchKernelGGL(k_unpack_status, grd, blk, 0, s->stream, g, cur_planes(s), env, (uint8_t *)s->stage, s->delta.snap);
        HIPCHK(hipGetLastError());
        s->delta.snap_valid[env] = 1;
        *mode = 1;
        return SF_OK;
    }
    hipLaunchKernelGGL(k_map_delta, dim3((g.PV + 255) / 256, g.H), dim3(256), 0, s->stream, g, cur_planes(s), env,
                       s->delta.snap + (size_t)env * g.plane_env, s->delta.dev, cap, s->delta.base,
                       with_row ? (const int32_t *)(s->status_block + (size_t)env * 8) : nullptr, (const double *)(s->elapsed_dev + env));
    HIPCHK(hipGetLastError());
    const int first = cap < kInline ? cap : kInline;
    HIPCHK(hipMemcpyAsync(s->delta.pinned, s->delta.dev, ((size_t)first + kDeltaHead) * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    *mode = 0;
    return SF_OK;
}
// behind the wait for the stream: the list out of the landing zone (a second copy if it is longer than what travelled with the count)
static int delta_finish(sf_sim *s, int cap, uint32_t *cells_out, int32_t *n_out)
{
    constexpr int kInline = 1024;
    const int first = cap < kInline ? cap : kInline;
    const uint32_t n = s->delta.pinned[0] - s->delta.base;
    s->delta.base = s->delta.pinned[0];
    if (n > (uint32_t)cap) { *n_out = -1; return SF_OK; }      // (the reference point is current: the caller fetches the whole map)
    if (n > (uint32_t)first) {
        HIPCHK(hipMemcpyAsync(s->delta.pinned + kDeltaHead + first, s->delta.dev + kDeltaHead + first, ((size_t)n - first) * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));
    }
    if (n) memcpy(cells_out, s->delta.pinned + kDeltaHead, (size_t)n * sizeof(uint32_t));
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
    SF_TRY(delta_enqueue(s, env, cap, &mode));
    SF_TRY(finish_call(s, "sf_get_fire_map_delta", true, nullptr));
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
    SF_TRY(refresh_status(s, nullptr));      // (nothing to launch behind a resident launch: it has left the block behind itself)
    int mode = 0;
    SF_TRY(delta_enqueue(s, env, cap, &mode, true));
    uint32_t *land = s->delta.pinned + 1;          // the row and its elapsed_time have travelled with the list's count ...
    if (mode == 1) {                               // ... unless there was no list
        land = s->delta.pinned + s->delta.cap + kDeltaHead;
        HIPCHK(hipMemcpyAsync(land, s->status_block + (size_t)env * 8, 8 * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
        HIPCHK(hipMemcpyAsync(land + 8, s->elapsed_dev + env, sizeof(double), hipMemcpyDeviceToHost, s->stream));
    }
    SF_TRY(finish_call(s, "sf_run_delta", true, nullptr));
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
    SF_TRY(ensure_stage(s, bytes));
    dim3 blk(256), grd((g.W + 255) / 256, g.H);
    SF_TRY(ensure_commit(s));
    SF_TRY(ensure_rm(s));
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
    SF_TRY(ensure_stage(s, bytes));
    dim3 blk(256), grd((g.W + 255) / 256, g.H);
    SF_TRY(ensure_commit(s));
    SF_TRY(ensure_rm(s));
    if (g.att)   // the caller's values are the truth now: nothing is owed any more
        hipLaunchKernelGGL(k_settle_env, grd, blk, 0, s->stream, g, (const uint8_t *)s->status, s->settled, s->burn,
                           (const EnvState *)s->commit, env, 0);
    HIPCHK(hipMemcpyAsync(s->stage, burn, bytes, hipMemcpyHostToDevice, s->stream));
    hipLaunchKernelGGL(k_pack_burn, grd, blk, 0, s->stream, g, s->burn, env, (const double *)s->stage);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s->stream));
    return SF_OK;
}

#include "sf_host_state.h"
#include "sf_host_ignite.h"

#include "sf_host_agents.h"

// The result block made current on the device (enqueue layer), also written to copy_to (may be null) and the registered sink.
static int refresh_status(sf_sim *s, int32_t *copy_to)
{
    const Geo &g = s->g;
    { int rc0 = ensure_commit(s); if (rc0) return rc0; }
    if (s->planes.row_fresh()) {
        // the resident launch has left the block (and the registered sink's copy) behind: nothing to count
        if (copy_to && copy_to != s->sink)
            HIPCHK(hipMemcpyAsync(copy_to, s->status_block, sizeof(int32_t) * 8 * g.E, hipMemcpyDeviceToDevice, s->stream));
        return SF_OK;
    }
    int32_t *sink2 = s->sink && s->sink != copy_to ? s->sink : nullptr;       // the registered sink follows every refresh
    if (g.ab == 1 && !s->generic) {
        // per-tile histograms: only the tiles touched since the last query are recounted; one launch writes the whole block
        SF_TRY(mark_hist_dirty(s));
        hipLaunchKernelGGL(k_counts_tiles, dim3((unsigned)g.E), dim3(1024), 0, s->stream, g, cur_planes(s), s->tdirty, s->thist,
                           (const EnvState *)s->commit, s->status_block, s->elapsed_dev, copy_to ? copy_to : sink2);
        if (copy_to && sink2) HIPCHK(hipMemcpyAsync(sink2, s->status_block, sizeof(int32_t) * 8 * g.E, hipMemcpyDeviceToDevice, s->stream));
        s->planes.counted(true);           // (the block - and the registered sink's copy - is current until something changes a status byte)
    } else {
        { int rc0 = ensure_rm(s); if (rc0) return rc0; }
        HIPCHK(hipMemsetAsync(s->status_block, 0, sizeof(int32_t) * 8 * g.E, s->stream));
        int bx = g.H < 64 ? g.H : 64;
        hipLaunchKernelGGL(k_counts, dim3(bx, g.E), dim3(256), 0, s->stream, g, (const uint8_t *)s->status,
                           (const EnvState *)s->commit, s->status_block);
        s->planes.counted(false);
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
    SF_TRY(begin_call(s, who, 0));
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
    SF_TRY(status_query(s, "sf_get_status", nullptr));
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
    s->planes.sink_replaced();                     // the new sink is filled by the next refresh
    return SF_OK;
}

#include "sf_host_comm.h"

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
    if (s->planes.blocked()) {
        // the resident launch keeps the cells in its blocked plane: the row-major status plane is refreshed from it (one sweep) and
        // is a snapshot until the next call - the blocked plane stays the current one, nothing is converted back
        const Geo &g = s->g;
        hipLaunchKernelGGL(k_bl_to_rm, dim3((g.PV + 63) / 64, g.H, g.E), dim3(64), 0, s->stream, g, (const uint8_t *)s->cells, s->status, (uint8_t *)nullptr);
        HIPCHK(hipGetLastError());
    } else s->planes.alias_handed_out();      // the caller holds a writable alias of the status plane: recount everything at the next query
    HIPCHK(hipStreamSynchronize(s->stream));
    *ptr = s->status; *row_pitch = s->g.P; *env_stride = s->g.plane_env;
    return SF_OK;
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
