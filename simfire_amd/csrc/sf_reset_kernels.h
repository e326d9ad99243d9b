// Reset: new episodes in one, many or all environments of a handle at once (k_reset_envs zeroes their slices, k_reset_ignite puts
// the ignitions, states and result rows down behind it on the same stream).  The only reset there is: sf_reset, sf_reset_env,
// sf_reset_envs, sf_reset_where and the agents' auto-reset all launch these two (reset_launch in simfire_hip.hip, the one unit
// that includes this file); what is written per environment is DESIGN.md section 15.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sf_common.h"
#include "sf_env_segs.h"

namespace {

struct ResetArgs {
    Geo g;
    EnvSeg seg[kEnvSegs];               // the slices to zero (sf_env_segs.h)
    int n_seg;
    // which environments.  List form: envs[n] (distinct) with xy[n][2].  Mask form (envs == null, n == E): environment e is taken iff
    // mask[e] != 0 - or, without a mask, iff commit[e].running != 1: what its result row shows as not running (0, or 2 = QUIT on the
    // runtime check and still pruning, sf_set_prune_after_quit) - and its ignition xy[e] lies on the grid.
    const int32_t *envs;
    const uint8_t *mask;
    const int32_t *xy;
    int n;
    // what k_reset_ignite writes
    CellPlanesMut pl;                    // the status bytes - and, blocked, the sprite masks - in whichever plane is current
    uint8_t *age;                        // the row-major sprite masks
    EnvState *commit;
    uint8_t *tflags;
    int ring;
    unsigned long long *vbits, *win_hint;
    uint8_t *seam;                       // null unless the row-major planes are current and the sprite plane is 1 byte wide
    uint8_t *tdirty;                     // null unless the tile histograms are known (they are zeroed then: all UNBURNED)
    int32_t *res_block, *res_sink;
    double *res_elapsed;
};

// The mask form's choice: is environment e taken?  Shared with k_episode_draw (sf_episode_kernels.h), which draws the new episode's
// parameters for exactly the environments the reset behind it takes.
__device__ __forceinline__ bool reset_taken(const uint8_t *mask, const EnvState *commit, int e)
{
    return mask ? mask[e] != 0 : commit[e].running != 1;
}

// Entry i of the launch: the environment it resets, or -1.  Both kernels decide by this function; k_reset_envs changes nothing it
// reads (commit[] is written by k_reset_ignite only, the mask and the ignitions are the caller's).
__device__ __forceinline__ int reset_pick(const ResetArgs &a, int i, int &x, int &y)
{
    int e = i;
    if (a.envs) e = a.envs[i];
    else if (!reset_taken(a.mask, a.commit, i)) return -1;
    x = a.xy[2 * i]; y = a.xy[2 * i + 1];
    if (x < 0 || x >= a.g.W || y < 0 || y >= a.g.H) return -1;      // (list form: the host has refused these before the launch)
    return e;
}

// blockIdx.y = entry, blockIdx.x with the grid's x extent strides over every slice (env_seg_walk, sf_env_segs.h); the workgroups of
// an entry that is not taken return after that one load.  Stores only: nothing is read from the slices.
__global__ __launch_bounds__(256) void k_reset_envs(ResetArgs a)
{
    int x, y;
    const long long e = reset_pick(a, blockIdx.y, x, y);
    if (e < 0) return;
    const long long gtid = (long long)blockIdx.x * blockDim.x + threadIdx.x, gstride = (long long)gridDim.x * blockDim.x;
    for (int k = 0; k < a.n_seg; ++k) {
        const EnvSeg c = a.seg[k];
        env_seg_walk<false>(c.base + e * c.stride, nullptr, c.len, gtid, gstride);
    }
}

// One thread per entry, launched behind k_reset_envs on the same stream: the ignition cell with its tile flag, bitmap words and the
// seam bytes k_rebuild_seams would find for a lone cell, the window hint, the state of update 0 and the result row that goes with it
// (running, 0 update() calls, cells per BurnStatus - the launches that follow bring it up to date by difference).
__global__ __launch_bounds__(256) void k_reset_ignite(ResetArgs a)
{
    const Geo &g = a.g;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    int x, y;
    const int e = reset_pick(a, i, x, y);
    if (e < 0) return;
    const int tyw = y / (g.LR * g.RB), tx = (x / 16) / g.LC;
    if (a.tdirty) a.tdirty[((long long)e * g.TY + tyw) * g.TX + tx] = 1;      // only the ignition's tile is to be recounted
    if (a.pl.cells) {                   // the blocked cell plane is the current one (1-byte sprite masks)
        uint8_t *sp = bl_status(a.pl.cells, g, e, y, x);
        *sp = SF_BURNING;
        *bl_mask_beside(sp) = 1u;
    } else {
        a.pl.status[(long long)e * g.plane_env + (long long)y * g.P + x] = SF_BURNING;
        age_store(g, a.age + (long long)e * g.age_env * g.ab, (long long)y * g.P + x, 1u);   // ignition step 0
    }
    if (a.seam) {                       // the copies of the sprite columns either side of a chunk boundary (k_rebuild_seams)
        const int cw = g.LC * 16;
        int b = -1, side = 0;
        if ((x + 1) % cw == 0) { b = (x + 1) / cw; side = 0; }
        else if (x % cw == 0) { b = x / cw; side = 1; }
        if (b >= 1 && b < g.chunks_x) a.seam[(long long)e * g.seam_env + (long long)(b * 2 + side) * g.Hs + y + kSeamPad] = 1u;
    }
    a.tflags[(((long long)a.ring * g.E + e) * g.TYp + tyw + 1) * g.TXp + tx + 1] = 1 | 4 | 8 | 16 | 32;   // all edge bits: conservative
    {
        const long long o = (long long)e * g.vb_env + (long long)y * g.VW + (x >> 10), plane = (long long)g.E * g.vb_env;
        const unsigned long long bit = 1ull << ((x >> 4) & 63);
        a.vbits[o] = bit;
        if ((x & 15) == 0) a.vbits[plane + o] = bit;
        if ((x & 15) == 15) a.vbits[2 * plane + o] = bit;
    }
    a.win_hint[e] = 0ull;               // (where the old fire stood says nothing about the new one)
    EnvState s;
    s.running = 1; s.steps = 0; s.complete = 0; s.elapsed = 0.0;
    s.time_quit = g.has_max_time && (g.update_rate > g.max_time || 0.0 > g.max_time);
    a.commit[e] = s;
    const int32_t row[8] = {1, 0, g.H * g.W - 1, 1, 0, 0, 0, 0};
    for (int k = 0; k < 8; ++k) {
        a.res_block[(long long)e * 8 + k] = row[k];
        if (a.res_sink) a.res_sink[(long long)e * 8 + k] = row[k];
    }
    a.res_elapsed[e] = 0.0;
}

}  // namespace
