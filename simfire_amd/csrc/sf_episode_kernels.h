// New episodes drawn on the device (sf_episodes_*): the ignition cell, the uniform wind and the agents' start
// cells of every environment that a reset is about to take, made by a counter-based draw that depends on (seed, environment, episode
// index) alone - not on the tick, the launch structure or the order in which environments finish.  k_episode_draw runs in front of
// the two reset kernels with the same mask and decides "taken" by their function (reset_taken, sf_reset_kernels.h); what it writes is
// what they and k_wind_rtable then read from device memory.  Part of simfire_hip.hip only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sf_common.h"
#include "sf_reset_kernels.h"

namespace {

constexpr int kEpAttempts = 64;       // ignition attempts of SF_EP_LIVE_CELL: one per lane (slots 0 .. 63)
constexpr uint32_t kEpSlotAgent = 64, kEpSlotU = 128, kEpSlotDir = 129;

// splitmix64's finaliser; everything modulo 2^64
__host__ __device__ __forceinline__ uint64_t ep_mix(uint64_t z)
{
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
// word `slot` of episode `ep` of environment `env`: a stream per (seed, environment), a counter (episode, slot) inside it
__host__ __device__ __forceinline__ uint64_t ep_word(uint64_t seed, uint32_t env, uint32_t ep, uint32_t slot)
{
    const uint64_t G = 0x9E3779B97F4A7C15ull;
    return ep_mix(ep_mix(seed + G * ((uint64_t)env + 1)) + G * (((uint64_t)ep << 8) | slot));
}
// an integer of [lo, hi] from a 32-bit half (multiply-shift: no division, no rejection)
__host__ __device__ __forceinline__ int ep_int(uint32_t h, int lo, int hi)
{
    return lo + (int)(((uint64_t)h * (uint64_t)(hi - lo + 1)) >> 32);
}
// a double of [a, b) from the word's upper 53 bits; mul then add (the library is built with -ffp-contract=off)
__host__ __device__ __forceinline__ double ep_double(uint64_t w, double a, double b)
{
    const double u = (double)(w >> 11) * 0x1.0p-53;
    const double d = (b - a) * u;
    return a + d;
}
// the cell of a box (x0, y0, x1, y1, inclusive): x from the high half over its columns, y from the low half over its rows
__host__ __device__ __forceinline__ void ep_cell(uint64_t w, const int32_t *box, int &x, int &y)
{
    x = ep_int((uint32_t)(w >> 32), box[0], box[2]);
    y = ep_int((uint32_t)w, box[1], box[3]);
}

struct EpisodeArgs {
    int H, W, P, E;
    const uint8_t *mask;             // as ResetArgs::mask (null: the environments whose result row shows them not running)
    const EnvState *commit;
    uint64_t seed;
    int flags;                       // SF_EP_*
    int32_t ign_box[4], agent_box[4];
    double U[2], U_dir[2];
    const double *rt;                // direction-major R tables (SF_EP_LIVE_CELL)
    long long tab_stride;            // elements between the tables of two environments (0: one shared table)
    uint32_t *index;                 // [E] the next episode of an environment
    int32_t *ign;                    // [E][2] what the reset behind this kernel ignites
    double *wind;                    // [E][2] the last wind drawn (U ft/min, U_dir degrees)
    int K;                           // agents per environment (0: none, or SF_EP_AGENTS off)
    int32_t *start, *xyid;           // AgentArgs::start / xyid
    uint32_t *due_cnt;               // the list k_wind_rtable takes: zero when the kernel starts
    int32_t *due;
    double *due_U, *due_D;
};

// One wave per environment, the grid over all of them; a wave whose environment the reset will not take leaves after one load.
// Nothing the predicate reads is written here.  Every lane reads index[e] before lane 0 - last of all - overwrites it, which is
// ordered inside one wave only: hence workgroups of exactly one wave.
static_assert(kEpAttempts == 64, "k_episode_draw is written for workgroups of exactly one wave");
__global__ __launch_bounds__(kEpAttempts) void k_episode_draw(EpisodeArgs a)
{
    const int e = blockIdx.x, lane = threadIdx.x;
    if (!reset_taken(a.mask, a.commit, e)) return;
    const uint32_t ep = a.index[e];
    if (a.flags & SF_EP_IGNITION) {
        // lane = attempt.  The first attempt that succeeds wins - what a loop over the attempts would choose; where none does,
        // attempt 63's cell is taken as it is (a box of dead cells still ignites somewhere, and burns nothing)
        int x, y;
        ep_cell(ep_word(a.seed, (uint32_t)e, ep, (uint32_t)lane), a.ign_box, x, y);
        bool ok = true;
        if (a.flags & SF_EP_LIVE_CELL) {
            const double *t = a.rt + (long long)e * a.tab_stride + (long long)y * a.P + x;
            const long long plane = (long long)a.H * a.P;
            ok = false;
#pragma unroll
            for (int k = 0; k < 8; ++k) ok = ok || t[k * plane] != 0.0;
        }
        const unsigned long long won = __ballot(ok);
        const int win = won ? __ffsll(won) - 1 : kEpAttempts - 1;
        x = __shfl(x, win); y = __shfl(y, win);
        if (lane == 0) { a.ign[2 * e] = x; a.ign[2 * e + 1] = y; }
    }
    if ((a.flags & SF_EP_AGENTS) && lane < a.K) {       // behind k_agents_finish, which has sent the agents to the OLD start cells
        int x, y;
        ep_cell(ep_word(a.seed, (uint32_t)e, ep, kEpSlotAgent + (uint32_t)lane), a.agent_box, x, y);
        const long long o = (long long)e * a.K + lane;
        a.start[o * 2] = x; a.start[o * 2 + 1] = y;
        a.xyid[o * 3] = x; a.xyid[o * 3 + 1] = y;       // (the id stays lane + 1)
    }
    if (lane == 0) {
        if (a.flags & SF_EP_WIND) {
            const double U = ep_double(ep_word(a.seed, (uint32_t)e, ep, kEpSlotU), a.U[0], a.U[1]);
            const double D = ep_double(ep_word(a.seed, (uint32_t)e, ep, kEpSlotDir), a.U_dir[0], a.U_dir[1]);
            a.wind[2 * e] = U; a.wind[2 * e + 1] = D;
            const uint32_t at = atomicAdd(a.due_cnt, 1u);       // (as k_wind_due; an environment appends once: at < E)
            a.due[at] = e;
            a.due_U[at] = U;
            a.due_D[at] = D;
        }
        a.index[e] = ep + 1u;
    }
}

}  // namespace
