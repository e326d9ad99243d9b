// Arrival times (sf_enable_arrival): the pass the host enqueues BEHIND the step launches - no step kernel knows
// about it.  Part of simfire_hip.hip only (the run units do not include it).
//
// The sprite masks are indexed by ABSOLUTE ignition step (sf_common.h, make_masks): a sprite created by update s (fire.py:571-587) owns
// bit slot_of(s, N), N = md + 3, of its cell's mask, and the bit is set at least until the prune of update s + md + 1 has looked at it.
// So a pass that finds an environment at t updates can name the ignition step of every sprite created by the updates t - md .. t: the
// bit at distance d = (slot_of(t) - bit) mod N belongs to s = t - d, and d <= md is unambiguous (the slots of d = md + 1, md + 2 - a
// pruned sprite's bit waiting to be recycled - are the only others).  With a pass at least every md updates nothing is missed.
// arrival1 (u32 [E][H][P]) holds s + 1, 0 = never; a cell is written only while it is 0, so the first sprite of a cell stays (a line
// drawn on a burning cell lets it ignite again) and a bit seen by two passes is harmless.  One lane owns a cell: plain loads and stores.
// A frozen environment (EnvState.running == 0) keeps its update count and its masks: it decodes to what it decoded before.  One that
// still prunes after QUIT (running == 2) counts its updates on (fold_state) and recycles its slots by them, like a running one.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sf_common.h"

namespace {

// What decodes the masks of an environment that has made t updates: rotate a mask right by k so that the bit of s = t - d sits at
// position N - 1 - d, drop positions 0 and 1 (d = md + 2, md + 1); the LOWEST bit left is the oldest sprite.
struct ArrivalKey {
    int t, N, k;
    uint32_t all;
};
__device__ __forceinline__ ArrivalKey arrival_key(int t, const Geo &g)
{
    ArrivalKey q;
    q.t = t; q.N = g.N;
    const int s1 = slot_of(t, g.N) + 1;
    q.k = s1 == g.N ? 0 : s1;
    q.all = (1u << g.N) - 1u;
    return q;
}
// s + 1 of the oldest sprite of mask m that the updates t - md .. t created, 0 = none
__device__ __forceinline__ uint32_t arrival_of(const ArrivalKey &q, uint32_t m)
{
    const uint32_t r = (q.k ? ((m >> q.k) | (m << (q.N - q.k))) : m) & q.all & ~3u;
    if (!r) return 0u;
    const int s = q.t - (q.N - 1 - (__ffs((int)r) - 1));
    return s < 0 ? 0u : (uint32_t)s + 1u;       // (no update before the reset: a bit that says so is not a sprite's)
}

// Sparse form: the blocked plane is current and plane 0 of the vector bitmap is valid (bit v of row y: the 16-cell vector holds a
// sprite bit).  One lane per bitmap word - 64 consecutive rows (one-word rows) per wave; a lane walks the set bits of its word, loads
// the vector's 16 mask bytes from its sector and decodes the bytes that are not zero.  A fire is a ring a few cells thick: a row's
// word holds a handful of bits, and the loads of a wave's lanes - different rows, the same columns - are independent of each other.
__global__ __launch_bounds__(256) void k_arrival_bits(Geo g, const uint8_t *cells, const unsigned long long *vbits, const EnvState *commit,
                                                      uint32_t *arrival1)
{
    const int e = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;      // word of the environment: row i / VW, word i % VW of the row
    if (i >= g.H * g.VW) return;
    unsigned long long word = vbits[(long long)e * g.vb_env + i];
    if (!word) return;
    const ArrivalKey q = arrival_key(commit[e].steps, g);
    const int y = i / g.VW, v0 = (i - y * g.VW) * 64;
    uint32_t *row = arrival1 + (long long)e * g.plane_env + (long long)y * g.P;
    while (word) {
        const int v = v0 + __ffsll((long long)word) - 1;
        word &= word - 1ull;
        if (v >= g.PV) break;                                  // (no bit beyond the row's vectors; the bound of every access below)
        const uint4 m = *reinterpret_cast<const uint4 *>(bl_mask_vec(cells, g, e, y, v));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t d = pick(m, j);
            if (!d) continue;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const uint32_t a1 = arrival_of(q, (d >> (8 * b)) & 0xFFu);
                if (!a1) continue;
                uint32_t *p = row + v * 16 + j * 4 + b;
                if (*p == 0u) *p = a1;
            }
        }
    }
}

// Dense form: one thread per cell of whichever plane is current - the row-major sprite-mask plane of any width (T, as k_step_cells),
// or the blocked plane (cells != null; one-byte masks) where the bitmap cannot be relied on.
template <typename T>
__global__ __launch_bounds__(256) void k_arrival_cells(Geo g, const uint8_t *age, const uint8_t *cells, const EnvState *commit, uint32_t *arrival1)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, e = blockIdx.z;
    if (x >= g.W) return;
    uint32_t m;
    if (cells) m = *bl_mask(cells, g, e, y, x);
    else m = reinterpret_cast<const T *>(age)[(long long)e * g.age_env + (long long)y * g.P + x];
    if (!m) return;
    const uint32_t a1 = arrival_of(arrival_key(commit[e].steps, g), m);
    if (!a1) return;
    uint32_t *p = arrival1 + (long long)e * g.plane_env + (long long)y * g.P + x;
    if (*p == 0u) *p = a1;
}

}  // namespace
