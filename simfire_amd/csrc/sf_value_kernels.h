// Values at risk (sf_values_set): the pass the host enqueues BEHIND the arrival pass - neither the arrival
// kernels nor a step kernel know about it.  Part of simfire_hip.hip only (the run units do not include it).
//
// The invariant: damage[e] == the sum of value[e][y][x] over the cells whose arrival1 is not 0, in integers.  The arrival pass in
// front has just completed arrival1 up to the environment's update count t = commit[e].steps; the record of an environment says up to
// which update + 1 its arrivals have been summed (upto1, 0 = nothing yet), so this pass adds the cells with upto1 < arrival1 <= t + 1.
// A pass runs at least every max_fire_duration updates, so every such cell still holds a live sprite and its vector's bit is set in
// plane 0 of the vector bitmap (the argument of sf_arrival_kernels.h): the sparse form finds them all by walking the bitmap.
// Every workgroup of an environment READS upto1, so none of them writes it: k_value_commit does, one lane per environment, behind the
// sum.  The sums are integers added by atomics: the order does not matter, the result is exact.
// A frozen environment (EnvState.running == 0) keeps its update count: its window is empty after the first pass.  A record of zeros
// (what a reset leaves, what a recount starts from) makes the window "every arrival there is".
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sf_common.h"

namespace {

constexpr int32_t kValueMax = 1 << 24;       // |value| <= 2^24: 2^26 cells of it fit int64 with room, a tick's loss is exact in double

// The per-environment record: one 16-byte slice that a reset zeroes and a fork copies (value_seg in simfire_hip.hip).
struct ValueRec {
    long long damage;
    uint32_t upto1;          // arrivals summed up to this update + 1; 0 = nothing summed yet
    uint32_t pad;
};
static_assert(sizeof(ValueRec) == 16, "the record is one 16-byte slice");

struct ValueArgs {
    const int32_t *values;   // int32 [n][H][P], n = E (per_env) or 1; the pitch padding is zero
    long long values_env;    // H * P (per_env) or 0
    const uint32_t *arrival1;
    const EnvState *commit;
    ValueRec *rec;
};

__device__ __forceinline__ bool value_in(uint32_t a1, uint32_t lo, uint32_t hi) { return a1 > lo && a1 <= hi; }

// The sum of a wave's lanes onto damage[e]: at most one 64-bit vector atomic per wave, none where the wave found nothing.  Every
// lane of the wave gets here (no lane has returned), so the shuffles read defined values.
__device__ __forceinline__ void value_wave_add(long long sum, ValueRec *rec)
{
    if (__ballot(sum != 0) == 0ull) return;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
    if ((threadIdx.x & 63) == 0 && sum != 0) atomicAdd(reinterpret_cast<unsigned long long *>(&rec->damage), (unsigned long long)sum);
}

__device__ __forceinline__ long long value_quad(const uint4 &a, const int4 &v, uint32_t lo, uint32_t hi)
{
    long long s = 0;
    if (value_in(a.x, lo, hi)) s += v.x;
    if (value_in(a.y, lo, hi)) s += v.y;
    if (value_in(a.z, lo, hi)) s += v.z;
    if (value_in(a.w, lo, hi)) s += v.w;
    return s;
}

// Sparse form: k_arrival_bits' grid - one lane per word of plane 0 of the vector bitmap.  A lane walks the set bits of its word; of each
// vector it loads the 16 arrival1 words (64 contiguous bytes of the row-major plane) and, only where one of them falls in the window,
// the 16 values beside them.  The sprite masks are not looked at: the chain is word -> arrival -> value.
__global__ __launch_bounds__(256) void k_value_bits(Geo g, const unsigned long long *vbits, ValueArgs a)
{
    const int e = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;      // word of the environment: row i / VW, word i % VW of the row
    const bool mine = i < g.H * g.VW;
    unsigned long long word = mine ? vbits[(long long)e * g.vb_env + i] : 0ull;
    const uint32_t lo = a.rec[e].upto1, hi = (uint32_t)a.commit[e].steps + 1u;
    long long sum = 0;
    if (hi > lo && word) {
        const int y = i / g.VW, v0 = (i - y * g.VW) * 64;
        const long long row = (long long)y * g.P;
        const uint32_t *arow = a.arrival1 + (long long)e * g.plane_env + row;
        const int32_t *vrow = a.values + (long long)e * a.values_env + row;
        while (word) {
            const int v = v0 + __ffsll((long long)word) - 1;
            word &= word - 1ull;
            if (v >= g.PV) break;                              // (no bit beyond the row's vectors; the bound of every access below)
            const uint4 *ap = reinterpret_cast<const uint4 *>(arow + v * 16);
            const uint4 a0 = ap[0], a1 = ap[1], a2 = ap[2], a3 = ap[3];
            const uint32_t any = (uint32_t)value_in(a0.x, lo, hi) | value_in(a0.y, lo, hi) | value_in(a0.z, lo, hi) | value_in(a0.w, lo, hi) |
                                 value_in(a1.x, lo, hi) | value_in(a1.y, lo, hi) | value_in(a1.z, lo, hi) | value_in(a1.w, lo, hi) |
                                 value_in(a2.x, lo, hi) | value_in(a2.y, lo, hi) | value_in(a2.z, lo, hi) | value_in(a2.w, lo, hi) |
                                 value_in(a3.x, lo, hi) | value_in(a3.y, lo, hi) | value_in(a3.z, lo, hi) | value_in(a3.w, lo, hi);
            if (!any) continue;
            const int4 *vp = reinterpret_cast<const int4 *>(vrow + v * 16);
            sum += value_quad(a0, vp[0], lo, hi) + value_quad(a1, vp[1], lo, hi) + value_quad(a2, vp[2], lo, hi) + value_quad(a3, vp[3], lo, hi);
        }
    }
    value_wave_add(sum, a.rec + e);
}

// Dense form: one thread per cell, the same window and the same reduction.  Where the arrival pass is dense, when forced, and for
// every recount (records of zeros in front: the window is every arrival).
__global__ __launch_bounds__(256) void k_value_cells(Geo g, ValueArgs a)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, e = blockIdx.z;
    const uint32_t lo = a.rec[e].upto1, hi = (uint32_t)a.commit[e].steps + 1u;
    long long sum = 0;
    if (x < g.W && hi > lo) {
        const long long c = (long long)y * g.P + x;
        if (value_in(a.arrival1[(long long)e * g.plane_env + c], lo, hi)) sum = a.values[(long long)e * a.values_env + c];
    }
    value_wave_add(sum, a.rec + e);
}

// Behind the sum, one lane per environment: the arrivals up to the update count are summed.
__global__ void k_value_commit(int E, const EnvState *commit, ValueRec *rec)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < E) rec[e].upto1 = (uint32_t)commit[e].steps + 1u;
}

// sf_values_set with a device pointer: a plane handed over in device memory is range-checked here (|value| <= kValueMax), the
// verdict left in one word that the call reads back before the plane is taken.
__global__ void k_value_range(const int32_t *v, long long n, uint32_t *bad)
{
    bool out = false;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        out |= v[i] > kValueMax || v[i] < -kValueMax;
    if (out) atomicOr(bad, 1u);
}

}  // namespace
