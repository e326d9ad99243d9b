// Ensemble statistics (sf_ensemble_stats): per-cell statistics over GROUPS of environments, read off the arrival
// plane (sf_arrival_kernels.h keeps it) and, for the loss, the value plane (sf_value_kernels.h).  Part of simfire_hip.hip only; the
// step kernels, the enqueue layer and the two passes do not know about it, and it writes nothing but the caller's outputs.
//
// One kernel, a streaming reduction over the member axis: a lane owns 4 consecutive cells of a row (one quad) and walks the group's
// member list, one 16-byte load of arrival1 per member - a wave reads 1 KB of contiguous plane per instruction.  (row, quad) is
// flattened into the thread index, so narrow grids launch no mostly-empty workgroups; the group is blockIdx.y (+ 32768 * blockIdx.z:
// G may be 2^20).  The member index is uniform over the workgroup (a scalar load).  The loop is unrolled by 4 with the four loads in
// front of their use (a lone dependent load per iteration would be latency-bound); K % 4 members run in a tail.
// With a1 the raw word (update + 1, 0 = never) and u = a1 - 1u, "reached by horizon h" is u <= (uint32_t)h: a1 == 0 wraps to 0xFFFFFFFF
// and fails for every horizon, "no limit" is 0xFFFFFFFE.  T is padded to TP = 1, 2, 4, 8 by repeating the last horizon, so the last
// counter is always n, the number of members behind `first` and `mean`.
// Lanes beyond the grid (and the cells x >= W of the last quad) load a cell that exists, count whatever it holds and store nothing;
// only the loss, which leaves the lane, masks them - there by zeroing the VALUE, not the arrival.  No lane returns before the wave
// reduction of the loss.  All results are integers or floats defined from integers: no order of evaluation shows in any bit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sf_common.h"

namespace {

constexpr int kEnsGroupsY = 32768;           // groups per blockIdx.z

struct EnsArgs {
    const uint32_t *arrival1;                // u32 [E][H][P]
    long long plane_env;                     // H * P
    int H, W, P, Q;                          // Q = ceil(W / 4): quads per row
    const int32_t *members;                  // i32 [G][K], device
    int G, K, T;                             // T: horizons asked for (the outputs' extent), <= TP
    uint32_t hz[8];                          // the horizons as bounds of u, padded with the last
    const int32_t *values;                   // the handle's value plane (pitch P, zeros in the padding) or null
    long long values_env;                    // H * P (a plane per environment) or 0 (one for all)
    int vec;                                 // 1: W % 4 == 0 and every output is 16-byte aligned - quad stores
    int32_t *count; float *prob; int32_t *first; float *mean;
    unsigned long long *loss;                // i64 [G][T], zeroed on the stream in front of the launch
};

template <int TP>
struct EnsAcc {
    uint32_t cnt[TP][4];                     // members that reached the cell by horizon t; cnt[TP - 1] is n
    uint32_t mn[4];                          // smallest u among the n
    unsigned long long sum[4];               // sum of u over the n
};

template <int TP>
__device__ __forceinline__ void ens_take(EnsAcc<TP> &c, const uint32_t (&hz)[TP], const uint4 &v, bool moments)
{
    const uint32_t u[4] = {v.x - 1u, v.y - 1u, v.z - 1u, v.w - 1u};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int t = 0; t < TP; ++t) c.cnt[t][j] += u[j] <= hz[t] ? 1u : 0u;
        if (moments) {
            const bool in = u[j] <= hz[TP - 1];
            c.mn[j] = in && u[j] < c.mn[j] ? u[j] : c.mn[j];
            c.sum[j] += in ? u[j] : 0u;
        }
    }
}

// The loss under a plane per environment: the member's own values, added where ITS fire reached the cell.
template <int TP>
__device__ __forceinline__ void ens_lose(long long (&ls)[TP], const uint32_t (&hz)[TP], const uint4 &v, const int4 &w, const bool (&live)[4])
{
    const uint32_t u[4] = {v.x - 1u, v.y - 1u, v.z - 1u, v.w - 1u};
    const int32_t x[4] = {live[0] ? w.x : 0, live[1] ? w.y : 0, live[2] ? w.z : 0, live[3] ? w.w : 0};
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int t = 0; t < TP; ++t) ls[t] += u[j] <= hz[t] ? x[j] : 0;
}

template <int TP, bool LOSS>
__global__ __launch_bounds__(256) void k_ensemble(EnsArgs a)
{
    const int g = (int)blockIdx.z * kEnsGroupsY + (int)blockIdx.y;
    if (g >= a.G) return;                                      // (the whole workgroup: nobody is left waiting in a shuffle)
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool mine = i < (long long)a.H * a.Q;
    const int y = mine ? (int)(i / a.Q) : 0, x0 = mine ? (int)(i - (long long)y * a.Q) * 4 : 0;
    const long long off = (long long)y * a.P + x0;             // 16-byte aligned: P is a multiple of 16, x0 of 4, and x0 + 3 < P
    const bool live[4] = {mine && x0 < a.W, mine && x0 + 1 < a.W, mine && x0 + 2 < a.W, mine && x0 + 3 < a.W};
    const int32_t *__restrict__ mem = a.members + (long long)g * a.K;
    const bool moments = a.first != nullptr || a.mean != nullptr;
    const bool own = LOSS && a.values_env != 0;                // a plane per environment: the loss is summed member by member
    uint32_t hz[TP];
#pragma unroll
    for (int t = 0; t < TP; ++t) hz[t] = a.hz[t];

    EnsAcc<TP> c;
    long long ls[TP];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int t = 0; t < TP; ++t) c.cnt[t][j] = 0u;
        c.mn[j] = 0xFFFFFFFFu;
        c.sum[j] = 0ull;
    }
#pragma unroll
    for (int t = 0; t < TP; ++t) ls[t] = 0;

    auto cells = [&](int e) { return *reinterpret_cast<const uint4 *>(a.arrival1 + (long long)e * a.plane_env + off); };
    auto worth = [&](int e) { return *reinterpret_cast<const int4 *>(a.values + (long long)e * a.values_env + off); };
    int k = 0;
    for (; k + 4 <= a.K; k += 4) {
        const int e0 = mem[k], e1 = mem[k + 1], e2 = mem[k + 2], e3 = mem[k + 3];
        const uint4 v0 = cells(e0), v1 = cells(e1), v2 = cells(e2), v3 = cells(e3);
        if (own) {
            const int4 w0 = worth(e0), w1 = worth(e1), w2 = worth(e2), w3 = worth(e3);
            ens_lose<TP>(ls, hz, v0, w0, live); ens_lose<TP>(ls, hz, v1, w1, live);
            ens_lose<TP>(ls, hz, v2, w2, live); ens_lose<TP>(ls, hz, v3, w3, live);
        }
        ens_take<TP>(c, hz, v0, moments); ens_take<TP>(c, hz, v1, moments);
        ens_take<TP>(c, hz, v2, moments); ens_take<TP>(c, hz, v3, moments);
    }
    for (; k < a.K; ++k) {
        const int e = mem[k];
        const uint4 v = cells(e);
        if (own) ens_lose<TP>(ls, hz, v, worth(e), live);
        ens_take<TP>(c, hz, v, moments);
    }

    if (LOSS) {
        if (!own) {                                            // one plane for all: the cell's value times the members that reached it
            const int4 w = worth(0);
            const int32_t x[4] = {live[0] ? w.x : 0, live[1] ? w.y : 0, live[2] ? w.z : 0, live[3] ? w.w : 0};
#pragma unroll
            for (int t = 0; t < TP; ++t)
#pragma unroll
                for (int j = 0; j < 4; ++j) ls[t] += (long long)x[j] * (long long)c.cnt[t][j];
        }
#pragma unroll
        for (int t = 0; t < TP; ++t) {                         // every lane of the wave is here: the shuffles read defined values
            long long s = ls[t];
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) s += __shfl_down(s, d, 64);
            if ((threadIdx.x & 63) == 0 && t < a.T && s != 0) atomicAdd(a.loss + (long long)g * a.T + t, (unsigned long long)s);
        }
    }
    if (!mine) return;

    const float fk = (float)a.K;
    const long long row = (long long)y * a.W + x0, plane = (long long)a.H * a.W;
    if (a.count || a.prob) {
#pragma unroll
        for (int t = 0; t < TP; ++t) {
            if (t >= a.T) break;
            const long long o = ((long long)g * a.T + t) * plane + row;
            const float p[4] = {__fdiv_rn((float)c.cnt[t][0], fk), __fdiv_rn((float)c.cnt[t][1], fk), __fdiv_rn((float)c.cnt[t][2], fk),
                                __fdiv_rn((float)c.cnt[t][3], fk)};
            if (a.vec) {
                if (a.count) *reinterpret_cast<int4 *>(a.count + o) = make_int4((int)c.cnt[t][0], (int)c.cnt[t][1], (int)c.cnt[t][2], (int)c.cnt[t][3]);
                if (a.prob) *reinterpret_cast<float4 *>(a.prob + o) = make_float4(p[0], p[1], p[2], p[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (a.count && live[j]) a.count[o + j] = (int)c.cnt[t][j];
                    if (a.prob && live[j]) a.prob[o + j] = p[j];
                }
            }
        }
    }
    if (moments) {
        const long long o = (long long)g * plane + row;
        int32_t f[4];
        float m[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t n = c.cnt[TP - 1][j];
            f[j] = n ? (int32_t)c.mn[j] : -1;
            m[j] = n ? (float)((double)c.sum[j] / (double)n) : -1.0f;
        }
        if (a.vec) {
            if (a.first) *reinterpret_cast<int4 *>(a.first + o) = make_int4(f[0], f[1], f[2], f[3]);
            if (a.mean) *reinterpret_cast<float4 *>(a.mean + o) = make_float4(m[0], m[1], m[2], m[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (a.first && live[j]) a.first[o + j] = f[j];
                if (a.mean && live[j]) a.mean[o + j] = m[j];
            }
        }
    }
}

}  // namespace
