// Distance fields (sf_distance): the exact squared Euclidean distance from every cell - or from a list of points -
// to the nearest cell whose BurnStatus a mask selects, in integers.  The reference has nothing of the kind.
// Separable form: k_dist_cols_down / k_dist_cols_up leave g[y][x], the vertical distance to the nearest selected cell of column x
// (u16, kDistNone = none in this column), in the library's scratch plane; k_dist_rows takes the lower envelope of r^2 + g[y][x +- r]^2
// along each row, k_dist_points the same minimum for single cells.  Part of the single translation unit simfire_hip.hip.  The status
// bytes are read from whichever cell plane is current; nothing but the scratch plane and `out` is written.
#pragma once
#include "sf_query_dev.h"

namespace {

constexpr int kDistNone = 65535;              // g: no selected cell in this column (H <= 65535: a real distance is 65534 at most)
constexpr int kDistColsThreads = 64;
constexpr int kDistDownAhead = 8;             // rows whose status vectors a lane of the pass down has in flight beside the ones it works on
constexpr int kDistUpAhead = 4;               // the same for the pass up (two 16-byte loads per row)
constexpr int kDistRowsThreads = 256;
constexpr int kDistMaxWidth = 8192;           // cells per row k_dist_rows stages (int32 in LDS: 32 KB); wider grids are refused
constexpr int kDistMaxRows = 64;              // rows of a narrow grid that share a k_dist_rows workgroup
constexpr long long kDistScratchDefault = 128ll << 20;     // bytes of scratch a call uses unless it names a budget

struct DistArgs {
    Geo g;
    CellPlanes pl;             // the status bytes, in whichever plane is current
    const int32_t *envs;       // the listed environments of this chunk [cn]
    uint16_t *gp;              // scratch: [cn][H][P]
    const int32_t *points;     // this chunk's [cn][k][3] (column, row, id), or null (plane form)
    void *out;                 // this chunk's part of the output: [cn][H][W] or [cn][k]
    int cn, k;
    uint32_t tlo, thi;         // the mask as the table of one byte permute (mask_sel01)
    int limit;                 // max_d2, or SF_DIST_FAR without a cap
    int reach;                 // columns either side of a point that can still lower its value: the smallest r with r^2 >= limit, W without a cap
    int f32, vec, rows;        // float output; 16-byte stores (W % 4 == 0 and an aligned output); rows per k_dist_rows workgroup
    double scale;
};

// 0/1 per byte of the 16 cells of vector v in row y: the cell is on the grid and its status is selected
__device__ __forceinline__ uint4 dist_sel01(const DistArgs &a, uint4 q, int v)
{
    // (the cells of the vector past the width are pitch padding: never a source)
    return and44(mask_sel01(a.tlo, a.thi, and4(q, 0x07070707u)), first01x16(a.g.W - v * 16));
}
__device__ __forceinline__ uint4 dist_vec(const DistArgs &a, int e, int y, int v)      // the 16 status bytes of vector v in row y
{
    return *reinterpret_cast<const uint4 *>(cell_status_vec(a.pl, a.g, e, y, v));
}
__device__ __forceinline__ int dist_next(int d) { return d + 1 < kDistNone ? d + 1 : kDistNone; }

// The pass down: one lane per (listed environment, 16-cell vector), row 0 to row H - 1; g = rows since the last selected cell of the
// column (kDistNone before the first).  The status loads do not depend on the running distances: those of the next kDistDownAhead rows
// are issued before the current ones are worked on (rows past the grid re-read row H - 1 and are not used).
__global__ __launch_bounds__(kDistColsThreads) void k_dist_cols_down(DistArgs a)
{
    const Geo &g = a.g;
    const long long tid = (long long)blockIdx.x * kDistColsThreads + threadIdx.x;
    if (tid >= (long long)a.cn * g.PV) return;
    const int i = (int)(tid / g.PV), v = (int)(tid - (long long)i * g.PV);
    const int e = a.envs[i];
    uint16_t *gp = a.gp + ((long long)i * g.H) * g.P + v * 16;
    int d[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) d[c] = kDistNone;
    uint4 cur[kDistDownAhead], nxt[kDistDownAhead];
#pragma unroll
    for (int j = 0; j < kDistDownAhead; ++j) cur[j] = dist_vec(a, e, min(j, g.H - 1), v);
    for (int y0 = 0; y0 < g.H; y0 += kDistDownAhead) {
#pragma unroll
        for (int j = 0; j < kDistDownAhead; ++j) nxt[j] = dist_vec(a, e, min(y0 + kDistDownAhead + j, g.H - 1), v);
#pragma unroll
        for (int j = 0; j < kDistDownAhead; ++j) {
            const int y = y0 + j;
            if (y < g.H) {
                const uint4 s = dist_sel01(a, cur[j], v);
                uint32_t w[8];
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    const uint32_t sel = (pick(s, c >> 2) >> (8 * (c & 3))) & 1u;
                    d[c] = sel ? 0 : dist_next(d[c]);
                    if (c & 1) w[c >> 1] |= (uint32_t)d[c] << 16;
                    else w[c >> 1] = (uint32_t)d[c];
                }
                uint4 *dst = reinterpret_cast<uint4 *>(gp + (long long)y * g.P);
                dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
                dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
            }
        }
#pragma unroll
        for (int j = 0; j < kDistDownAhead; ++j) cur[j] = nxt[j];
    }
}

// The pass up over what the pass down left (g == 0 marks a selected cell): g = min(g, rows to the next selected cell below).
// A vector whose values do not change is not written again.
__global__ __launch_bounds__(kDistColsThreads) void k_dist_cols_up(DistArgs a)
{
    const Geo &g = a.g;
    const long long tid = (long long)blockIdx.x * kDistColsThreads + threadIdx.x;
    if (tid >= (long long)a.cn * g.PV) return;
    const int i = (int)(tid / g.PV), v = (int)(tid - (long long)i * g.PV);
    uint16_t *gp = a.gp + ((long long)i * g.H) * g.P + v * 16;
    int u[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) u[c] = kDistNone;
    uint4 cur[kDistUpAhead][2], nxt[kDistUpAhead][2];
#pragma unroll
    for (int j = 0; j < kDistUpAhead; ++j) {
        const uint4 *src = reinterpret_cast<const uint4 *>(gp + (long long)max(g.H - 1 - j, 0) * g.P);
        cur[j][0] = src[0]; cur[j][1] = src[1];
    }
    for (int y0 = g.H - 1; y0 >= 0; y0 -= kDistUpAhead) {
#pragma unroll
        for (int j = 0; j < kDistUpAhead; ++j) {
            const uint4 *src = reinterpret_cast<const uint4 *>(gp + (long long)max(y0 - kDistUpAhead - j, 0) * g.P);
            nxt[j][0] = src[0]; nxt[j][1] = src[1];
        }
#pragma unroll
        for (int j = 0; j < kDistUpAhead; ++j) {
            const int y = y0 - j;
            if (y >= 0) {
                uint32_t w[8];
                uint32_t changed = 0;
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    const uint32_t word = pick(cur[j][c >> 3], (c >> 1) & 3);
                    const int gv = (int)((word >> (16 * (c & 1))) & 0xFFFFu);
                    u[c] = gv == 0 ? 0 : dist_next(u[c]);
                    const int o = u[c] < gv ? u[c] : gv;
                    changed |= (uint32_t)(o ^ gv);
                    if (c & 1) w[c >> 1] |= (uint32_t)o << 16;
                    else w[c >> 1] = (uint32_t)o;
                }
                if (changed) {
                    uint4 *dst = reinterpret_cast<uint4 *>(gp + (long long)y * g.P);
                    dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
                    dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kDistUpAhead; ++j) { cur[j][0] = nxt[j][0]; cur[j][1] = nxt[j][1]; }
    }
}

// The value as it is stored: the int32 itself, or the bits of (float)(sqrt((double)v) / scale) - IEEE sqrt and divide in double, one
// rounding to float32 (the library is built with -ffp-contract=off and no fast-math)
__device__ __forceinline__ int32_t dist_value(const DistArgs &a, int v)
{
    if (!a.f32) return v;
    return __float_as_int((float)(sqrt((double)v) / a.scale));
}

// One workgroup: a.rows rows of one listed environment.  g^2 of the rows is staged into LDS as int32 (kDistNone -> SF_DIST_FAR, never
// squared), with the first and last column of each row that holds a value (s_lo / s_hi).  Then one lane per cell: best = min(g2[x],
// limit), and for r = r0, r0 + 1, ... the minimum with r^2 + g2[x +- r] where that column lies in [lo, hi] and holds a value, until
// r^2 >= best or r passes the far end of [lo, hi]; r0 = the distance from x to [lo, hi] (nearer columns hold nothing), 1 inside it.
// 32-bit sums cannot overflow: r^2 + g2 <= (W - 1)^2 + (H - 1)^2 < 2^31 (the host refuses larger grids), and FAR is never added to.
__global__ __launch_bounds__(kDistRowsThreads) void k_dist_rows(DistArgs a)
{
    extern __shared__ __attribute__((aligned(16))) int32_t g2[];      // [a.rows][P]
    __shared__ int s_lo[kDistMaxRows], s_hi[kDistMaxRows];
    const Geo &g = a.g;
    const int t = threadIdx.x;
    const int i = blockIdx.y, y0 = blockIdx.x * a.rows;
    const int nr = min(a.rows, g.H - y0);
    if (t < nr) { s_lo[t] = 0x7FFFFFFF; s_hi[t] = -1; }
    __syncthreads();
    const int G8 = g.P >> 3;                       // groups of 8 cells (16 bytes of g) per row
    const uint16_t *gp = a.gp + ((long long)i * g.H + y0) * g.P;
    for (int idx = t; idx < nr * G8; idx += kDistRowsThreads) {
        const int r = idx / G8, j = idx - r * G8;
        const uint4 q = *reinterpret_cast<const uint4 *>(gp + (long long)r * g.P + j * 8);
        int32_t o[8];
        int lo = 0x7FFFFFFF, hi = -1;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int gv = (int)((pick(q, c >> 1) >> (16 * (c & 1))) & 0xFFFFu);
            o[c] = gv == kDistNone ? SF_DIST_FAR : gv * gv;
            if (gv != kDistNone) { lo = min(lo, j * 8 + c); hi = j * 8 + c; }
        }
        int4 *dst = reinterpret_cast<int4 *>(g2 + r * g.P + j * 8);
        dst[0] = make_int4(o[0], o[1], o[2], o[3]);
        dst[1] = make_int4(o[4], o[5], o[6], o[7]);
        if (hi >= 0) { atomicMin(&s_lo[r], lo); atomicMax(&s_hi[r], hi); }
    }
    __syncthreads();

    int32_t *out = static_cast<int32_t *>(a.out) + ((long long)i * g.H + y0) * g.W;
    const int cells = nr * g.P;
    for (int base = 0; base < cells; base += kDistRowsThreads) {          // (every lane makes every turn: the shuffles below need them all)
        const int idx = base + t;
        const int r = idx / g.P, x = idx - r * g.P;
        const bool on = idx < cells && x < g.W;
        int32_t val = 0;
        if (on) {
            const int32_t *row = g2 + r * g.P;
            int best = min(row[x], a.limit);
            const int lo = s_lo[r], hi = s_hi[r];
            if (lo <= hi) {
                const int rmax = max(x - lo, hi - x);
                for (int rr = x < lo ? lo - x : (x > hi ? x - hi : 1); rr <= rmax && rr * rr < best; ++rr) {
                    const int r2 = rr * rr;
                    if (x - rr >= lo) { const int v = row[x - rr]; if (v != SF_DIST_FAR) best = min(best, r2 + v); }
                    if (x + rr <= hi) { const int v = row[x + rr]; if (v != SF_DIST_FAR) best = min(best, r2 + v); }
                }
            }
            val = dist_value(a, best);
        }
        if (a.vec) {               // P and the workgroup size are multiples of 4: lane & 3 == x & 3, and a quad of cells lies in one row
            const int32_t v1 = __shfl_down(val, 1), v2 = __shfl_down(val, 2), v3 = __shfl_down(val, 3);
            if (on && (t & 3) == 0) *reinterpret_cast<int4 *>(out + (long long)r * g.W + x) = make_int4(val, v1, v2, v3);
        } else if (on) {
            out[(long long)r * g.W + x] = val;
        }
    }
}

// Point form: one wave per (listed environment, point).  Its lanes share the columns x - reach .. x + reach of row y of g and reduce
// min(limit, dx^2 + g^2) across the wave; an entry with id <= 0 or a cell off the grid gives -1 (-1.0f).
__global__ __launch_bounds__(kDistRowsThreads) void k_dist_points(DistArgs a)
{
    const Geo &g = a.g;
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.y, j = blockIdx.x * (kDistRowsThreads / 64) + (threadIdx.x >> 6);
    if (j >= a.k) return;                            // (wave-uniform)
    const QueryPoint p = query_point(a.points, (long long)i * a.k + j, g.W, g.H);
    const int x = p.x, y = p.y;
    int32_t val;
    if (!p.ok) {
        val = a.f32 ? __float_as_int(-1.0f) : -1;
    } else {
        const uint16_t *row = a.gp + ((long long)i * g.H + y) * g.P;
        const int xa = max(x - a.reach, 0), xb = min(x + a.reach, g.W - 1);
        int best = a.limit;
        for (int c = xa + lane; c <= xb; c += 64) {
            const int gv = row[c];
            if (gv != kDistNone) best = min(best, (c - x) * (c - x) + gv * gv);
        }
        best = wave_min(best);
        val = dist_value(a, best);
    }
    if (lane == 0) static_cast<int32_t *>(a.out)[(long long)i * a.k + j] = val;
}

}  // namespace
