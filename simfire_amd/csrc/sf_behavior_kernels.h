// Fire behaviour per cell (sf_behavior): heat per unit area, head rate of spread, Byram's fireline intensity and
// flame length from the R table the handle holds now, the planes, the "workable" mask, a per-environment summary and a per-point form.
// Part of the single translation unit simfire_hip.hip.  Reads whichever cell plane is current; writes nothing but its outputs and
// the heat cache.  Units are the reference's: feet, minutes, pounds, BTU.  Three kernels: k_behavior_hpa (the cache, once per
// terrain), k_behavior (a call that asks for a plane) and k_behavior_scan (a call that asks for the summary and / or points only).
//   I_R   float32, sfdev::cell_terms (rothermel.py:74-92); HPA = (float)((double)I_R * (384.0 / (double)sigma))   BTU/ft2
//   R     = max_k rt[k][c] (float64), head = the lowest k that attains it, -1 where all eight are 0
//   I_B   = (float)(((double)HPA * R) / 60.0)                                                                     BTU/ft/s
//   L     = (float)(0.45 * pow(I_B (f64), 0.46)); I_B and L are 0 where the float64 I_B is not > 0                  ft (Byram 1959)
// Compiled with -ffp-contract=off like the rest: the rounding sequence above is the specification.
#pragma once
#include "sf_query_dev.h"
#include "rothermel_dev.h"

namespace {

constexpr int kBehThreads = 256;

// The heat cache of tables t0 + z, z = blockIdx.z: float [tables][H * W], one value per cell - the only transcendentals of the
// feature, once per terrain.  An unburnable cell (w_0 <= 0) has I_R = 0 and HPA = 0 whatever its sigma.
__global__ __launch_bounds__(kBehThreads) void k_behavior_hpa(int H, int W, const double *lay, int t0, float h, float S_T, float S_e, float p_p,
                                                              float M_f, float *hpa)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const int t = t0 + (int)blockIdx.z;
    const long long n = (long long)H * W, i = (long long)y * W + x;
    const double *L = lay + (long long)t * 7 * n;
    const float sigma = (float)L[3 * n + i];
    const sfdev::CellTerms c = sfdev::cell_terms((float)L[i], (float)L[n + i], (float)L[2 * n + i], sigma, h, S_T, S_e, p_p, M_f, 0.0f, 0.0f,
                                                 0.0f, 0.0f);
    hpa[(long long)t * n + i] = c.burnable ? (float)((double)c.I_R * (384.0 / (double)sigma)) : 0.0f;
}

struct BehArgs {
    CellGeo g;
    CellPlanes pl;             // the status bytes, in whichever plane is current
    long long rt_env;          // Geo's: elements between two environments' tables (0: one shared table)
    const double *rt;          // [tables][8][H][P]
    const float *hpa;          // the heat cache [tables][H * W]
    long long hpa_env;         // floats between two environments' tables (0: one shared table)
    const int32_t *envs;       // [n]
    int n;
    uint32_t smask;            // bit s = BurnStatus s: the cells the planes show (0: every cell)
    uint32_t summask;          // the cells the summary and the point form look at
    float flame_limit;
    float edge[4];
    float *o_hpa, *o_ros, *o_int, *o_flame;      // [n][H][W] dense, or null
    int8_t *o_head;
    uint8_t *o_work;
    float *max_flame, *max_int;                  // [n], zeroed in front of the launch
    int32_t *classes;                            // [n][5], zeroed in front of the launch
    const int32_t *points;                       // [n][k][3] = (column, row, id)
    float *point_flame;                          // [n][k]
    int k;
    int planes, summary;       // some plane is asked for / some summary output is
    long long blocks_env;      // item blocks per listed environment: ceil(H * ceil(W / 4) / kBehThreads); k_behavior_scan: ceil(H * PV / kBehThreads)
    long long total;           // n * blocks_env (0 without planes and summary); the point form's items follow
};

struct BehCell {
    float ros, ib, L;
    int head;
};

// the four quantities of one cell from its eight rates and its heat per unit area
__device__ __forceinline__ BehCell beh_cell(const double (&r)[8], float hpa)
{
    double m = r[0];
    int h = 0;
    bool nz = r[0] != 0.0;
#pragma unroll
    for (int k = 1; k < 8; ++k) {
        nz = nz || r[k] != 0.0;
        if (r[k] > m) { m = r[k]; h = k; }       // (strictly greater: the lowest k keeps a tie)
    }
    BehCell b;
    b.head = nz ? h : -1;
    b.ros = (float)m;
    const double ib = ((double)hpa * m) / 60.0;
    const bool pos = ib > 0.0;                   // (I_R < 0 is a rounding artefact of eta_M at M_f >= M_x: such a cell does not burn)
    b.ib = pos ? (float)ib : 0.0f;
    b.L = pos ? (float)(0.45 * pow(ib, 0.46)) : 0.0f;
    return b;
}

// the quantities of cell (y, x) of environment e, loaded cell by cell (the point form and the scan: a few cells per lane at most)
__device__ __forceinline__ BehCell beh_cell_at(const BehArgs &a, int e, int y, int x)
{
    double r[8];
    const double *rp = a.rt + (long long)e * a.rt_env + (long long)y * a.g.P + x;
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = rp[(long long)k * a.g.plane_env];
    return beh_cell(r, a.hpa[(long long)e * a.hpa_env + (long long)y * a.g.W + x]);
}

// What the lanes of a workgroup found for listed environment i -> the outputs: a wave reduction where a wave has a selected cell,
// then the workgroup's LDS slots, then integer atomics (the maxima as bit patterns: the values are >= 0).  Two barriers: every
// thread of the workgroup calls it.
__device__ __forceinline__ void beh_reduce(const BehArgs &a, uint32_t *s_red, int i, int t, bool sel_any, uint32_t mf, uint32_t mi, uint32_t (&cls)[5])
{
    if (__any(sel_any)) {
        mf = wave_max(mf);
        mi = wave_max(mi);
#pragma unroll
        for (int q = 0; q < 5; ++q) cls[q] = wave_sum(cls[q]);
        if ((t & 63) == 0) {
            atomicMax(&s_red[0], mf);
            atomicMax(&s_red[1], mi);
#pragma unroll
            for (int q = 0; q < 5; ++q) if (cls[q]) atomicAdd(&s_red[2 + q], cls[q]);
        }
    }
    __syncthreads();
    if (t < 7) {
        const uint32_t v = s_red[t];
        if (v) {
            if (t == 0) { if (a.max_flame) atomicMax(reinterpret_cast<unsigned int *>(a.max_flame) + i, v); }
            else if (t == 1) { if (a.max_int) atomicMax(reinterpret_cast<unsigned int *>(a.max_int) + i, v); }
            else if (a.classes) atomicAdd(a.classes + (long long)i * 5 + (t - 2), (int)v);
            s_red[t] = 0u;
        }
    }
    __syncthreads();
}

// the point form: one lane per point
__device__ __forceinline__ void beh_points(const BehArgs &a, int t)
{
    if (!a.point_flame) return;
    const long long npts = (long long)a.n * a.k;
    for (long long w = blockIdx.x; w * kBehThreads < npts; w += gridDim.x) {
        const long long idx = w * kBehThreads + t;
        if (idx >= npts) continue;
        const int i = (int)(idx / a.k);
        const int e = a.envs[i];
        const QueryPoint p = query_point(a.points, idx, a.g.W, a.g.H);
        float best = -1.0f;
        if (p.ok) {
            best = 0.0f;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int y = p.y + dy, x = p.x + dx;
                    if (y < 0 || y >= a.g.H || x < 0 || x >= a.g.W) continue;
                    const uint32_t s = *cell_status(a.pl, a.g, e, y, x) & 7u;
                    if (!((a.summask >> s) & 1u)) continue;
                    const BehCell b = beh_cell_at(a, e, y, x);
                    best = b.L > best ? b.L : best;
                }
        }
        a.point_flame[idx] = best;
    }
}

// A grid-stride loop over (listed environment, block of kBehThreads items); an item is (row, group of 4 columns): per plane of the R
// table a lane reads 32 contiguous bytes and a wave 2 KiB of one row.  VEC (W % 4 == 0 and every output aligned for it): the heat
// cache is read and the planes are written 16 bytes (4 for the byte planes) at a time; else cell by cell, columns < W only.
// The summary goes through beh_reduce once per item block, the point form follows (beh_points).  Launched when a plane is asked for.
template <bool VEC>
__global__ __launch_bounds__(kBehThreads) void k_behavior(BehArgs a)
{
    __shared__ uint32_t s_red[8];      // 0: max flame bits, 1: max intensity bits, 2..6: class counts
    const CellGeo &g = a.g;
    const int t = threadIdx.x;
    const int gx = (g.W + 3) >> 2;
    const int items = g.H * gx;
    if (t < 8) s_red[t] = 0u;
    __syncthreads();
    for (long long w = blockIdx.x; w < a.total; w += gridDim.x) {
        const int i = (int)(w / a.blocks_env);
        const int item = (int)(w - (long long)i * a.blocks_env) * kBehThreads + t;
        const int e = a.envs[i];
        uint32_t mf = 0u, mi = 0u, cls[5] = {0u, 0u, 0u, 0u, 0u};
        bool sel_any = false;
        if (item < items) {
            const int y = item / gx, x = (item - y * gx) * 4;
            uint32_t sw = 0u;
            if (a.smask || a.summary) sw = *reinterpret_cast<const uint32_t *>(cell_status(a.pl, g, e, y, x)) & 0x07070707u;
            bool show[4], sel[4], need = false;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t s = (sw >> (8 * j)) & 7u;
                const bool in = x + j < g.W;
                show[j] = in && a.planes && (a.smask == 0u || ((a.smask >> s) & 1u));
                sel[j] = in && a.summary && ((a.summask >> s) & 1u);
                need = need || show[j] || sel[j];
                sel_any = sel_any || sel[j];
            }
            float o_hpa[4] = {0.f, 0.f, 0.f, 0.f}, o_ros[4] = {0.f, 0.f, 0.f, 0.f}, o_ib[4] = {0.f, 0.f, 0.f, 0.f}, o_L[4] = {0.f, 0.f, 0.f, 0.f};
            int o_head[4] = {-1, -1, -1, -1};
            if (need) {
                double r[4][8];
                const double *rp = a.rt + (long long)e * a.rt_env + (long long)y * g.P + x;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const double2 lo = *reinterpret_cast<const double2 *>(rp + (long long)k * g.plane_env);
                    const double2 hi = *reinterpret_cast<const double2 *>(rp + (long long)k * g.plane_env + 2);
                    r[0][k] = lo.x; r[1][k] = lo.y; r[2][k] = hi.x; r[3][k] = hi.y;
                }
                const float *hp = a.hpa + (long long)e * a.hpa_env + (long long)y * g.W + x;
                float hv[4] = {0.f, 0.f, 0.f, 0.f};
                if (VEC) {
                    const float4 q = *reinterpret_cast<const float4 *>(hp);
                    hv[0] = q.x; hv[1] = q.y; hv[2] = q.z; hv[3] = q.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) if (x + j < g.W) hv[j] = hp[j];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (!(show[j] || sel[j])) continue;
                    const BehCell b = beh_cell(r[j], hv[j]);
                    if (show[j]) { o_hpa[j] = hv[j]; o_ros[j] = b.ros; o_ib[j] = b.ib; o_L[j] = b.L; o_head[j] = b.head; }
                    if (sel[j]) {
                        const uint32_t lb = __float_as_uint(b.L), ib = __float_as_uint(b.ib);
                        mf = lb > mf ? lb : mf;
                        mi = ib > mi ? ib : mi;
                        const int c = (b.L >= a.edge[0]) + (b.L >= a.edge[1]) + (b.L >= a.edge[2]) + (b.L >= a.edge[3]);
#pragma unroll
                        for (int q = 0; q < 5; ++q) cls[q] += c == q ? 1u : 0u;
                    }
                }
            }
            if (a.planes) {
                const long long o = ((long long)i * g.H + y) * g.W + x;
                if (VEC) {
                    if (a.o_hpa) *reinterpret_cast<float4 *>(a.o_hpa + o) = make_float4(o_hpa[0], o_hpa[1], o_hpa[2], o_hpa[3]);
                    if (a.o_ros) *reinterpret_cast<float4 *>(a.o_ros + o) = make_float4(o_ros[0], o_ros[1], o_ros[2], o_ros[3]);
                    if (a.o_int) *reinterpret_cast<float4 *>(a.o_int + o) = make_float4(o_ib[0], o_ib[1], o_ib[2], o_ib[3]);
                    if (a.o_flame) *reinterpret_cast<float4 *>(a.o_flame + o) = make_float4(o_L[0], o_L[1], o_L[2], o_L[3]);
                    if (a.o_head)
                        *reinterpret_cast<uint32_t *>(a.o_head + o) = (uint32_t)(o_head[0] & 0xFF) | ((uint32_t)(o_head[1] & 0xFF) << 8) |
                                                                      ((uint32_t)(o_head[2] & 0xFF) << 16) | ((uint32_t)(o_head[3] & 0xFF) << 24);
                    if (a.o_work)
                        *reinterpret_cast<uint32_t *>(a.o_work + o) = (o_L[0] <= a.flame_limit ? 1u : 0u) | (o_L[1] <= a.flame_limit ? 0x100u : 0u) |
                                                                      (o_L[2] <= a.flame_limit ? 0x10000u : 0u) | (o_L[3] <= a.flame_limit ? 0x1000000u : 0u);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (x + j >= g.W) continue;
                        if (a.o_hpa) a.o_hpa[o + j] = o_hpa[j];
                        if (a.o_ros) a.o_ros[o + j] = o_ros[j];
                        if (a.o_int) a.o_int[o + j] = o_ib[j];
                        if (a.o_flame) a.o_flame[o + j] = o_L[j];
                        if (a.o_head) a.o_head[o + j] = (int8_t)o_head[j];
                        if (a.o_work) a.o_work[o + j] = o_L[j] <= a.flame_limit ? (uint8_t)1 : (uint8_t)0;
                    }
                }
            }
        }
        if (a.summary) beh_reduce(a, s_red, i, t, sel_any, mf, mi, cls);      // (uniform over the workgroup: its barriers are not divergent)
    }
    beh_points(a, t);
}

// The call without planes: the summary and / or the point form.  A grid-stride loop over (listed environment, block of kBehThreads
// items); an item is (row, 16-cell vector): one 16-byte load of status bytes from either layout, and only the cells summary_mask
// selects - a fire's front is a few cells in a thousand - go on to their eight rates and their heat, cell by cell.
__global__ __launch_bounds__(kBehThreads) void k_behavior_scan(BehArgs a)
{
    __shared__ uint32_t s_red[8];      // 0: max flame bits, 1: max intensity bits, 2..6: class counts
    const int t = threadIdx.x;
    const CellGeo &g = a.g;
    const int items = g.H * g.PV;
    if (t < 8) s_red[t] = 0u;
    __syncthreads();
    for (long long w = blockIdx.x; w < a.total; w += gridDim.x) {
        const int i = (int)(w / a.blocks_env);
        const int item = (int)(w - (long long)i * a.blocks_env) * kBehThreads + t;
        const int e = a.envs[i];
        uint32_t mf = 0u, mi = 0u, cls[5] = {0u, 0u, 0u, 0u, 0u};
        uint32_t m = 0u;               // bit j: cell x0 + j is on the grid and selected
        if (item < items) {
            const int y = item / g.PV, x0 = (item - y * g.PV) * 16;
            const uint4 q = and4(*reinterpret_cast<const uint4 *>(cell_status(a.pl, g, e, y, x0)), 0x07070707u);
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const uint32_t s = (pick(q, j >> 2) >> (8 * (j & 3))) & 7u;
                m |= (x0 + j < g.W && ((a.summask >> s) & 1u)) ? 1u << j : 0u;
            }
            for (uint32_t left = m; left; left &= left - 1u) {
                const BehCell b = beh_cell_at(a, e, y, x0 + __ffs((int)left) - 1);
                const uint32_t lb = __float_as_uint(b.L), ib = __float_as_uint(b.ib);
                mf = lb > mf ? lb : mf;
                mi = ib > mi ? ib : mi;
                const int c = (b.L >= a.edge[0]) + (b.L >= a.edge[1]) + (b.L >= a.edge[2]) + (b.L >= a.edge[3]);
#pragma unroll
                for (int k = 0; k < 5; ++k) cls[k] += c == k ? 1u : 0u;
            }
        }
        beh_reduce(a, s_red, i, t, m != 0u, mf, mi, cls);
    }
    beh_points(a, t);
}

}  // namespace
