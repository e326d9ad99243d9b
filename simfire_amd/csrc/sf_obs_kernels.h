// Observation tensors for a policy (sf_observe): fire_map, BurnStatus indicators, the attribute planes of
// get_attribute_data() normalised by get_attribute_bounds() and agent_positions (simfire/sim/simulation.py:317-403, 480-499), cropped and
// pooled, written in one launch as out[n][C][oh][ow] (float32 or bfloat16).
// Part of the single translation unit simfire_hip.hip.  Reads whichever cell plane is current and writes nothing but `out`.
#pragma once
#include "sf_common.h"

namespace {

constexpr int kObsThreads = 256;
constexpr int kObsLds = 24576;           // staged status bytes of one workgroup's source region (the host picks tiles that fit)
constexpr uint8_t kObsOff = 0xFF;        // staged byte of a cell off the grid (crop window, pitch padding): takes the value `pad`

// What sf_observe copies into device memory per call: the channel list and the normalisation bounds
struct ObsHead {
    int32_t code[SF_OBS_MAX_CHANNELS];   // SF_OBS_*
    int32_t mode[SF_OBS_MAX_CHANNELS];   // 0 mean, 1 max
    double lo[7], span[7];               // attribute a = code - SF_OBS_W_0: min and max - min (simulation.py:334-374)
};

struct ObsArgs {
    Geo g;
    CellPlanes pl;             // the status bytes, in whichever plane is current
    const double *lay;         // dense layers [tables][7][H * W]: w_0 delta M_x sigma elevation U U_dir
    long long lay_tab;         // doubles between two environments' tables (0: one shared table)
    const ObsHead *head;
    const int32_t *envs;       // [n]
    const int32_t *centers;    // [n][2] (column, row), or null = no crop
    const int32_t *agents;     // [n][k][3] (column, row, id), or null
    void *out;
    int n, C, f, ch, cw, oh, ow, k;
    int TX, TY, tiles_x, stride;   // output cells per workgroup (TX x TY), LDS bytes per staged source row
    int norm, bf16;
    double pad;
};

// float32 -> bfloat16 bits, round to nearest even (what torch's .to(torch.bfloat16) does for finite values)
__device__ __forceinline__ uint16_t obs_bf16(float v)
{
    const uint32_t u = __float_as_uint(v);
    if ((u & 0x7F800000u) == 0x7F800000u) return (uint16_t)((u >> 16) | ((u & 0xFFFFu) ? 0x40u : 0u));
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

// One workgroup: one listed environment, one tile of TX x TY output cells.  Its source region (TY * f rows of TX * f cells, shifted by the
// crop window) is staged into LDS as whole 16-cell vectors - one 16-byte load per vector from either plane, each status byte read once -,
// then every thread makes one output cell for all C channels, channel after channel (one f64 accumulator: no register arrays).  The
// workgroups of one tile are consecutive over the listed environments, so a shared table's attribute planes come out of L2 / MALL.
__global__ __launch_bounds__(kObsThreads) void k_observe(ObsArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t st[kObsLds];
    __shared__ int32_t s_code[SF_OBS_MAX_CHANNELS], s_mode[SF_OBS_MAX_CHANNELS];
    __shared__ double s_lo[7], s_span[7];
    __shared__ int32_t s_cell[SF_OBS_MAX_AGENTS], s_id[SF_OBS_MAX_AGENTS];
    const Geo &g = a.g;
    const int t = threadIdx.x;
    const int i = (int)(blockIdx.x % (unsigned)a.n);
    const int tile = (int)(blockIdx.x / (unsigned)a.n);
    const int ox0 = (tile % a.tiles_x) * a.TX, oy0 = (tile / a.tiles_x) * a.TY;
    const int e = a.envs[i];
    long long cx0 = 0, cy0 = 0;                     // source cell of output window (0, 0)
    if (a.centers) {
        cx0 = (long long)a.centers[2 * i] - a.cw / 2;
        cy0 = (long long)a.centers[2 * i + 1] - a.ch / 2;
    }
    const long long sxa = cx0 + (long long)ox0 * a.f, sya = cy0 + (long long)oy0 * a.f;   // the region's first source column / row
    const long long va = sxa >> 4;                  // its first vector (floor, also left of the grid)
    const int shift = (int)(sxa - va * 16);
    const int rows = a.TY * a.f, nvec = (shift + a.TX * a.f + 15) >> 4;

    if (t < a.C) { s_code[t] = a.head->code[t]; s_mode[t] = a.head->mode[t]; }
    if (t < 7) { s_lo[t] = a.head->lo[t]; s_span[t] = a.head->span[t]; }
    // agent_positions of update_agent_positions on a fresh map: entry j shows at its cell iff no later entry moves the same id and no
    // later entry writes the same cell (simulation.py:493-494); padding (id <= 0, off the grid) takes no part
    if (a.agents && t < a.k) {
        const int32_t *p = a.agents + ((long long)i * a.k + t) * 3;
        const int x = p[0], y = p[1], id = p[2];
        bool win = id > 0 && x >= 0 && x < g.W && y >= 0 && y < g.H;
        for (int m = t + 1; win && m < a.k; ++m) {
            const int32_t *q = a.agents + ((long long)i * a.k + m) * 3;
            const bool real = q[2] > 0 && q[0] >= 0 && q[0] < g.W && q[1] >= 0 && q[1] < g.H;
            if (real && (q[2] == id || (q[0] == x && q[1] == y))) win = false;
        }
        s_cell[t] = win ? y * g.W + x : -1;
        s_id[t] = id;
    }
    // stage the region's status bytes (& 7), kObsOff off the grid
    for (int idx = t; idx < rows * nvec; idx += kObsThreads) {
        const int r = idx / nvec, j = idx - r * nvec;
        const long long y = sya + r, v = va + j;
        uint4 q = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
        if (y >= 0 && y < g.H && v >= 0 && v < g.PV) {
            q = and4(*reinterpret_cast<const uint4 *>(cell_status_vec(a.pl, g, e, y, v)), 0x07070707u);
            const int in = g.W - (int)v * 16;        // cells of the vector on the grid (the rest is pitch padding)
            if (in < 16) {
                const uint32_t m0 = spread01(first01(in)), m1 = spread01(first01(in - 4)), m2 = spread01(first01(in - 8)),
                               m3 = spread01(first01(in - 12));
                q = make_uint4((q.x & m0) | ~m0, (q.y & m1) | ~m1, (q.z & m2) | ~m2, (q.w & m3) | ~m3);
            }
        }
        *reinterpret_cast<uint4 *>(st + r * a.stride + j * 16) = q;
    }
    __syncthreads();

    const int tx = t % a.TX, ty = t / a.TX;
    const int ox = ox0 + tx, oy = oy0 + ty;
    if (ty >= a.TY || ox >= a.ow || oy >= a.oh) return;
    const int f = a.f;
    const long long wx = sxa + (long long)tx * f, wy = sya + (long long)ty * f;      // the output cell's window in source cells
    const uint8_t *base = st + ty * f * a.stride + shift + tx * f;
    bool agents_here = false;
    if (a.agents)
        for (int m = 0; m < a.k; ++m) {
            const int c = s_cell[m];
            if (c >= 0) {
                const int y = c / g.W, x = c - y * g.W;
                agents_here |= y >= wy && y < wy + f && x >= wx && x < wx + f;
            }
        }
    const double *lay = a.lay + (long long)e * a.lay_tab;
    const long long plane = (long long)g.H * g.W;
    const long long o_plane = (long long)a.oh * a.ow;
    const long long o_cell = (long long)i * a.C * o_plane + (long long)oy * a.ow + ox;
#pragma unroll 1
    for (int c = 0; c < a.C; ++c) {
        const int code = s_code[c], mode = s_mode[c];
        const int at = code - SF_OBS_W_0;              // attribute 0..6 (w_0 sigma delta M_x elevation wind_speed wind_direction)
        const int li = at == 0 ? 0 : (at == 1 ? 3 : (at == 2 ? 1 : (at == 3 ? 2 : at)));       // its layer in lay
        const double *lp = lay + (long long)li * plane;
        const bool attr = at >= 0 && at < 7;
        const double lo = attr ? s_lo[at] : 0.0, span = attr ? s_span[at] : 1.0;
        double acc = 0.0;
#pragma unroll 1
        for (int dy = 0; dy < f; ++dy) {
            const uint8_t *row = base + dy * a.stride;
#pragma unroll 1
            for (int dx = 0; dx < f; ++dx) {
                const uint32_t s = row[dx];
                double v;
                if (s == kObsOff) v = a.pad;
                else if (code == SF_OBS_FIRE_MAP) v = (double)s;
                else if (code < SF_OBS_W_0) v = s == (uint32_t)(code - SF_OBS_BURN_STATUS) ? 1.0 : 0.0;
                else if (attr) {
                    const double raw = lp[(wy + dy) * g.W + wx + dx];
                    // the dtypes of get_attribute_data (simulation.py:397-403), as k_attribute_planes casts them
                    v = (at == 0 || at == 2 || at == 3) ? (double)(float)raw : (at == 1 ? (double)(uint32_t)raw : raw);
                    if (a.norm) v = (v - lo) / span;
                } else {                                   // SF_OBS_AGENTS
                    v = 0.0;
                    if (agents_here) {
                        const int cell = (int)(wy + dy) * g.W + (int)(wx + dx);
                        for (int m = 0; m < a.k; ++m)
                            if (s_cell[m] == cell) v = (double)s_id[m];
                    }
                }
                if (dy == 0 && dx == 0) acc = v;
                else if (mode) acc = v > acc ? v : acc;
                else acc = acc + v;
            }
        }
        if (!mode && f > 1) acc = acc / ((double)f * f);
        const float r = (float)acc;
        const long long o = o_cell + (long long)c * o_plane;
        if (a.bf16) static_cast<uint16_t *>(a.out)[o] = obs_bf16(r);
        else static_cast<float *>(a.out)[o] = r;
    }
}

}  // namespace
