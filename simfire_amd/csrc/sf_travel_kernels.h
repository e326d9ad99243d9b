// Fire travel time (sf_travel): the minimum time, in minutes, at which fire starting on the source cells now gets
// to every cell over the R table the handle holds - Finney's minimum travel time on the graph of the automaton: cell c is entered from
// its neighbour c + SRC_OFFSETS[k] at the cost w_k(c) = float32(pixel_scale / rt[k][c]) (+inf where rt[k][c] is not > 0).  A FORECAST in
// continuous time, not the automaton: no whole updates, no burn-out of sources.  The reference has nothing of the kind.
//   T = 0 on sources; T(c) = min_k float32(T(n_k) + w_k(c)) on passable cells over the on-grid neighbours that are source or passable.
// float32 addition is monotone and the weights are >= 0, so the greatest solution is unique and ANY order of relaxations reaches it:
// nothing below depends on scheduling.
// k_travel: ONE workgroup per listed environment, resident until that environment's search ends - no workgroup waits for another.
// The working array T (float32 [H][W] dense: 0 sources, +inf passable, -1 neither) lives in the caller's minutes plane or in the
// handle's scratch.  The grid is cut into tiles of 32 x 32 cells, a thread per cell; a bitmap in LDS says which tiles are ACTIVE (at
// the start those that hold a source or a neighbour of one).  One activation: the tile and a halo of one cell to LDS, the eight weights of every open cell
// to registers (eight float64 divisions), chaotic relaxation in LDS - a sweep is 8 LDS reads, 8 adds and one barrier-or; a lane may
// read a neighbour's old or new value, both are upper bounds - until a sweep changes nothing, the changed cells back to T, and the
// bit of every neighbouring tile whose facing border (corner) cell fell.  The workgroup scans the bitmap in rounds until it is empty;
// values only fall, over a finite set of floats.  max_minutes = M drops every candidate above M, so every value <= M stays exact.
// The final passes (same kernel): over the tiles that were ever active pred, reached and last; the points, a lane each; M in place of
// +inf in the minutes plane.
// Part of the single translation unit simfire_hip.hip.  The status bytes are read from whichever cell plane is current; nothing but
// the scratch and the outputs is written.  Compiled with -ffp-contract=off like the rest: every sum is one float32 addition.
#pragma once
#include "sf_query_dev.h"

namespace {

constexpr int kTravelThreads = 1024;
constexpr int kTravelTile = 32;                       // cells per tile edge: kTravelTile * kTravelTile = kTravelThreads, a thread per cell
constexpr int kTravelPitch = kTravelTile + 2;         // the tile and its halo in LDS
constexpr int kTravelMaxWidth = 8192;                 // wider grids are refused (as the other searches do)
constexpr int kTravelMaxTiles = 131072;               // two bitmaps of that many bits: 32 KiB of LDS
constexpr long long kTravelScratchDefault = 1ll << 30;
static_assert(kTravelTile * kTravelTile == kTravelThreads, "k_travel: a thread per cell of a tile");

struct TravelArgs {
    Geo g;
    CellPlanes pl;               // the status bytes, in whichever plane is current
    const double *rt;            // [tables][8][H][P]; g.rt_env elements between two environments' tables (0: one shared table)
    const int32_t *envs;         // the listed environments of this chunk
    const uint8_t *sources;      // dense u8 [H * W] (src_env = 0) or [E][H * W], or null
    const uint8_t *passable;     // the same forms, or null
    long long src_env, pass_env;
    const int32_t *points;       // this chunk's [cn][k][3] = (column, row, id), or null
    int k;
    uint32_t smask, tmask;       // bit s = BurnStatus s: source_mask / through_mask
    int conn8;
    float cap;                   // max_minutes, +inf without a cap
    float *work;                 // this chunk's working arrays: the minutes plane or the scratch
    long long work_env;          // floats between two listed environments' arrays
    int work_vec;                // 16-byte stores of the staging (W % 4 == 0 and an aligned array)
    int fix_cap;                 // the working array is the minutes plane and there is a cap: +inf becomes the cap at the end
    int pred_vec;                // 4-byte stores of pred's pre-fill (W % 4 == 0 and an aligned plane)
    int8_t *pred;                // this chunk's part of the outputs (null: not asked for)
    float *point_minutes, *last;
    int32_t *reached, *activations;
};

// bytes of scratch per listed environment: the working array
__host__ __device__ inline long long travel_env_bytes(const Geo &g) { return ((long long)g.H * g.W * 4 + 255) / 256 * 256; }

// 2: source, 1: passable (and not a source), 0: neither - cell (y, x) on the grid with the status byte s
__device__ __forceinline__ int travel_class(const TravelArgs &a, int e, int y, int x, uint32_t s)
{
    const long long c = (long long)y * a.g.W + x;
    s &= 7u;
    if (((a.smask >> s) & 1u) || (a.sources && a.sources[a.src_env * e + c] != 0)) return 2;
    if (((a.tmask >> s) & 1u) && (!a.passable || a.passable[a.pass_env * e + c] != 0)) return 1;
    return 0;
}

__device__ __forceinline__ bool travel_diagonal(int k) { return k == 0 || k == 2 || k == 5 || k == 7; }

// w_k of the cell whose plane-0 entry of the table is at rp: the time fire from the neighbour c + SRC_OFFSETS[k] needs to cross it
__device__ __forceinline__ float travel_w(const TravelArgs &a, const double *rp, int k)
{
    if (!a.conn8 && travel_diagonal(k)) return __builtin_inff();
    const double r = rp[(long long)k * a.g.plane_env];
    return r > 0.0 ? (float)(a.g.pixel_scale / r) : __builtin_inff();
}

__device__ __forceinline__ const double *travel_rt(const TravelArgs &a, int e, int y, int x)
{
    return a.rt + (long long)e * a.g.rt_env + (long long)y * a.g.P + x;
}

// The tile whose first cell is (y0, x0) and its halo from the working array to LDS: cells that are neither source nor passable and
// cells past the grid read +inf there.  Returns the thread's own value as the array holds it (-1 past the grid).
__device__ __forceinline__ float travel_load(const TravelArgs &a, const float *T, float *s_T, int y0, int x0, int t, bool &in)
{
    const Geo &g = a.g;
    const int ly = t >> 5, lx = t & 31, y = y0 + ly, x = x0 + lx;
    in = y < g.H && x < g.W;
    float v = -1.0f;
    if (in) v = T[(long long)y * g.W + x];
    s_T[(ly + 1) * kTravelPitch + lx + 1] = v >= 0.0f ? v : __builtin_inff();
    if (t < 4 * kTravelTile + 4) {
        int hy, hx;
        if (t < kTravelPitch) { hy = 0; hx = t; }
        else if (t < 2 * kTravelPitch) { hy = kTravelPitch - 1; hx = t - kTravelPitch; }
        else if (t < 2 * kTravelPitch + kTravelTile) { hy = t - 2 * kTravelPitch + 1; hx = 0; }
        else { hy = t - 2 * kTravelPitch - kTravelTile + 1; hx = kTravelPitch - 1; }
        const int yy = y0 + hy - 1, xx = x0 + hx - 1;
        float hv = -1.0f;
        if (yy >= 0 && yy < g.H && xx >= 0 && xx < g.W) hv = T[(long long)yy * g.W + xx];
        s_T[hy * kTravelPitch + hx] = hv >= 0.0f ? hv : __builtin_inff();
    }
    return v;
}

// the value of neighbour k (SRC_OFFSETS order: c_dx / c_dy) of the thread's cell in the LDS tile; own = its own index
__device__ __forceinline__ float travel_nb(const float *s_T, int own, int k)
{
    constexpr int dx[8] = {+1, 0, -1, +1, -1, +1, 0, -1}, dy[8] = {+1, +1, +1, 0, 0, -1, -1, -1};
    return s_T[own + dy[k] * kTravelPitch + dx[k]];
}

__global__ __launch_bounds__(kTravelThreads) void k_travel(TravelArgs a)
{
    extern __shared__ uint32_t s_bits[];                  // [2][words]: the active tiles, the tiles that were ever active
    __shared__ float s_T[kTravelPitch * kTravelPitch];
    __shared__ uint32_t s_sum[2];                         // reached, the bits of last
    const Geo &g = a.g;
    const int t = threadIdx.x, nt = kTravelThreads;
    const int i = blockIdx.x, e = a.envs[i];
    const int H = g.H, W = g.W;
    const int TXn = (W + kTravelTile - 1) / kTravelTile, TYn = (H + kTravelTile - 1) / kTravelTile, words = (TXn * TYn + 31) >> 5;
    uint32_t *s_act = s_bits, *s_seen = s_bits + words;
    float *T = a.work + (long long)i * a.work_env;
    int8_t *pred = a.pred ? a.pred + (long long)i * H * W : nullptr;
    const float cap = a.cap, inf = __builtin_inff();
    for (int w = t; w < 2 * words; w += nt) s_bits[w] = 0u;
    if (t < 2) s_sum[t] = 0u;
    __syncthreads();

    // staging, four cells per turn: the working array (0 sources, +inf passable, -1 neither), pred's pre-fill, the first active tiles
    const int G4 = (W + 3) / 4;
#pragma unroll 1
    for (int idx = t; idx < H * G4; idx += nt) {
        const int y = idx / G4, x0 = (idx - y * G4) * 4;
        const uint32_t sw = *reinterpret_cast<const uint32_t *>(cell_status(a.pl, a.g, e, y, x0));
        const int in = min(4, W - x0);
        float v[4] = {-1.0f, -1.0f, -1.0f, -1.0f};
        bool src = false;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (c >= in) continue;
            const int cls = travel_class(a, e, y, x0 + c, sw >> (8 * c));
            v[c] = cls == 2 ? 0.0f : (cls == 1 ? inf : -1.0f);
            src = src || cls == 2;
            // a source on the border of its tile: the tiles beyond hold neighbours of it, and no changed value will ever wake them
            const int sx = (x0 + c) % kTravelTile, sy = y % kTravelTile;
            if (cls == 2 && (sx == 0 || sx == kTravelTile - 1 || sy == 0 || sy == kTravelTile - 1)) {
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int ny = y + dy, nx = x0 + c + dx;
                        if (ny < 0 || ny >= H || nx < 0 || nx >= W) continue;
                        const int tile = (ny / kTravelTile) * TXn + nx / kTravelTile;
                        atomicOr(&s_act[tile >> 5], 1u << (tile & 31));
                    }
            }
        }
        float *dst = T + (long long)y * W + x0;
        if (a.work_vec) {
            *reinterpret_cast<float4 *>(dst) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) if (c < in) dst[c] = v[c];
        }
        if (pred) {
            int8_t *pd = pred + (long long)y * W + x0;
            if (a.pred_vec) *reinterpret_cast<uint32_t *>(pd) = 0xFFFFFFFFu;
            else {
#pragma unroll
                for (int c = 0; c < 4; ++c) if (c < in) pd[c] = (int8_t)-1;
            }
        }
        if (src) {
            const int tile = (y / kTravelTile) * TXn + x0 / kTravelTile;
            atomicOr(&s_act[tile >> 5], 1u << (tile & 31));
        }
    }

    // the search: rounds over the bitmap until a round finds no active tile
    const int ly = t >> 5, lx = t & 31, own = (ly + 1) * kTravelPitch + lx + 1;
    int acts = 0;
    for (;;) {
        bool found = false;
#pragma unroll 1
        for (int w = 0; w < words; ++w) {
            for (;;) {
                __syncthreads();                  // the tile before is done: its values are in T, its neighbours' bits set
                const uint32_t bits = s_act[w];
                if (!bits) break;
                const int b = __ffs((int)bits) - 1;
                __syncthreads();                  // every thread has read the word
                if (t == 0) { s_act[w] = bits & ~(1u << b); s_seen[w] |= 1u << b; }
                found = true;
                ++acts;
                const int tile = w * 32 + b, ty = tile / TXn, tx = tile - ty * TXn;
                const int y = ty * kTravelTile + ly, x = tx * kTravelTile + lx;
                bool in;
                float cur = travel_load(a, T, s_T, ty * kTravelTile, tx * kTravelTile, t, in);
                const bool open = in && cur > 0.0f;           // (a source stays 0; +inf is open)
                float wk[8];
                if (open) {
                    const double *rp = travel_rt(a, e, y, x);
#pragma unroll
                    for (int k = 0; k < 8; ++k) wk[k] = travel_w(a, rp, k);
                } else {
#pragma unroll
                    for (int k = 0; k < 8; ++k) wk[k] = inf;
                }
                bool dirty = false;
                __syncthreads();
                for (;;) {
                    bool ch = false;
                    if (open) {
                        float best = cur;
#pragma unroll
                        for (int k = 0; k < 8; ++k) {
                            const float c = travel_nb(s_T, own, k) + wk[k];
                            if (c < best && c <= cap) best = c;
                        }
                        if (best < cur) { cur = best; s_T[own] = best; ch = true; dirty = true; }
                    }
                    if (!__syncthreads_or(ch)) break;
                }
                if (dirty) {
                    T[(long long)y * W + x] = cur;
                    const bool L = lx == 0 && tx > 0, R = lx == kTravelTile - 1 && tx + 1 < TXn;
                    const bool U = ly == 0 && ty > 0, D = ly == kTravelTile - 1 && ty + 1 < TYn;
                    auto wake = [&](int n) { atomicOr(&s_act[n >> 5], 1u << (n & 31)); };
                    if (L) wake(tile - 1);
                    if (R) wake(tile + 1);
                    if (U) wake(tile - TXn);
                    if (D) wake(tile + TXn);
                    if (a.conn8) {
                        if (U && L) wake(tile - TXn - 1);
                        if (U && R) wake(tile - TXn + 1);
                        if (D && L) wake(tile + TXn - 1);
                        if (D && R) wake(tile + TXn + 1);
                    }
                }
            }
        }
        if (!found) break;
    }

    // pred, reached, last: over the tiles that were ever active (no other tile holds a finite value).  A cell counts when it is
    // passable, not a source and has a finite value - which is within the cap, nothing above it was ever stored.
    if (pred || a.reached || a.last) {
        uint32_t cnt = 0u, mx = 0u;
#pragma unroll 1
        for (int w = 0; w < words; ++w) {
            uint32_t bits = s_seen[w];
            while (bits) {
                const int b = __ffs((int)bits) - 1;
                bits &= bits - 1u;
                const int tile = w * 32 + b, ty = tile / TXn, tx = tile - ty * TXn;
                const int y = ty * kTravelTile + ly, x = tx * kTravelTile + lx;
                __syncthreads();
                bool in;
                const float v = travel_load(a, T, s_T, ty * kTravelTile, tx * kTravelTile, t, in);
                __syncthreads();
                bool cand = in && v >= 0.0f && v < inf;
                if (cand && v == 0.0f) cand = travel_class(a, e, y, x, *cell_status(a.pl, a.g, e, y, x)) == 1;      // (a weight that rounds to 0)
                if (cand) {
                    ++cnt;
                    mx = max(mx, __float_as_uint(v));
                    if (pred) {
                        const double *rp = travel_rt(a, e, y, x);
                        int p = -1;
#pragma unroll
                        for (int k = 7; k >= 0; --k)
                            if (travel_nb(s_T, own, k) + travel_w(a, rp, k) == v) p = k;
                        pred[(long long)y * W + x] = (int8_t)p;
                    }
                }
            }
        }
        cnt = wave_sum(cnt); mx = wave_max(mx);
        if ((t & 63) == 0 && cnt) { atomicAdd(&s_sum[0], cnt); atomicMax(&s_sum[1], mx); }      // (the values are >= 0: their bits order as they do)
    }

    // the points: lane t answers point t.  On a cell that is neither source nor passable: the time at which it would be reached
    if (t < a.k && a.point_minutes) {
        const QueryPoint p = query_point(a.points, (long long)i * a.k + t, W, H);
        const int px = p.x, py = p.y;
        float r = -1.0f;
        if (p.ok) {
            float v = T[(long long)py * W + px];
            if (v < 0.0f) {
                const double *rp = travel_rt(a, e, py, px);
                v = inf;
                for (int k = 0; k < 8; ++k) {
                    const int nx = px + c_dx[k], ny = py + c_dy[k];
                    if (nx < 0 || nx >= W || ny < 0 || ny >= H) continue;
                    const float tn = T[(long long)ny * W + nx];
                    if (tn < 0.0f) continue;
                    const float c = tn + travel_w(a, rp, k);
                    if (c < v) v = c;
                }
            }
            r = v <= cap ? v : cap;
        }
        a.point_minutes[(long long)i * a.k + t] = r;
    }
    __syncthreads();

    // the minutes plane under a cap: what no route reaches within it shows the cap
    if (a.fix_cap) {
#pragma unroll 1
        for (int idx = t; idx < H * G4; idx += nt) {
            const int y = idx / G4, x0 = (idx - y * G4) * 4;
            float *dst = T + (long long)y * W + x0;
            if (a.work_vec) {
                float4 q = *reinterpret_cast<float4 *>(dst);
                if (q.x == inf || q.y == inf || q.z == inf || q.w == inf)
                    *reinterpret_cast<float4 *>(dst) = make_float4(q.x == inf ? cap : q.x, q.y == inf ? cap : q.y, q.z == inf ? cap : q.z, q.w == inf ? cap : q.w);
            } else {
                const int in = min(4, W - x0);
                for (int c = 0; c < in; ++c) if (dst[c] == inf) dst[c] = cap;
            }
        }
    }
    if (t == 0) {
        if (a.reached) a.reached[i] = (int32_t)s_sum[0];
        if (a.last) a.last[i] = __uint_as_float(s_sum[1]);
        if (a.activations) a.activations[i] = acts;
    }
}

}  // namespace
