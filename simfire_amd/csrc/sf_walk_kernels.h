// Walking distance (sf_walk): the number of moves of a walker that enters only walkable cells until it steps
// onto a target cell - a breadth-first search over the 4- or 8-neighbourhood, level by level.  The reference has nothing of the kind.
// The bit planes, the bands, the halo and the level of a band are sf_bands.h; ONE workgroup per listed environment, resident until
// the search ends - no workgroup waits for another.  Three planes: T (targets), U (walkable, not a target, not yet reached) and the
// FRONT (the cells the last level added; at the start T).  Only the front is dilated; a band whose front and halo are empty skips
// the level.  The search ends at the first level that adds nothing (__syncthreads_or) or at max_moves.
// k_walk<true>: at most one band per thread - the front stays in registers, U in the thread's own LDS row, the halo in LDS; a level
// is halo read | barrier | dilate and publish | barrier-or.  k_walk<false>: larger grids - the planes live in the handle's scratch
// (L2), the front and the halo twice: a level reads the old copies and writes the new ones, so the passes of 1024 bands need no
// order and no barrier between them.
// Outputs inside the search: a lane per point tests after every level whether a target-or-walkable neighbour of its cell has left U
// (targets were never in it): the first level at which one has is its value, the lowest move code among those neighbours its step -
// no distance plane is needed.  The plane form is pre-filled coalesced (0 / far / blocked) and every level scatters its number to
// the cells it added.  reached is popcount(U at the start) - popcount(U at the end).
// Part of the single translation unit simfire_hip.hip.  The status bytes are read from whichever cell plane is current; nothing but
// the scratch and the outputs is written.
#pragma once
#include "sf_bands.h"
#include "sf_query_dev.h"

namespace {

constexpr int kWalkMaxWidth = 8192;           // wider grids are refused (as sf_distance and sf_reach do)
constexpr long long kWalkScratchDefault = 256ll << 20;
constexpr int32_t kWalkFar = 2147483647, kWalkBlocked = -1;

struct WalkArgs {
    BandArgs band;               // slo / shi: target_mask, tlo / thi: through_mask; scratch: T | the other front | U | halo top [2] | bottom [2] | edges [2]
    const uint8_t *targets;      // dense u8 [H * W] (tgt_env = 0) or [E][H * W], or null
    long long tgt_env;
    int tgt_vec;                 // 16-byte loads of targets (W % 16 == 0 and an aligned plane)
    int max_moves;               // 0: no cap
    int moves_vec;               // 16-byte stores of the pre-fill (W % 4 == 0 and an aligned output)
    int32_t *moves;              // this chunk's part of the outputs (null: not asked for)
    int32_t *point_moves, *point_step, *reached, *levels;
};

// bytes of scratch per listed environment: three bit planes (front, front, U) and two halos
__host__ __device__ inline long long walk_env_bytes(const Geo &g) { return band_env_bytes((long long)band_rows(g.H) * band_words(g.P), 3, 2); }

// The level's number to the cells the band added: a store per set bit (the cells of U lie on the grid)
__device__ __forceinline__ void walk_scatter(const band_word (&f)[kBandRows], int32_t *band, int W, int32_t level)
{
#pragma unroll
    for (int j = 0; j < kBandRows; ++j) {
        band_word w = f[j];
        int32_t *row = band + (long long)j * W;
        while (w) {
            row[__builtin_ctzll(w)] = level;
            w &= w - 1;
        }
    }
}

// Neighbour n of a cell: 0..3 are the moves of the action word (code n + 1: row - 1, row + 1, column - 1, column + 1), 4..7 the diagonals
__device__ __forceinline__ int walk_dx(int n) { return n == 2 || n == 4 || n == 6 ? -1 : (n == 3 || n == 5 || n == 7 ? 1 : 0); }
__device__ __forceinline__ int walk_dy(int n) { return n == 0 || n == 4 || n == 5 ? -1 : (n == 1 || n == 6 || n == 7 ? 1 : 0); }

__device__ __forceinline__ uint32_t walk_bit(const band_word *plane, int WORDS, int y, int x) { return (uint32_t)(plane[band_at(WORDS, y, x >> 6)] >> (x & 63)) & 1u; }

// dynamic LDS of k_walk<true> with nt threads: U [nt][kBandLdsRow] and the halo top [nt], bottom [nt], edges [nt]; k_walk<false>: none
__host__ __device__ inline size_t walk_lds_bytes(int nt, bool resident) { return resident ? (size_t)nt * (kBandLdsRow * 8 + 8 + 8 + 4) : 0; }

template <bool RES>
__global__ __launch_bounds__(kBandThreads) void k_walk(const WalkArgs *__restrict__ ap)
{
    extern __shared__ __attribute__((aligned(16))) band_word s_walk[];       // walk_lds_bytes(nt, RES)
    __shared__ int s_reached;
    const WalkArgs &a = *ap;
    const BandArgs &ba = a.band;
    const Geo &g = ba.g;
    const int t = threadIdx.x, nt = blockDim.x;
    const int i = blockIdx.x, e = ba.envs[i];
    const int WORDS = ba.WORDS, BR = ba.BR, nb = ba.nb, conn8 = ba.conn8, M = a.max_moves;
    const int32_t far = M ? M : kWalkFar;
    const long long plane_words = (long long)nb * kBandRows;
    band_word *pl_a = reinterpret_cast<band_word *>(ba.scratch + (long long)i * ba.scratch_env);      // T, then a front
    band_word *pl_b = pl_a + plane_words;                                                              // the other front
    band_word *pl_u = pl_b + plane_words;
    band_word *g_top = pl_u + plane_words, *g_bot = g_top + 2 * (long long)nb;                         // [2][nb] each
    uint32_t *g_edge = reinterpret_cast<uint32_t *>(g_bot + 2 * (long long)nb);
    band_word *s_u = s_walk;
    band_word *l_top = s_walk + kBandLdsRow * nt, *l_bot = l_top + nt;
    uint32_t *l_edge = reinterpret_cast<uint32_t *>(l_bot + nt);
    const int passes = RES ? 1 : (nb + nt - 1) / nt;
    int32_t *out = a.moves ? a.moves + (long long)i * g.H * g.W : nullptr;
    if (t == 0) s_reached = 0;

    // staging: a word per thread and turn into the planes T and U of the scratch
    const uint8_t *tgt = a.targets ? a.targets + a.tgt_env * e : nullptr;
#pragma unroll 1
    for (int idx = t; idx < nb * kBandRows; idx += nt) {
        const int y = idx / WORDS, wi = idx - y * WORDS;
        band_word sd, op;
        band_stage(ba, e, y, wi, tgt, a.tgt_vec, sd, op);
        pl_a[band_at(WORDS, y, wi)] = sd; pl_u[band_at(WORDS, y, wi)] = op & ~sd;
    }
    __syncthreads();

    // the plane form's pre-fill, four cells per turn: 0 on targets, far on walkable cells, blocked elsewhere
    if (out) {
        const int G4 = (g.W + 3) / 4;
#pragma unroll 1
        for (int idx = t; idx < g.H * G4; idx += nt) {
            const int y = idx / G4, x0 = (idx - y * G4) * 4;
            const long long at = band_at(WORDS, y, x0 >> 6);
            const uint32_t tb = (uint32_t)(pl_a[at] >> (x0 & 63)) & 0xFu, ub = (uint32_t)(pl_u[at] >> (x0 & 63)) & 0xFu;
            int32_t v[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = (tb >> c) & 1u ? 0 : ((ub >> c) & 1u ? far : kWalkBlocked);
            int32_t *dst = out + (long long)y * g.W + x0;
            if (a.moves_vec) {
                *reinterpret_cast<int4 *>(dst) = make_int4(v[0], v[1], v[2], v[3]);
            } else {
                const int in = min(4, g.W - x0);
                for (int c = 0; c < in; ++c) dst[c] = v[c];
            }
        }
    }

    // the points: lane t answers point t.  pel: bit n = neighbour n (move code n + 1; 4..7 the diagonals) is on the grid and a target
    // or walkable
    const int k = ba.k;
    bool pend = false;
    int px = 0, py = 0;
    uint32_t pel = 0;
    int32_t pval = -1, pstep = -1;
    const int nn = conn8 ? 8 : 4;
    if (t < k) {
        const QueryPoint p = query_point(ba.points, (long long)i * k + t, g.W, g.H);
        px = p.x; py = p.y;
        if (p.ok) {
            pstep = 0;
            if (walk_bit(pl_a, WORDS, py, px)) {
                pval = 0;
            } else {
                pval = far;
                for (int n = 0; n < nn; ++n) {
                    const int nx = px + walk_dx(n), ny = py + walk_dy(n);
                    if (nx >= 0 && nx < g.W && ny >= 0 && ny < g.H && (walk_bit(pl_a, WORDS, ny, nx) | walk_bit(pl_u, WORDS, ny, nx))) pel |= 1u << n;
                }
                pend = pel != 0;
            }
        }
    }

    // the bands: the front to registers and U to LDS (k_walk<true>), the first halo
    band_word f[kBandRows];                   // the band's front: k_walk<true> for the whole search, k_walk<false> that of the pass
    bool live = false;
    int cnt = 0;
    for (int p = 0; p < passes; ++p) {
        const int b = p * nt + t;
        if (b < nb) {
            band_word any = 0;
#pragma unroll
            for (int j = 0; j < kBandRows; ++j) {
                f[j] = band_ref(pl_a, (uint32_t)b * (kBandRows * 8u) + j * 8u);
                const band_word u = band_ref(pl_u, (uint32_t)b * (kBandRows * 8u) + j * 8u);
                if (RES) s_u[t * kBandLdsRow + j] = u;
                cnt += __popcll(u);
                any |= f[j];
            }
            live = any != 0;
            band_publish(RES ? l_top : g_top, RES ? l_bot : g_bot, RES ? l_edge : g_edge, b, f);
        }
    }
    __syncthreads();

    // what a point sees after level L (the cells with d <= L have left U): its value is L + 1 at the first L at which a neighbour has
    auto test_point = [&](int L) {
        if (!pend) return;
        for (int n = 0; n < nn; ++n) {
            if (!((pel >> n) & 1u)) continue;
            const int nx = px + walk_dx(n), ny = py + walk_dy(n);
            const int b =(ny / kBandRows) * WORDS + (nx >> 6);
            const band_word u = RES ? s_u[b * kBandLdsRow + (ny % kBandRows)] : pl_u[(long long)b * kBandRows + (ny % kBandRows)];
            if (!((u >> (nx & 63)) & 1u)) {
                pval = L + 1; pstep = conn8 ? 0 : n + 1; pend = false;
                break;
            }
        }
    };
    test_point(0);
    if (!RES && k) __syncthreads();           // (k_walk<false>: the next level writes U at once; k_walk<true> has its halo barrier in between)

    // the search: levels until one adds nothing (or max_moves)
    int L = 0, cur = 0;
    for (;;) {
        if (M && L == M) break;
        int added = 0;
        if (RES) {
            const bool on = t < nb;
            const int br = on ? t / WORDS : 0, wi = on ? t - br * WORDS : 0;
            BandHalo h = {};
            if (on) h = band_halo(WORDS, BR, l_top, l_bot, l_edge, br, wi);
            __syncthreads();                  // every band has read its halo: the level may now publish
            if (on && (live || (h.top | h.bot) != 0 || (h.el | h.er) != 0)) {
                live = band_level(f, s_u + t * kBandLdsRow, h, conn8);
                band_publish(l_top, l_bot, l_edge, t, f);
                if (live) {
                    added = 1;
                    if (out) walk_scatter(f, out + ((long long)br * kBandRows) * g.W + wi * 64, g.W, L + 1);
                }
            }
        } else {
            const band_word *f_old = cur ? pl_b : pl_a;
            band_word *f_new = cur ? pl_a : pl_b;
            const band_word *top_old = g_top + (long long)cur * nb, *bot_old = g_bot + (long long)cur * nb;
            const uint32_t *edge_old = g_edge + (long long)cur * nb;
            band_word *top_new = g_top + (long long)(cur ^ 1) * nb, *bot_new = g_bot + (long long)(cur ^ 1) * nb;
            uint32_t *edge_new = g_edge + (long long)(cur ^ 1) * nb;
            for (int p = 0; p < passes; ++p) {
                const int b = p * nt + t;
                if (b < nb) {
                    const int br = b / WORDS, wi = b - br * WORDS;
                    const BandHalo h = band_halo(WORDS, BR, top_old, bot_old, edge_old, br, wi);
                    band_load(f, f_old, b);
                    const bool nw = band_level(f, pl_u + (long long)b * kBandRows, h, conn8);
                    band_store(f_new, b, f);
                    band_publish(top_new, bot_new, edge_new, b, f);
                    if (nw) {
                        added = 1;
                        if (out) walk_scatter(f, out + ((long long)br * kBandRows) * g.W + wi * 64, g.W, L + 1);
                    }
                }
            }
            cur ^= 1;
        }
        if (!__syncthreads_or(added)) break;
        ++L;
        if (!M || L < M) test_point(L);
        if (!RES && k) __syncthreads();
    }

    // epilogue
    if (a.reached) {
        for (int p = 0; p < passes; ++p) {
            const int b = p * nt + t;
            if (b < nb) {
#pragma unroll
                for (int j = 0; j < kBandRows; ++j)
                    cnt -= __popcll(RES ? s_u[t * kBandLdsRow + j] : band_ref(pl_u, (uint32_t)b * (kBandRows * 8u) + j * 8u));
            }
        }
        cnt = wave_sum(cnt);
        if ((t & 63) == 0 && cnt) atomicAdd(&s_reached, cnt);
    }
    if (t < k) {
        if (a.point_moves) a.point_moves[(long long)i * k + t] = pval;
        if (a.point_step) a.point_step[(long long)i * k + t] = pstep;
    }
    __syncthreads();
    if (t == 0) {
        if (a.reached) a.reached[i] = s_reached;
        if (a.levels) a.levels[i] = L;
    }
}

}  // namespace
