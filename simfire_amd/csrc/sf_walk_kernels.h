// Walking distance (sf_walk): the number of moves of a walker that enters only walkable cells until it steps
// onto a target cell - a breadth-first search over the 4- or 8-neighbourhood, level by level.  The reference has nothing of the kind.
// One bit per cell, 64 cells per word, band-major planes as in the flood fill of section 23 (whose staging, halo and addressing
// helpers are used here); ONE workgroup per listed environment, resident until the search ends - no workgroup waits for another.
// A thread owns a BAND: one word column times 16 rows.  Three planes: T (targets), U (walkable, not a target, not yet reached) and
// the FRONT (the cells the last level added; at the start T).  A level is, per band, front' = dilate(front) & U, U &= ~front': Jacobi,
// in place over the 16 rows with the old row above carried in a register; the rows and columns of the neighbouring bands come
// through a halo (top / bottom words, edge columns).  Only the front is dilated; a band whose front and halo are empty skips the
// level.  The search ends at the first level that adds nothing (__syncthreads_or) or at max_moves.
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
#include "sf_reach_kernels.h"

namespace {

constexpr int kWalkThreads = 1024;
constexpr int kWalkMaxWidth = 8192;           // wider grids are refused (as sf_distance and sf_reach do)
constexpr long long kWalkScratchDefault = 256ll << 20;
constexpr int32_t kWalkFar = 2147483647, kWalkBlocked = -1;

struct WalkArgs {
    // of these the search uses: g, pl, envs, passable, pass_env, pass_vec, points, k, scratch, scratch_env, slo / shi (the
    // target mask), tlo / thi (the through mask), conn8, WORDS, BR, nb - the staging helper takes them in this form
    ReachArgs r;
    const uint8_t *targets;      // dense u8 [H * W] (tgt_env = 0) or [E][H * W], or null
    long long tgt_env;
    int tgt_vec;                 // 16-byte loads of targets (W % 16 == 0 and an aligned plane)
    int max_moves;               // 0: no cap
    int moves_vec;               // 16-byte stores of the pre-fill (W % 4 == 0 and an aligned output)
    int32_t *moves;              // this chunk's part of the outputs (null: not asked for)
    int32_t *point_moves, *point_step, *reached, *levels;
};

// bytes of scratch per listed environment: three bit planes (front, front, U) of BR * 16 rows, and two halos of two words and one
// edge dword per band
__host__ __device__ inline long long walk_env_bytes(const Geo &g)
{
    const long long nb = (long long)reach_band_rows(g) * reach_words(g);
    return (nb * kReachRows * 24 + nb * 40 + 255) / 256 * 256;
}

// The 64 cells of word wi of row y of a dense u8 plane as bits (cell != 0); cells past the width give 0
__device__ __forceinline__ reach_word walk_plane_bits(const uint8_t *plane, int vec, const Geo &g, int y, int wi)
{
    reach_word out = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int v = wi * 4 + q;
        if (v >= g.PV) break;
        const uint32_t b = pack16(and44(nz01x16(dense_vec16(plane, vec, g.W, y, v)), first01x16(g.W - v * 16)));
        out |= (reach_word)b << (16 * q);
    }
    return out;
}

// One level of a band, in place: f (the front) becomes dilate(f) & U, and those cells leave U (ub: the band's 16 words of U, LDS or
// the scratch plane).  Jacobi: every row is dilated from the OLD rows - the one above is carried in prev, the one below is still
// untouched.  Returns whether a cell was added.
__device__ __forceinline__ bool walk_level(reach_word (&f)[kReachRows], reach_word *ub, const ReachHalo &h, int conn8)
{
    reach_word any = 0, prev = h.top;
#pragma unroll
    for (int j = 0; j < kReachRows; ++j) {
        const reach_word cur = f[j], next = j == kReachRows - 1 ? h.bot : f[j + 1];
        reach_word w = (cur << 1) | (cur >> 1) | (reach_word)((h.el >> (j + 1)) & 1u) | (reach_word)((h.er >> (j + 1)) & 1u) << 63;
        w |= reach_spread(prev, (h.el >> j) & 1u, (h.er >> j) & 1u, conn8) | reach_spread(next, (h.el >> (j + 2)) & 1u, (h.er >> (j + 2)) & 1u, conn8);
        const reach_word u = ub[j], nw = w & u;
        if (nw) ub[j] = u & ~nw;
        f[j] = nw;
        prev = cur;
        any |= nw;
        if ((j & 3) == 3) __builtin_amdgcn_sched_barrier(0);       // (keeps the U reads of all rows from being hoisted to the top)
    }
    return any != 0;
}

// The level's number to the cells the band added: a store per set bit (the cells of U lie on the grid)
__device__ __forceinline__ void walk_scatter(const reach_word (&f)[kReachRows], int32_t *band, int W, int32_t level)
{
#pragma unroll
    for (int j = 0; j < kReachRows; ++j) {
        reach_word w = f[j];
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

__device__ __forceinline__ uint32_t walk_bit(const reach_word *plane, int WORDS, int y, int x)
{
    return (uint32_t)(plane[reach_at(WORDS, y, x >> 6)] >> (x & 63)) & 1u;
}

// dynamic LDS of k_walk<true> with nt threads: U [nt][kReachLdsRow] (a thread's 16 words and one of padding) and the halo top [nt],
// bottom [nt], edges [nt]; k_walk<false> uses none
__host__ __device__ inline size_t walk_lds_bytes(int nt, bool resident) { return resident ? (size_t)nt * (kReachLdsRow * 8 + 8 + 8 + 4) : 0; }

template <bool RES>
__global__ __launch_bounds__(kWalkThreads) void k_walk(const WalkArgs *__restrict__ ap)
{
    extern __shared__ __attribute__((aligned(16))) reach_word s_walk[];       // walk_lds_bytes(nt, RES)
    __shared__ int s_reached;
    const WalkArgs &a = *ap;
    const ReachArgs &r = a.r;
    const Geo &g = r.g;
    const int t = threadIdx.x, nt = blockDim.x;
    const int i = blockIdx.x, e = r.envs[i];
    const int WORDS = r.WORDS, BR = r.BR, nb = r.nb, conn8 = r.conn8, M = a.max_moves;
    const int32_t far = M ? M : kWalkFar;
    const long long plane_words = (long long)nb * kReachRows;
    reach_word *pl_a = reinterpret_cast<reach_word *>(r.scratch + (long long)i * r.scratch_env);      // T, then a front
    reach_word *pl_b = pl_a + plane_words;                                                              // the other front
    reach_word *pl_u = pl_b + plane_words;
    reach_word *g_top = pl_u + plane_words, *g_bot = g_top + 2 * (long long)nb;                         // [2][nb] each
    uint32_t *g_edge = reinterpret_cast<uint32_t *>(g_bot + 2 * (long long)nb);
    reach_word *s_u = s_walk;
    reach_word *l_top = s_walk + kReachLdsRow * nt, *l_bot = l_top + nt;
    uint32_t *l_edge = reinterpret_cast<uint32_t *>(l_bot + nt);
    const int passes = RES ? 1 : (nb + nt - 1) / nt;
    int32_t *out = a.moves ? a.moves + (long long)i * g.H * g.W : nullptr;
    if (t == 0) s_reached = 0;

    // staging: a word per thread and turn into the planes T and U of the scratch
    const uint8_t *tgt = a.targets ? a.targets + a.tgt_env * e : nullptr;
#pragma unroll 1
    for (int idx = t; idx < nb * kReachRows; idx += nt) {
        const int y = idx / WORDS, wi = idx - y * WORDS;
        reach_word sd, op;
        reach_stage(r, e, y, wi, sd, op);
        if (tgt && y < g.H) sd |= walk_plane_bits(tgt, a.tgt_vec, g, y, wi);
        pl_a[reach_at(WORDS, y, wi)] = sd; pl_u[reach_at(WORDS, y, wi)] = op & ~sd;
    }
    __syncthreads();

    // the plane form's pre-fill, four cells per turn: 0 on targets, far on walkable cells, blocked elsewhere
    if (out) {
        const int G4 = (g.W + 3) / 4;
#pragma unroll 1
        for (int idx = t; idx < g.H * G4; idx += nt) {
            const int y = idx / G4, x0 = (idx - y * G4) * 4;
            const long long at = reach_at(WORDS, y, x0 >> 6);
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
    const int k = r.k;
    bool pend = false;
    int px = 0, py = 0;
    uint32_t pel = 0;
    int32_t pval = -1, pstep = -1;
    const int nn = conn8 ? 8 : 4;
    if (t < k) {
        const QueryPoint p = query_point(r.points, (long long)i * k + t, g.W, g.H);
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
    reach_word fres[RES ? kReachRows : 1];
    bool live = false;
    int cnt = 0;
    for (int p = 0; p < passes; ++p) {
        const int b = p * nt + t;
        if (b < nb) {
            reach_word fpass[RES ? 1 : kReachRows];
            reach_word (&f)[kReachRows] = *reinterpret_cast<reach_word (*)[kReachRows]>(RES ? fres : fpass);
            reach_word any = 0;
#pragma unroll
            for (int j = 0; j < kReachRows; ++j) {
                f[j] = reach_ref(pl_a, (uint32_t)b * (kReachRows * 8u) + j * 8u);
                const reach_word u = reach_ref(pl_u, (uint32_t)b * (kReachRows * 8u) + j * 8u);
                if (RES) s_u[t * kReachLdsRow + j] = u;
                cnt += __popcll(u);
                any |= f[j];
            }
            live = any != 0;
            reach_ref(RES ? l_top : g_top, (uint32_t)b * 8u) = f[0]; reach_ref(RES ? l_bot : g_bot, (uint32_t)b * 8u) = f[kReachRows - 1];
            reach_ref(RES ? l_edge : g_edge, (uint32_t)b * 4u) = reach_edges(f);
        }
    }
    __syncthreads();

    // what a point sees after level L (the cells with d <= L have left U): its value is L + 1 at the first L at which a neighbour has
    auto test_point = [&](int L) {
        if (!pend) return;
        for (int n = 0; n < nn; ++n) {
            if (!((pel >> n) & 1u)) continue;
            const int nx = px + walk_dx(n), ny = py + walk_dy(n);
            const int b =(ny / kReachRows) * WORDS + (nx >> 6);
            const reach_word u = RES ? s_u[b * kReachLdsRow + (ny % kReachRows)] : pl_u[(long long)b * kReachRows + (ny % kReachRows)];
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
            ReachHalo h = {};
            if (on) h = reach_halo(WORDS, BR, l_top, l_bot, l_edge, br, wi);
            __syncthreads();                  // every band has read its halo: the level may now publish
            if (on && (live || (h.top | h.bot) != 0 || (h.el | h.er) != 0)) {
                reach_word (&f)[kReachRows] = *reinterpret_cast<reach_word (*)[kReachRows]>(fres);
                live = walk_level(f, s_u + t * kReachLdsRow, h, conn8);
                reach_ref(l_top, (uint32_t)t * 8u) = f[0]; reach_ref(l_bot, (uint32_t)t * 8u) = f[kReachRows - 1]; reach_ref(l_edge, (uint32_t)t * 4u) = reach_edges(f);
                if (live) {
                    added = 1;
                    if (out) walk_scatter(f, out + ((long long)br * kReachRows) * g.W + wi * 64, g.W, L + 1);
                }
            }
        } else {
            const reach_word *f_old = cur ? pl_b : pl_a;
            reach_word *f_new = cur ? pl_a : pl_b;
            const reach_word *top_old = g_top + (long long)cur * nb, *bot_old = g_bot + (long long)cur * nb;
            const uint32_t *edge_old = g_edge + (long long)cur * nb;
            reach_word *top_new = g_top + (long long)(cur ^ 1) * nb, *bot_new = g_bot + (long long)(cur ^ 1) * nb;
            uint32_t *edge_new = g_edge + (long long)(cur ^ 1) * nb;
            for (int p = 0; p < passes; ++p) {
                const int b = p * nt + t;
                if (b < nb) {
                    const int br = b / WORDS, wi = b - br * WORDS;
                    const ReachHalo h = reach_halo(WORDS, BR, top_old, bot_old, edge_old, br, wi);
                    reach_word fpass[RES ? 1 : kReachRows];
                    reach_word (&f)[kReachRows] = *reinterpret_cast<reach_word (*)[kReachRows]>(fpass);
#pragma unroll
                    for (int j = 0; j < kReachRows; ++j) f[j] = reach_ref(f_old, (uint32_t)b * (kReachRows * 8u) + j * 8u);
                    const bool nw = walk_level(f, pl_u + (long long)b * kReachRows, h, conn8);
#pragma unroll
                    for (int j = 0; j < kReachRows; ++j) reach_ref(f_new, (uint32_t)b * (kReachRows * 8u) + j * 8u) = f[j];
                    reach_ref(top_new, (uint32_t)b * 8u) = f[0]; reach_ref(bot_new, (uint32_t)b * 8u) = f[kReachRows - 1]; reach_ref(edge_new, (uint32_t)b * 4u) = reach_edges(f);
                    if (nw) {
                        added = 1;
                        if (out) walk_scatter(f, out + ((long long)br * kReachRows) * g.W + wi * 64, g.W, L + 1);
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
                for (int j = 0; j < kReachRows; ++j)
                    cnt -= __popcll(RES ? s_u[t * kReachLdsRow + j] : reach_ref(pl_u, (uint32_t)b * (kReachRows * 8u) + j * 8u));
            }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) cnt += __shfl_xor(cnt, m);
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
