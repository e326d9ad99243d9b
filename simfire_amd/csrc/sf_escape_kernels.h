// Escape routes (sf_escape): the ESCAPE SLACK of every cell or point - how many more moves a walker may wait
// where it stands and still reach a target cell, never standing on a cell at or after the moment the fire closes it.  The reference
// has nothing of the kind; the definitions are the library's own:
//   D(c), the deadline, from T = minutes[c]: NEVER if T < 0 or not T < horizon; else q = ((double)T - margin) / minutes_per_move and
//   D = q > 0 ? (int)ceil(q) : 0.  A walker may stand on c at move index m (now: 0) exactly when m < D(c).
//   S(c) = min(D(c) - 1, max over the target-or-walkable neighbours n of S(n) - 1) on walkable cells, SAFE on targets, with SAFE - 1 =
//   SAFE, NEVER - 1 = SAFE and the maximum over nothing LOST (-1); BLOCKED (-2) on cells that are neither: a bottleneck shortest path.
// ONE workgroup per listed environment, resident until the search ends - no workgroup waits for another.  The bit planes, the bands,
// the halo and a level's arithmetic (band_round, band_grow) are sf_bands.h.  Three planes: A (the safe set; at the start the
// targets), W (walkable, no target) and U (walkable, not in A, open now; at the start the NEVER cells).
// Staging: the planes; a histogram of the finite deadlines 1..bins of the W cells in LDS (a wave per word, a lane per cell: the
// NEVER word is one ballot), its prefix sum, the non-empty buckets compacted (deadline and first entry) and the cells scattered into
// the environment's list - a counting sort; the order inside a bucket does not matter.  The histogram has left LDS before U moves in.
// Phase 1: A is flooded from the targets through U (band_round, the fill of sf_reach): those cells are SAFE.
// Phase 2: v runs from the largest deadline - 1 down to 0.  The lanes set the U bits of the bucket D == v + 1; every live band takes
// new = dilate(A) & U, A |= new, U &= ~new: the cells of new have slack v.  The WHOLE of A is dilated - a cell that opens late may sit
// next to an old one.  A band is live when a cell of it opened this level or when it or one of its eight neighbours grew last level.  A level
// that opens nothing and follows one that added nothing jumps to the next non-empty bucket; the search ends with the buckets.
// k_escape<true>: at most one band per thread - A stays in registers, U in the thread's own LDS row, the halo in LDS.
// k_escape<false>: larger grids - the planes and two copies of the halo live in the scratch; every level passes over all bands.
// Points: lane t owns point t with the deadlines of its cell and neighbours; after level v a walkable neighbour n has joined exactly
// when D(n) > v and its U bit is clear - no slack plane is needed.  The plane form is pre-filled coalesced and every level scatters.
// Part of the single translation unit simfire_hip.hip.  Nothing but the scratch and the outputs is written.
#pragma once
#include "sf_bands.h"
#include "sf_query_dev.h"
#include "sf_walk_kernels.h"

namespace {

constexpr int kEscapeMaxWidth = 8192;
constexpr long long kEscapeScratchDefault = 1280ll << 20;       // 256 environments of 1024 x 1024 are one chunk (4.7 MiB each)
constexpr int32_t kEscapeSafe = 2147483647, kEscapeLost = -1, kEscapeBlocked = -2;
constexpr int kEscapeNever = 2147483647;      // a deadline: the fire does not close the cell within the horizon
constexpr int kEscapeMaxMoves = 32768;        // the largest finite deadline: the bins of the histogram (128 KiB of LDS)
constexpr long long kEscapeBoundsBytes = ((2ll * kEscapeMaxMoves + 3) * 4 + 255) / 256 * 256;       // the non-empty buckets: deadline [bins] | first entry [bins + 1]

struct EscapeArgs {
    BandArgs band;               // slo / shi: target_mask, tlo / thi: through_mask; scratch: A | W | U | halo top [2] | bottom [2] | edges [2] | list | buckets
    const uint8_t *targets;      // dense u8 [H * W] (tgt_env = 0) or [E][H * W], or null
    long long tgt_env;
    int tgt_vec;
    const float *minutes;        // this chunk's [cn][H][W]
    double per_move, margin, horizon;
    int unreached_safe;
    int bins;                    // the move bound: no finite deadline is larger
    int slack_vec;               // 16-byte stores of the pre-fill (W % 4 == 0 and an aligned output)
    long long o_list, o_buckets; // byte offsets in an environment's scratch
    int32_t *slack;              // this chunk's part of the outputs (null: not asked for)
    int32_t *point_slack, *point_step, *safe, *escapable, *lost, *top;
};

// bytes of scratch per listed environment: three bit planes and two halos | the sorted cells | the buckets
__host__ __device__ inline long long escape_list_offset(const Geo &g) { return band_env_bytes((long long)band_rows(g.H) * band_words(g.P), 3, 2); }
__host__ __device__ inline long long escape_env_bytes(const Geo &g)
{
    return escape_list_offset(g) + (4ll * g.H * g.W + 255) / 256 * 256 + kEscapeBoundsBytes;
}
// dynamic LDS: the histogram first, then U [nt][kBandLdsRow] and the halo (k_escape<true>)
__host__ __device__ inline size_t escape_lds_bytes(int nt, bool resident)
{
    const size_t hist = (size_t)kEscapeMaxMoves * 4, search = resident ? (size_t)nt * (kBandLdsRow * 8 + 8 + 8 + 4) : 0;
    return hist > search ? hist : search;
}

__device__ __forceinline__ int escape_deadline(float T, double horizon, double margin, double per_move)
{
    if (T < 0.0f || !((double)T < horizon)) return kEscapeNever;
    const double q = ((double)T - margin) / per_move;
    return q > 0.0 ? (int)ceil(q) : 0;
}

// A value to the cells w of one row (the cells of U lie on the grid)
__device__ __forceinline__ void escape_scatter(int32_t *row, band_word w, int32_t val)
{
    while (w) {
        row[__builtin_ctzll(w)] = val;
        w &= w - 1;
    }
}

template <bool RES>
__global__ __launch_bounds__(kBandThreads) void k_escape(const EscapeArgs *__restrict__ ap)
{
    extern __shared__ __attribute__((aligned(16))) band_word s_esc[];        // escape_lds_bytes(nt, RES)
    __shared__ unsigned long long s_wave[kBandThreads / 64];
    __shared__ uint32_t s_wake[2][kBandThreads / 32];                        // k_escape<true>: bit b = band b is live, by the level's parity
    __shared__ int s_walkable, s_top, s_safe, s_targets, s_set, s_buckets;
    const EscapeArgs &a = *ap;
    const BandArgs &ba = a.band;
    const Geo &g = ba.g;
    const int t = threadIdx.x, nt = blockDim.x, lane = t & 63;
    const int i = blockIdx.x, e = ba.envs[i];
    const int WORDS = ba.WORDS, BR = ba.BR, nb = ba.nb, conn8 = ba.conn8, bins = a.bins;
    const long long plane_words = (long long)nb * kBandRows;
    uint8_t *scratch = ba.scratch + (long long)i * ba.scratch_env;
    band_word *pl_a = reinterpret_cast<band_word *>(scratch);
    band_word *pl_w = pl_a + plane_words;
    band_word *pl_u = pl_w + plane_words;
    band_word *g_top = pl_u + plane_words, *g_bot = g_top + 2 * (long long)nb;                          // [2][nb] each
    uint32_t *g_edge = reinterpret_cast<uint32_t *>(g_bot + 2 * (long long)nb);
    int32_t *list = reinterpret_cast<int32_t *>(scratch + a.o_list);
    int32_t *bk_d = reinterpret_cast<int32_t *>(scratch + a.o_buckets), *bk_at = bk_d + kEscapeMaxMoves;      // deadline [<= bins] | first entry [<= bins + 1]
    int *hist = reinterpret_cast<int *>(s_esc);
    band_word *s_u = s_esc;
    band_word *l_top = s_esc + kBandLdsRow * nt, *l_bot = l_top + nt;
    uint32_t *l_edge = reinterpret_cast<uint32_t *>(l_bot + nt);
    const int passes = RES ? 1 : (nb + nt - 1) / nt;
    const float *mins = a.minutes + (long long)i * g.H * g.W;
    int32_t *out = a.slack ? a.slack + (long long)i * g.H * g.W : nullptr;
    if (t == 0) { s_walkable = 0; s_top = 0; s_safe = 0; s_targets = 0; s_set = 0; s_buckets = 0; }
    if (t < 2 * (kBandThreads / 32)) (&s_wake[0][0])[t] = 0;
#pragma unroll 1
    for (int b = t; b < bins; b += nt) hist[b] = 0;

    // staging 1: a word per thread and turn into the planes A (targets) and W (walkable, no target); U empty
    const uint8_t *tgt = a.targets ? a.targets + a.tgt_env * e : nullptr;
#pragma unroll 1
    for (int idx = t; idx < nb * kBandRows; idx += nt) {
        const int y = idx / WORDS, wi = idx - y * WORDS;
        band_word sd, op;
        band_stage(ba, e, y, wi, tgt, a.tgt_vec, sd, op);
        const long long at = band_at(WORDS, y, wi);
        pl_a[at] = sd; pl_w[at] = op & ~sd; pl_u[at] = 0;
    }
    __syncthreads();

    // staging 2: a wave per word, a lane per cell - the deadlines of the W cells: NEVER cells to U (or, unreached_safe, to A), the
    // finite ones counted by deadline
    {
        int walkable = 0, top = 0;
#pragma unroll 1
        for (int idx = t >> 6; idx < g.H * WORDS; idx += nt >> 6) {
            const int y = idx / WORDS, wi = idx - y * WORDS;
            const long long at = band_at(WORDS, y, wi);
            const band_word w = pl_w[at];
            if (!w) continue;
            const bool mine = (w >> lane) & 1u;
            int D = 0;
            if (mine) D = escape_deadline(mins[(long long)y * g.W + wi * 64 + lane], a.horizon, a.margin, a.per_move);
            const band_word never = __ballot(mine && D == kEscapeNever);
            if (mine && D > 0 && D <= bins) {
                atomicAdd(&hist[D - 1], 1);
                top = max(top, D);
            }
            if (lane == 0) {
                if (a.unreached_safe) {
                    pl_a[at] |= never; pl_w[at] = w & ~never;
                    walkable += __popcll(w & ~never);
                } else {
                    pl_u[at] = never;
                    walkable += __popcll(w);
                }
            }
        }
        top = wave_max(top);
        if (lane == 0) { if (walkable) atomicAdd(&s_walkable, walkable); if (top) atomicMax(&s_top, top); }
    }
    __syncthreads();

    // staging 3: the prefix sum of the histogram, a run of bins per thread; the non-empty buckets compacted (deadline, first entry);
    // a bin then holds its bucket's cursor
    {
        const int per = (bins + nt - 1) / nt, b0 = min(bins, t * per), b1 = min(bins, b0 + per);
        unsigned long long mine = 0;              // non-empty bins << 32 | cells
        for (int b = b0; b < b1; ++b) { const int c = hist[b]; mine += (unsigned long long)c + (c ? 1ull << 32 : 0ull); }
        unsigned long long incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const unsigned long long u = __shfl_up(incl, o); if (lane >= o) incl += u; }
        if (lane == 63) s_wave[t >> 6] = incl;
        __syncthreads();
        unsigned long long before = incl - mine;
        for (int w = 0; w < (t >> 6); ++w) before += s_wave[w];
        int at = (int)(before & 0xFFFFFFFFull), nk = (int)(before >> 32);
        for (int b = b0; b < b1; ++b) {
            const int c = hist[b];
            if (c) { bk_d[nk] = b + 1; bk_at[nk] = at; ++nk; }
            hist[b] = at;
            at += c;
        }
        if (t == nt - 1) { bk_at[nk] = at; s_buckets = nk; }
    }
    __syncthreads();

    // staging 4: the cells into their buckets
#pragma unroll 1
    for (int idx = t >> 6; idx < g.H * WORDS; idx += nt >> 6) {
        const int y = idx / WORDS, wi = idx - y * WORDS;
        const long long at = band_at(WORDS, y, wi);
        const band_word w = pl_w[at] & ~pl_u[at];
        if (!((w >> lane) & 1u)) continue;
        const int x = wi * 64 + lane;
        const int D = escape_deadline(mins[(long long)y * g.W + x], a.horizon, a.margin, a.per_move);
        if (D > 0 && D <= bins) list[atomicAdd(&hist[D - 1], 1)] = y * g.W + x;
    }
    const int n_buckets = s_buckets;

    // the plane form's pre-fill, four cells per turn: SAFE on targets, LOST on walkable cells, BLOCKED elsewhere
    if (out) {
        const int G4 = (g.W + 3) / 4;
#pragma unroll 1
        for (int idx = t; idx < g.H * G4; idx += nt) {
            const int y = idx / G4, x0 = (idx - y * G4) * 4;
            const long long at = band_at(WORDS, y, x0 >> 6);
            const uint32_t tb = (uint32_t)(pl_a[at] >> (x0 & 63)) & 0xFu, wb = (uint32_t)(pl_w[at] >> (x0 & 63)) & 0xFu;
            int32_t v[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = (tb >> c) & 1u ? kEscapeSafe : ((wb >> c) & 1u ? kEscapeLost : kEscapeBlocked);
            int32_t *dst = out + (long long)y * g.W + x0;
            if (a.slack_vec) {
                *reinterpret_cast<int4 *>(dst) = make_int4(v[0], v[1], v[2], v[3]);
            } else {
                const int in = min(4, g.W - x0);
                for (int c = 0; c < in; ++c) dst[c] = v[c];
            }
        }
    }

    // the points: lane t answers point t.  pst: bits 0..7 - neighbour n (move code n + 1; 4..7 the diagonals) is walkable with a deadline
    // > 0 and has not joined yet; kPend: a neighbour may still join; kOk / kTarget: the point is one / stands on a target; kFound: a
    // neighbour has joined - pbest its slack, bits 12..14 its number (the levels fall, so the first is the largest; among those of one
    // level the lowest number).  pd_lo / pd_hi: the neighbours' deadlines, 16 bits each (0xFFFF: NEVER)
    constexpr uint32_t kPend = 1u << 8, kOk = 1u << 9, kTarget = 1u << 10, kFound = 1u << 11;
    const int k = ba.k;
    int px = 0, py = 0, pbest = kEscapeLost;
    uint32_t pst = 0;
    unsigned long long pd_lo = 0, pd_hi = 0;      // neighbours 0..3 / 4..7
    if (t < k) {
        const QueryPoint p = query_point(ba.points, (long long)i * k + t, g.W, g.H);
        px = p.x; py = p.y;
        if (p.ok) {
            pst = kOk;
            if (walk_bit(pl_a, WORDS, py, px)) {
                pst |= kTarget;
            } else {
#pragma unroll 1
                for (int n = 0; n < (conn8 ? 8 : 4); ++n) {       // (a loop, not unrolled: eight divisions in flight would spill)
                    const int nx = px + walk_dx(n), ny = py + walk_dy(n);
                    if (nx < 0 || nx >= g.W || ny < 0 || ny >= g.H) continue;
                    if (walk_bit(pl_a, WORDS, ny, nx)) {      // a target: no higher-numbered neighbour can do better
                        pst |= kFound | (uint32_t)n << 12; pbest = kEscapeSafe;
                        break;
                    } else if (walk_bit(pl_w, WORDS, ny, nx)) {
                        const int D = escape_deadline(mins[ny * g.W + nx], a.horizon, a.margin, a.per_move);
                        if (D > 0) {
                            pst |= 1u << n;
                            const unsigned long long d16 = (unsigned long long)min(D, 0xFFFF) << (16 * (n & 3));
                            if (n < 4) pd_lo |= d16; else pd_hi |= d16;
                        }
                    }
                }
                // (beside a target the point stays pending through the flood only: a NEVER neighbour with a lower number that the
                // flood reaches is SAFE too, and the tie goes to the lowest number)
                if ((pst & 0xFFu) && escape_deadline(mins[py * g.W + px], a.horizon, a.margin, a.per_move) > 0) pst |= kPend;
            }
        }
    }
    __syncthreads();                          // the list and the planes are written, the histogram is read: LDS is free

    // after the flood (v = 0xFFFE, val = SAFE) and after level v (val = v): has a neighbour joined?  No barrier follows a call, though
    // the next level's lanes may already be opening their bucket: those atomics set bits of cells with D <= the next v + 1 <= v, which
    // the test skips (it looks at neighbours with D > v only), and leave every other bit of the word as it is.
    auto test_point = [&](int v, int32_t val) {
        if (!(pst & kPend)) return;
        uint32_t m = pst & 0xFFu;
#pragma unroll 1
        while (m) {
            const int n = __builtin_ctz(m);
            m &= m - 1;
            if ((int)(((n < 4 ? pd_lo : pd_hi) >> (16 * (n & 3))) & 0xFFFFu) <= v) continue;
            const int nx = px + walk_dx(n), ny = py + walk_dy(n);
            const int b = (ny / kBandRows) * WORDS + (nx >> 6);
            const band_word u = RES ? s_u[b * kBandLdsRow + (ny % kBandRows)] : pl_u[(long long)b * kBandRows + (ny % kBandRows)];
            if (!((u >> (nx & 63)) & 1u)) {
                pbest = val; pst = (pst & ~(kPend | 7u << 12)) | kFound | (uint32_t)n << 12;
                break;
            }
        }
    };

    // phase 1: A to registers and U to LDS (k_escape<true>), the halo; then the flood of A through U to its fixed point
    band_word f[kBandRows];
    for (int p = 0; p < passes; ++p) {
        const int b = p * nt + t;
        if (b < nb) {
            int targets = 0;
#pragma unroll
            for (int j = 0; j < kBandRows; ++j) {
                f[j] = band_ref(pl_a, (uint32_t)b * (kBandRows * 8u) + j * 8u);
                if (RES) s_u[t * kBandLdsRow + j] = band_ref(pl_u, (uint32_t)b * (kBandRows * 8u) + j * 8u);
                targets += __popcll(f[j]);
            }
            if (targets) atomicAdd(&s_targets, targets);
            band_publish(RES ? l_top : g_top, RES ? l_bot : g_bot, RES ? l_edge : g_edge, b, f);
        }
    }
    __syncthreads();
    for (;;) {
        int changed = 0;
        for (int p = 0; p < passes; ++p) {
            const int b = p * nt + t;
            const bool on = b < nb;
            const int br = on ? b / WORDS : 0, wi = on ? b - br * WORDS : 0;
            BandHalo h = {};
            if (on) h = band_halo(WORDS, BR, RES ? l_top : g_top, RES ? l_bot : g_bot, RES ? l_edge : g_edge, br, wi);
            __syncthreads();                  // every band of the pass has read its halo: the pass may now publish
            if (on) {
                if (!RES) band_load(f, pl_a, b);
                if (band_round(f, RES ? s_u + t * kBandLdsRow : pl_u + (long long)b * kBandRows, h, conn8)) {
                    changed = 1;
                    if (!RES) band_store(pl_a, b, f);
                    band_publish(RES ? l_top : g_top, RES ? l_bot : g_bot, RES ? l_edge : g_edge, b, f);
                }
            }
            if (!RES) __syncthreads();        // a later pass of the round reads what this one published
        }
        if (!__syncthreads_or(changed)) break;
    }
    // the flooded cells leave U: they are SAFE
    {
        int safe = 0;
        for (int p = 0; p < passes; ++p) {
            const int b = p * nt + t;
            if (b < nb) {
                const int br = b / WORDS, wi = b - br * WORDS;
                band_word *ub = RES ? s_u + t * kBandLdsRow : pl_u + (long long)b * kBandRows;
                if (!RES) band_load(f, pl_a, b);
                const int cell0 = br * kBandRows * g.W + wi * 64;
#pragma unroll
                for (int j = 0; j < kBandRows; ++j) {
                    const band_word u = ub[j], n = f[j] & u;
                    if (n) {
                        ub[j] = u & ~n;
                        safe += __popcll(n);
                        if (out) escape_scatter(out + (cell0 + j * g.W), n, kEscapeSafe);
                    }
                }
            }
        }
        if (safe) atomicAdd(&s_safe, safe);
    }
    __syncthreads();
    test_point(0xFFFE, kEscapeSafe);         // (no barrier behind it: see test_point)
    if (pst & kFound) pst &= ~kPend;          // beside a target, or a flooded cell: SAFE is the most a neighbour can have

    // phase 2: the levels, from the largest deadline down
    int bi = n_buckets - 1;                   // the next bucket to open
    int v = bi >= 0 ? bk_d[bi] - 1 : -1, cur = 0, par = 0;
    bool grew_any = false;                    // some band grew last level
    const int my_br = t < nb ? t / WORDS : 0, my_wi = t < nb ? t - my_br * WORDS : 0;       // k_escape<true>: the thread's band
    while (v >= 0) {
        bool opens = bi >= 0 && bk_d[bi] == v + 1;
        if (!opens && !grew_any) {            // nothing can join before the next bucket opens
            if (bi < 0) break;
            v = bk_d[bi] - 1; opens = true;
        }
        if (RES && t < kBandThreads / 32) s_wake[par ^ 1][t] = 0;         // (read last level; this level's growth writes it behind the barrier)
        if (opens) {
            const int q1 = bk_at[bi + 1];
#pragma unroll 1
            for (int q = bk_at[bi] + t; q < q1; q += nt) {
                const int c = list[q], y = c / g.W, x = c - y * g.W;
                const int b = (y / kBandRows) * WORDS + (x >> 6);
                if (RES) {
                    atomicOr(reinterpret_cast<unsigned long long *>(&s_u[b * kBandLdsRow + (y % kBandRows)]), 1ull << (x & 63));
                    atomicOr(&s_wake[par][b >> 5], 1u << (b & 31));
                } else {
                    atomicOr(reinterpret_cast<unsigned long long *>(&pl_u[(long long)b * kBandRows + (y % kBandRows)]), 1ull << (x & 63));
                }
            }
            --bi;
        }
        int added = 0;
        if (RES) {
            const bool on = t < nb;
            BandHalo h = {};
            if (on) h = band_halo(WORDS, BR, l_top, l_bot, l_edge, my_br, my_wi);
            __syncthreads();                  // the bucket is open and every band has read its halo: the level may now publish
            // a band is live when a cell of it opened this level or when it or a neighbour grew last level
            if (on && ((s_wake[par][t >> 5] >> (t & 31)) & 1u)) {
                const int cell0 = my_br * kBandRows * g.W + my_wi * 64;
                if (band_grow(f, s_u + t * kBandLdsRow, h, conn8, [&](int j, band_word n) {
                        if (out) escape_scatter(out + (cell0 + j * g.W), n, v);
                    })) {
                    added = 1;
                    band_publish(l_top, l_bot, l_edge, t, f);
                    const int c0 = max(my_wi - 1, 0), c1 = min(my_wi + 1, WORDS - 1);
                    for (int r = max(my_br - 1, 0); r <= min(my_br + 1, BR - 1); ++r) {
                        const int lo = r * WORDS + c0;
                        const unsigned long long m = ((1ull << (c1 - c0 + 1)) - 1ull) << (lo & 31);
                        atomicOr(&s_wake[par ^ 1][lo >> 5], (uint32_t)m);
                        if (m >> 32) atomicOr(&s_wake[par ^ 1][(lo >> 5) + 1], (uint32_t)(m >> 32));
                    }
                }
            }
            par ^= 1;
        } else {
            const band_word *top_old = g_top + (long long)cur * nb, *bot_old = g_bot + (long long)cur * nb;
            const uint32_t *edge_old = g_edge + (long long)cur * nb;
            band_word *top_new = g_top + (long long)(cur ^ 1) * nb, *bot_new = g_bot + (long long)(cur ^ 1) * nb;
            uint32_t *edge_new = g_edge + (long long)(cur ^ 1) * nb;
            __syncthreads();                  // the bucket is open
            for (int p = 0; p < passes; ++p) {
                const int b = p * nt + t;
                if (b < nb) {
                    const int br = b / WORDS, wi = b - br * WORDS;
                    const BandHalo h = band_halo(WORDS, BR, top_old, bot_old, edge_old, br, wi);
                    band_load(f, pl_a, b);
                    const int cell0 = br * kBandRows * g.W + wi * 64;
                    if (band_grow(f, pl_u + (long long)b * kBandRows, h, conn8, [&](int j, band_word n) {
                            if (out) escape_scatter(out + (cell0 + j * g.W), n, v);
                        })) {
                        added = 1;
                        band_store(pl_a, b, f);
                    }
                    band_publish(top_new, bot_new, edge_new, b, f);
                }
            }
            cur ^= 1;
        }
        grew_any = __syncthreads_or(added) != 0;
        test_point(v, v);                     // (no barrier behind it: see test_point)
        --v;
    }

    // epilogue
    {                                         // the cells of A: the targets, the flooded cells and what the levels added
        int cells = 0;
        for (int p = 0; p < passes; ++p) {
            const int b = p * nt + t;
            if (b < nb) {
                if (!RES) band_load(f, pl_a, b);
#pragma unroll
                for (int j = 0; j < kBandRows; ++j) cells += __popcll(f[j]);
            }
        }
        if (cells) atomicAdd(&s_set, cells);
    }
    if (t < k) {
        int32_t val = kEscapeBlocked, step = -1;
        if (pst & kOk) {
            step = 0;
            if (pst & kTarget) {
                val = kEscapeSafe;
            } else if (pst & kFound) {
                const int D = escape_deadline(mins[py * g.W + px], a.horizon, a.margin, a.per_move);
                const int32_t own = D == kEscapeNever ? kEscapeSafe : D - 1, via = pbest == kEscapeSafe ? kEscapeSafe : pbest - 1;
                val = max(min(own, via), kEscapeLost);
                if (val >= 0 && val < kEscapeSafe && !conn8) step = (int32_t)((pst >> 12) & 7u) + 1;
            } else {
                val = kEscapeLost;
            }
        }
        if (a.point_slack) a.point_slack[(long long)i * k + t] = val;
        if (a.point_step) a.point_step[(long long)i * k + t] = step;
    }
    __syncthreads();
    if (t == 0) {
        if (a.safe) a.safe[i] = s_safe;
        const int esc = s_set - s_targets - s_safe;
        if (a.escapable) a.escapable[i] = esc;
        if (a.lost) a.lost[i] = s_walkable - s_safe - esc;
        if (a.top) a.top[i] = s_top;
    }
}

}  // namespace
