// Reach of the fire (sf_reach): the flood fill of the seed cells (status selected by source_mask) through the
// open cells (status selected by through_mask, and passable) - every cell the fire can still get to.  The reference has nothing of
// the kind.  One bit per cell, 64 cells per word, ceil(P / 64) words per row; ONE workgroup per listed environment, resident until
// that environment's fixed point - no workgroup ever waits for another.  A thread owns a BAND: one word column times kReachRows
// consecutive rows.  The plane that is filled is F = seeds | reach (seeds are never open, so reach = F & open); a round is, per band,
// a Gauss-Seidel sweep down and one up with the band's F in registers and its open words in the thread's own LDS row - row y takes
// spread(row y -+ 1) & open, then fills along the row with one 64-bit add per direction - and between rounds the band's first and
// last row and its first and last column go to the neighbouring bands through a halo (three arrays: top / bottom words, edge
// columns).  k_reach<true>: the grid has at most one band per thread - F stays in registers and open in LDS for the whole fill, the
// halo is LDS.  k_reach<false>: larger grids - the two bit planes and the halo live in the handle's scratch (L2), and the workgroup
// walks the bands in passes of 1024 inside every round (a pass loads its bands' F to registers and open to LDS).  The staging writes
// both planes to the scratch first, so that no more than one word's status vectors are in flight per thread.  The epilogue (same
// kernel) counts, sums the value plane, writes the byte mask and tests the points from the final bit plane.
// Zero scratch memory and zero spills at 1024 threads x 128 VGPRs hang on two things: scheduling barriers every two rows of a sweep
// (without them the scheduler hoists every row's LDS read and bit reversal to the top of the unrolled sweep), and 32-bit byte offsets
// from uniform bases (reach_ref) instead of a 64-bit address per access.
// Part of the single translation unit simfire_hip.hip.  The status bytes are read from whichever cell plane is current; nothing but
// the scratch and the outputs is written.
#pragma once
#include "sf_query_dev.h"

namespace {

constexpr int kReachThreads = 1024;
constexpr int kReachRows = 16;                // rows of a band: its F is 16 x 2 = 32 VGPRs
constexpr int kReachMaxWidth = 8192;          // wider grids are refused (as sf_distance does)
constexpr long long kReachScratchDefault = 256ll << 20;     // bytes of scratch a call uses unless it names a budget

typedef unsigned long long reach_word;

struct ReachArgs {
    Geo g;
    CellPlanes pl;               // the status bytes, in whichever plane is current
    const int32_t *envs;         // the listed environments of this chunk [cn]
    const uint8_t *passable;     // dense u8 [H * W] (pass_env = 0) or [E][H * W], or null
    long long pass_env;
    int pass_vec;                // 16-byte loads of passable (W % 16 == 0 and an aligned plane)
    const int32_t *vals;         // the value plane int32 [1 or E][H][P], or null (no value output)
    long long val_env;
    const int32_t *points;       // this chunk's [cn][k][3] (column, row, id), or null
    int k;
    uint8_t *scratch;            // [cn][scratch_env]: F plane | open plane | halo top | halo bottom | halo edges
    long long scratch_env;
    int32_t *count;              // this chunk's part of the outputs (null: not asked for)
    long long *value;
    uint8_t *mask;
    int32_t *seeds;
    int32_t *point_in;
    int32_t *rounds;
    uint32_t slo, shi, tlo, thi; // source_mask / through_mask as tables of one byte permute (mask_sel01)
    int conn8, max_rounds;
    int WORDS, BR, nb;           // words per row, band rows = ceil(H / kReachRows), bands = BR * WORDS
    int mask_vec;                // 16-byte stores of the mask (W % 16 == 0 and an aligned output)
};

__host__ __device__ inline int reach_words(const Geo &g) { return (g.P + 63) / 64; }
__host__ __device__ inline int reach_band_rows(const Geo &g) { return (g.H + kReachRows - 1) / kReachRows; }
// bytes of scratch per listed environment: two bit planes of BR * kReachRows rows, two halo words and one edge dword per band
__host__ __device__ inline long long reach_env_bytes(const Geo &g)
{
    const long long nb = (long long)reach_band_rows(g) * reach_words(g);
    return (nb * kReachRows * 16 + nb * 20 + 255) / 256 * 256;
}

// Where word wi of row y lies in a bit plane: band-major - the 16 words of a band (one word column, 16 rows) are neighbours, so a
// thread reads and writes its band with 16-byte accesses at constant offsets from one address
__device__ __forceinline__ long long reach_at(int WORDS, int y, int wi)
{
    return ((long long)(y / kReachRows) * WORDS + wi) * kReachRows + (y % kReachRows);
}

// 0/1 per byte of the 16 passable bytes of vector v in row y (cells past the width: 0)
__device__ __forceinline__ uint4 reach_passable01(const ReachArgs &a, int e, int y, int v)
{
    return nz01x16(dense_vec16(a.passable + a.pass_env * e, a.pass_vec, a.g.W, y, v));
}

// The seed and the open bits of word wi of row y: four status vectors, both masks (mask_sel01), the on-grid mask, passable; rows
// past the height, vectors past the pitch and the pitch padding give 0.
__device__ __forceinline__ void reach_stage(const ReachArgs &a, int e, int y, int wi, reach_word &sd, reach_word &op)
{
    const Geo &g = a.g;
    sd = 0; op = 0;
    if (y >= g.H) return;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int v = wi * 4 + q;
        if (v >= g.PV) break;
        const uint4 s = and4(*reinterpret_cast<const uint4 *>(cell_status_vec(a.pl, g, e, y, v)), 0x07070707u);
        const uint4 on = first01x16(g.W - v * 16);
        const uint32_t sb = pack16(and44(mask_sel01(a.slo, a.shi, s), on));
        uint4 o = and44(mask_sel01(a.tlo, a.thi, s), on);
        if (a.passable) o = and44(o, reach_passable01(a, e, y, v));
        sd |= (reach_word)sb << (16 * q);
        op |= (reach_word)pack16(o) << (16 * q);
    }
}

// What row y takes from a neighbouring row w: the row itself, and with diagonals its two shifts - l / r: bit 63 of the word to the
// left / bit 0 of the word to the right of w
__device__ __forceinline__ reach_word reach_spread(reach_word w, reach_word l, reach_word r, int conn8)
{
    return conn8 ? (w | (w << 1) | (w >> 1) | l | (r << 63)) : w;
}
// The fill along a row inside one word: every run of open bits that holds or touches a bit of w is filled.  Towards the higher bits
// the carry of ONE add runs through a run of open bits (o + G clears the run from the generator up; the generators themselves are
// or-ed back in); towards the lower bits the same on the reversed words.  cl / cr: the neighbouring words' bit 63 / bit 0.
__device__ __forceinline__ reach_word reach_fill(reach_word w, reach_word o, reach_word cl, reach_word cr)
{
    const reach_word gu = (w | (w << 1) | cl) & o;
    w |= (((o + gu) ^ o) & o) | gu;
    const reach_word gd = (w | (w >> 1) | (cr << 63)) & o;
    const reach_word ro = __brevll(o), rg = __brevll(gd);
    w |= __brevll(((ro + rg) ^ ro) & ro) | gd;
    return w;
}
// bit 0 of the band's rows in bits 0..15, bit 63 of them in bits 16..31
__device__ __forceinline__ uint32_t reach_edges(const reach_word (&f)[kReachRows])
{
    uint32_t ed = 0;
#pragma unroll
    for (int j = 0; j < kReachRows; ++j) ed |= ((uint32_t)f[j] & 1u) << j | (uint32_t)(f[j] >> 63) << (16 + j);
    return ed;
}

// base[bytes / sizeof(T)] with a 32-bit byte offset (a plane of one environment is far below 4 GiB): one uniform base and one
// 32-bit register per access instead of a 64-bit address each
template <class T> __device__ __forceinline__ T &reach_ref(T *base, uint32_t bytes) { return *(T *)((char *)base + bytes); }

struct ReachHalo {           // what band (br, wi) reads of its eight neighbours: 0 past the grid
    reach_word top, bot;     // the row above its first / below its last row, its own word column
    uint32_t el, er;         // rows -1 .. 16 of the column to its left (bit 63 of that word) / to its right (bit 0): bit j + 1 = row j
};
__device__ __forceinline__ ReachHalo reach_halo(int WORDS, int BR, const reach_word *h_top, const reach_word *h_bot, const uint32_t *h_edge, int br, int wi)
{
    const int b = br * WORDS + wi;
    const bool up = br > 0, dn = br + 1 < BR, lf = wi > 0, rt = wi + 1 < WORDS;
    ReachHalo h;
    const uint32_t b8 = (uint32_t)b * 8u, W8 = (uint32_t)WORDS * 8u;
    h.top = up ? reach_ref(h_bot, b8 - W8) : 0;
    h.bot = dn ? reach_ref(h_top, b8 + W8) : 0;
    const uint32_t edl = lf ? reach_ref(h_edge, (uint32_t)b * 4u - 4u) : 0, edr = rt ? reach_ref(h_edge, (uint32_t)b * 4u + 4u) : 0;
    const reach_word tl = up && lf ? reach_ref(h_bot, b8 - W8 - 8u) : 0, tr = up && rt ? reach_ref(h_bot, b8 - W8 + 8u) : 0;
    const reach_word bl = dn && lf ? reach_ref(h_top, b8 + W8 - 8u) : 0, brw = dn && rt ? reach_ref(h_top, b8 + W8 + 8u) : 0;
    h.el = (edl >> 16) << 1 | (uint32_t)(tl >> 63) | (uint32_t)(bl >> 63) << 17;
    h.er = (edr & 0xFFFFu) << 1 | ((uint32_t)tr & 1u) | ((uint32_t)brw & 1u) << 17;
    return h;
}

// One round of a band: the sweep down, the sweep up.  The band's open words are read where they are used (ob[j]: LDS, or the
// scratch plane) - only F stays in registers.  Returns whether a bit was added.
__device__ __forceinline__ bool reach_round(reach_word (&f)[kReachRows], const reach_word *ob, const ReachHalo &h, int conn8)
{
    reach_word changed = 0;
#pragma unroll
    for (int j = 0; j < kReachRows; ++j) {
        const reach_word o = ob[j];
        const reach_word prev = j == 0 ? h.top : f[j - 1];
        reach_word w = f[j] | (reach_spread(prev, (h.el >> j) & 1u, (h.er >> j) & 1u, conn8) & o);
        w = reach_fill(w, o, (h.el >> (j + 1)) & 1u, (h.er >> (j + 1)) & 1u);
        changed |= w ^ f[j];
        f[j] = w;
        if (j & 1) __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int j = kReachRows - 1; j >= 0; --j) {
        const reach_word o = ob[j];
        const reach_word next = j == kReachRows - 1 ? h.bot : f[j + 1];
        reach_word w = f[j] | (reach_spread(next, (h.el >> (j + 2)) & 1u, (h.er >> (j + 2)) & 1u, conn8) & o);
        w = reach_fill(w, o, (h.el >> (j + 1)) & 1u, (h.er >> (j + 1)) & 1u);
        changed |= w ^ f[j];
        f[j] = w;
        if (j & 1) __builtin_amdgcn_sched_barrier(0);
    }
    return changed != 0;
}

// dynamic LDS of k_reach with nt threads: the open words [nt][kReachLdsRow] - a thread's 16 words and one of padding, so that the
// 8-byte reads of the lanes of a wave fall on all banks - and, in k_reach<true>, the halo top [nt], bottom [nt], edges [nt]
constexpr int kReachLdsRow = kReachRows + 1;
__host__ __device__ inline size_t reach_lds_bytes(int nt, bool resident) { return (size_t)nt * (kReachLdsRow * 8 + (resident ? 8 + 8 + 4 : 0)); }

template <bool RES>
__global__ __launch_bounds__(kReachThreads) void k_reach(const ReachArgs *__restrict__ ap)
{
    extern __shared__ __attribute__((aligned(16))) reach_word s_reach[];      // reach_lds_bytes(nt, RES)
    __shared__ int s_count, s_seeds;
    __shared__ long long s_value;
    // (the arguments lie in the call block, not in the kernel's argument segment: a field is loaded where it is used, and what only
    // the staging or the epilogue needs holds no scalar register during the fill)
    const ReachArgs &a = *ap;
    const Geo &g = a.g;
    const int t = threadIdx.x, nt = blockDim.x;
    const int i = blockIdx.x, e = a.envs[i];
    const int WORDS = a.WORDS, BR = a.BR, nb = a.nb, conn8 = a.conn8, max_rounds = a.max_rounds;
    const long long plane_words = (long long)nb * kReachRows;
    reach_word *pl_f = reinterpret_cast<reach_word *>(a.scratch + (long long)i * a.scratch_env);
    reach_word *pl_o = pl_f + plane_words;
    reach_word *s_open = s_reach;
    reach_word *h_top = RES ? s_reach + kReachLdsRow * nt : pl_o + plane_words;
    reach_word *h_bot = h_top + (RES ? nt : nb);
    uint32_t *h_edge = reinterpret_cast<uint32_t *>(h_bot + (RES ? nt : nb));
    const int passes = RES ? 1 : (nb + nt - 1) / nt;
    if (t == 0) { s_count = 0; s_seeds = 0; s_value = 0; }

    // staging: a word per thread and turn (neighbouring threads, neighbouring words of a row) into the two planes of the scratch - the
    // status vectors of ONE word in flight per thread, not those of a band -, then every band's rows from there, and its halo
#pragma unroll 1
    for (int idx = t; idx < nb * kReachRows; idx += nt) {
        const int y = idx / WORDS, wi = idx - y * WORDS;
        reach_word sd, op;
        reach_stage(a, e, y, wi, sd, op);
        pl_f[reach_at(WORDS, y, wi)] = sd; pl_o[reach_at(WORDS, y, wi)] = op;
    }
    __syncthreads();
    reach_word fres[RES ? kReachRows : 1];        // k_reach<true>: the band's F for the whole fill
    for (int p = 0; p < passes; ++p) {
        const int b = p * nt + t;
        if (b < nb) {
            reach_word fpass[RES ? 1 : kReachRows];
            reach_word (&f)[kReachRows] = *reinterpret_cast<reach_word (*)[kReachRows]>(RES ? fres : fpass);
#pragma unroll
            for (int j = 0; j < kReachRows; ++j) {
                f[j] = reach_ref(pl_f, (uint32_t)b * (kReachRows * 8u) + j * 8u);
                if (RES) s_open[t * kReachLdsRow + j] = reach_ref(pl_o, (uint32_t)b * (kReachRows * 8u) + j * 8u);
            }
            reach_ref(h_top, (uint32_t)b * 8u) = f[0]; reach_ref(h_bot, (uint32_t)b * 8u) = f[kReachRows - 1]; reach_ref(h_edge, (uint32_t)b * 4u) = reach_edges(f);
        }
    }
    __syncthreads();

    // the fill: rounds until no band adds a bit (or max_rounds)
    int rounds = 0;
    bool fixed = false;
    for (;;) {
        ++rounds;
        int changed = 0;
        for (int p = 0; p < passes; ++p) {
            const int b = p * nt + t;
            const bool on = b < nb;
            const int br = on ? b / WORDS : 0, wi = on ? b - br * WORDS : 0;
            ReachHalo h = {};
            if (on) h = reach_halo(WORDS, BR, h_top, h_bot, h_edge, br, wi);
            __syncthreads();                  // every band of the pass has read its halo: the pass may now publish
            if (on) {
                reach_word fpass[RES ? 1 : kReachRows];
                reach_word (&f)[kReachRows] = *reinterpret_cast<reach_word (*)[kReachRows]>(RES ? fres : fpass);
                const reach_word *ob = s_open + t * kReachLdsRow;
                if (!RES) {                   // the band's open words go to the thread's own LDS row, as in k_reach<true>; F to registers
#pragma unroll
                    for (int j = 0; j < kReachRows; ++j) s_open[t * kReachLdsRow + j] = reach_ref(pl_o, (uint32_t)b * (kReachRows * 8u) + j * 8u);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int j = 0; j < kReachRows; ++j) f[j] = reach_ref(pl_f, (uint32_t)b * (kReachRows * 8u) + j * 8u);
                }
                if (reach_round(f, ob, h, conn8)) {
                    changed = 1;
                    if (!RES) {
#pragma unroll
                        for (int j = 0; j < kReachRows; ++j) reach_ref(pl_f, (uint32_t)b * (kReachRows * 8u) + j * 8u) = f[j];
                    }
                    reach_ref(h_top, (uint32_t)b * 8u) = f[0]; reach_ref(h_bot, (uint32_t)b * 8u) = f[kReachRows - 1]; reach_ref(h_edge, (uint32_t)b * 4u) = reach_edges(f);
                }
            }
            if (!RES) __syncthreads();        // a later pass of the round reads what this one published
        }
        if (!__syncthreads_or(changed)) { fixed = true; break; }
        if (rounds == max_rounds) break;
    }

    // epilogue: counts from the bands; the reach plane F & open for what reads single cells
    const bool plane = a.mask || a.value || a.point_in;
    int cnt = 0, sds = 0;
    for (int p = 0; p < passes; ++p) {
        const int b = p * nt + t;
        if (b < nb) {
            reach_word fpass[RES ? 1 : kReachRows];
            reach_word (&f)[kReachRows] = *reinterpret_cast<reach_word (*)[kReachRows]>(RES ? fres : fpass);
#pragma unroll
            for (int j = 0; j < kReachRows; ++j) {
                const uint32_t at = (uint32_t)b * (kReachRows * 8u) + j * 8u;
                if (!RES) f[j] = reach_ref(pl_f, at);
                const reach_word o = RES ? s_open[t * kReachLdsRow + j] : reach_ref(pl_o, at);
                cnt += __popcll(f[j] & o);
                sds += __popcll(f[j] & ~o);
                if (plane) reach_ref(pl_f, at) = f[j] & o;
            }
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { cnt += __shfl_xor(cnt, m); sds += __shfl_xor(sds, m); }
    if ((t & 63) == 0) { atomicAdd(&s_count, cnt); atomicAdd(&s_seeds, sds); }
    __syncthreads();                          // (the plane is written, too)

    if (a.value) {                            // a wave per word that has a bit: lane = cell
        long long sum = 0;
        const int32_t *vals = a.vals + a.val_env * e;
        const int lane = t & 63;
        for (int idx = t >> 6; idx < g.H * WORDS; idx += nt >> 6) {
            const int y = idx / WORDS, wi = idx - y * WORDS;
            const reach_word w = pl_f[reach_at(WORDS, y, wi)];
            if (w) {
                if ((w >> lane) & 1u) sum += vals[(long long)y * g.P + wi * 64 + lane];
            }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m);
        if (lane == 0 && sum) atomicAdd(reinterpret_cast<unsigned long long *>(&s_value), (unsigned long long)sum);
    }
    if (a.mask) {                             // 16 cells per turn
        const int G16 = (g.W + 15) / 16;
        uint8_t *out = a.mask + (long long)i * g.H * g.W;
        for (int idx = t; idx < g.H * G16; idx += nt) {
            const int y = idx / G16, q = idx - y * G16;
            const uint32_t bits = (uint32_t)(pl_f[reach_at(WORDS, y, q >> 2)] >> (16 * (q & 3))) & 0xFFFFu;
            uint32_t d[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const uint32_t n4 = (bits >> (4 * c)) & 0xFu;
                d[c] = (n4 | n4 << 7 | n4 << 14 | n4 << 21) & 0x01010101u;
            }
            uint8_t *dst = out + (long long)y * g.W + q * 16;
            if (a.mask_vec) {
                *reinterpret_cast<uint4 *>(dst) = make_uint4(d[0], d[1], d[2], d[3]);
            } else {
                const int in = min(16, g.W - q * 16);
                for (int c = 0; c < in; ++c) dst[c] = (uint8_t)((bits >> c) & 1u);
            }
        }
    }
    if (a.point_in) {
        for (int j = t; j < a.k; j += nt) {
            const QueryPoint p = query_point(a.points, (long long)i * a.k + j, g.W, g.H);
            int32_t val = -1;
            if (p.ok) val = (int32_t)((pl_f[reach_at(WORDS, p.y, p.x >> 6)] >> (p.x & 63)) & 1u);
            a.point_in[(long long)i * a.k + j] = val;
        }
    }
    __syncthreads();
    if (t == 0) {
        if (a.count) a.count[i] = s_count;
        if (a.seeds) a.seeds[i] = s_seeds;
        if (a.value) a.value[i] = s_value;
        if (a.rounds) a.rounds[i] = fixed ? rounds : -rounds;
    }
}

}  // namespace
