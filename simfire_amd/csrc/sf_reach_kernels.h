// Reach of the fire (sf_reach): the flood fill of the seed cells (status selected by source_mask) through the
// open cells (status selected by through_mask, and passable) - every cell the fire can still get to.  The reference has nothing of
// the kind.  The bit planes, the bands, the halo and the round of a band are sf_bands.h; ONE workgroup per listed environment,
// resident until that environment's fixed point - no workgroup ever waits for another.  The plane that is filled is F = seeds | reach
// (seeds are never open, so reach = F & open).  k_reach<true>: the grid has at most one band per thread - F stays in registers and
// open in the thread's own LDS row for the whole fill, the halo is LDS.  k_reach<false>: larger grids - the two bit planes and the
// halo live in the handle's scratch (L2), and the workgroup walks the bands in passes of 1024 inside every round (a pass loads its
// bands' F to registers and open to LDS).  The staging writes both planes to the scratch first, so that no more than one word's
// status vectors are in flight per thread.  The epilogue (same kernel) counts, sums the value plane, writes the byte mask and tests
// the points from the final bit plane.  Zero scratch memory and zero spills at 1024 threads x 128 VGPRs.
// Part of the single translation unit simfire_hip.hip.  The status bytes are read from whichever cell plane is current; nothing but
// the scratch and the outputs is written.
#pragma once
#include "sf_bands.h"
#include "sf_query_dev.h"

namespace {

constexpr int kReachMaxWidth = 8192;          // wider grids are refused (as sf_distance does)
constexpr long long kReachScratchDefault = 256ll << 20;     // bytes of scratch a call uses unless it names a budget

struct ReachArgs {
    BandArgs band;               // slo / shi: source_mask, tlo / thi: through_mask; scratch: F plane | open plane | halo top | bottom | edges
    const int32_t *vals;         // the value plane int32 [1 or E][H][P], or null (no value output)
    long long val_env;
    int32_t *count;              // this chunk's part of the outputs (null: not asked for)
    long long *value;
    uint8_t *mask;
    int32_t *seeds;
    int32_t *point_in;
    int32_t *rounds;
    int max_rounds;
    int mask_vec;                // 16-byte stores of the mask (W % 16 == 0 and an aligned output)
};

// bytes of scratch per listed environment: two bit planes and one halo
__host__ __device__ inline long long reach_env_bytes(const Geo &g) { return band_env_bytes((long long)band_rows(g.H) * band_words(g.P), 2, 1); }

// dynamic LDS of k_reach with nt threads: the open words [nt][kBandLdsRow] and, in k_reach<true>, the halo top [nt], bottom [nt], edges [nt]
__host__ __device__ inline size_t reach_lds_bytes(int nt, bool resident) { return (size_t)nt * (kBandLdsRow * 8 + (resident ? 8 + 8 + 4 : 0)); }

template <bool RES>
__global__ __launch_bounds__(kBandThreads) void k_reach(const ReachArgs *__restrict__ ap)
{
    extern __shared__ __attribute__((aligned(16))) band_word s_reach[];       // reach_lds_bytes(nt, RES)
    __shared__ int s_count, s_seeds;
    __shared__ long long s_value;
    // (the arguments lie in the call block, not in the kernel's argument segment: a field is loaded where it is used, and what only
    // the staging or the epilogue needs holds no scalar register during the fill)
    const ReachArgs &a = *ap;
    const BandArgs &ba = a.band;
    const Geo &g = ba.g;
    const int t = threadIdx.x, nt = blockDim.x;
    const int i = blockIdx.x, e = ba.envs[i];
    const int WORDS = ba.WORDS, BR = ba.BR, nb = ba.nb, conn8 = ba.conn8, max_rounds = a.max_rounds;
    const long long plane_words = (long long)nb * kBandRows;
    band_word *pl_f = reinterpret_cast<band_word *>(ba.scratch + (long long)i * ba.scratch_env);
    band_word *pl_o = pl_f + plane_words;
    band_word *s_open = s_reach;
    band_word *h_top = RES ? s_reach + kBandLdsRow * nt : pl_o + plane_words;
    band_word *h_bot = h_top + (RES ? nt : nb);
    uint32_t *h_edge = reinterpret_cast<uint32_t *>(h_bot + (RES ? nt : nb));
    const int passes = RES ? 1 : (nb + nt - 1) / nt;
    if (t == 0) { s_count = 0; s_seeds = 0; s_value = 0; }

    // staging: a word per thread and turn (neighbouring threads, neighbouring words of a row) into the two planes of the scratch - the
    // status vectors of ONE word in flight per thread, not those of a band -, then every band's rows from there, and its halo
#pragma unroll 1
    for (int idx = t; idx < nb * kBandRows; idx += nt) {
        const int y = idx / WORDS, wi = idx - y * WORDS;
        band_word sd, op;
        band_stage(ba, e, y, wi, nullptr, 0, sd, op);
        pl_f[band_at(WORDS, y, wi)] = sd; pl_o[band_at(WORDS, y, wi)] = op;
    }
    __syncthreads();
    band_word f[kBandRows];                       // the band's F: k_reach<true> for the whole fill, k_reach<false> that of the pass
    for (int p = 0; p < passes; ++p) {
        const int b = p * nt + t;
        if (b < nb) {
#pragma unroll
            for (int j = 0; j < kBandRows; ++j) {     // (written out: as two band_load the fill loop of k_reach<true> recomputes its halo addresses every round)
                f[j] = band_ref(pl_f, (uint32_t)b * (kBandRows * 8u) + j * 8u);
                if (RES) s_open[t * kBandLdsRow + j] = band_ref(pl_o, (uint32_t)b * (kBandRows * 8u) + j * 8u);
            }
            band_publish(h_top, h_bot, h_edge, b, f);
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
            BandHalo h = {};
            if (on) h = band_halo(WORDS, BR, h_top, h_bot, h_edge, br, wi);
            __syncthreads();                  // every band of the pass has read its halo: the pass may now publish
            if (on) {
                band_word *ob = s_open + t * kBandLdsRow;
                if (!RES) {                   // the band's open words go to the thread's own LDS row, as in k_reach<true>; F to registers
                    band_load(ob, pl_o, b);
                    __builtin_amdgcn_sched_barrier(0);
                    band_load(f, pl_f, b);
                }
                if (band_round(f, ob, h, conn8)) {
                    changed = 1;
                    if (!RES) band_store(pl_f, b, f);
                    band_publish(h_top, h_bot, h_edge, b, f);
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
#pragma unroll
            for (int j = 0; j < kBandRows; ++j) {
                const uint32_t at = (uint32_t)b * (kBandRows * 8u) + j * 8u;
                if (!RES) f[j] = band_ref(pl_f, at);
                const band_word o = RES ? s_open[t * kBandLdsRow + j] : band_ref(pl_o, at);
                cnt += __popcll(f[j] & o);
                sds += __popcll(f[j] & ~o);
                if (plane) band_ref(pl_f, at) = f[j] & o;
            }
        }
    }
    cnt = wave_sum(cnt); sds = wave_sum(sds);
    if ((t & 63) == 0) { atomicAdd(&s_count, cnt); atomicAdd(&s_seeds, sds); }
    __syncthreads();                          // (the plane is written, too)

    if (a.value) {                            // a wave per word that has a bit: lane = cell
        long long sum = 0;
        const int32_t *vals = a.vals + a.val_env * e;
        const int lane = t & 63;
        for (int idx = t >> 6; idx < g.H * WORDS; idx += nt >> 6) {
            const int y = idx / WORDS, wi = idx - y * WORDS;
            const band_word w = pl_f[band_at(WORDS, y, wi)];
            if (w) {
                if ((w >> lane) & 1u) sum += vals[(long long)y * g.P + wi * 64 + lane];
            }
        }
        sum = wave_sum(sum);
        if (lane == 0 && sum) atomicAdd(reinterpret_cast<unsigned long long *>(&s_value), (unsigned long long)sum);
    }
    if (a.mask) {                             // 16 cells per turn
        const int G16 = (g.W + 15) / 16;
        uint8_t *out = a.mask + (long long)i * g.H * g.W;
        for (int idx = t; idx < g.H * G16; idx += nt) {
            const int y = idx / G16, q = idx - y * G16;
            const uint32_t bits = (uint32_t)(pl_f[band_at(WORDS, y, q >> 2)] >> (16 * (q & 3))) & 0xFFFFu;
            uint32_t d[4];                    // (shifts, not bits_bytes16: with its multiply here the scheduler reorders rows of the fill loop)
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
        for (int j = t; j < ba.k; j += nt) {
            const QueryPoint p = query_point(ba.points, (long long)i * ba.k + j, g.W, g.H);
            int32_t val = -1;
            if (p.ok) val = (int32_t)((pl_f[band_at(WORDS, p.y, p.x >> 6)] >> (p.x & 63)) & 1u);
            a.point_in[(long long)i * ba.k + j] = val;
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
