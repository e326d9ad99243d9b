// Connected components (sf_components): the selected cells of an environment fall into maximal 4- or 8-connected
// sets, numbered 1..C by the row-major index of their first cell.  The answer is a partition, so nothing here dilates a bit plane
// (sf_bands.h): the work is a union-find over a label plane of one int32 per cell - the caller's labels output where that is asked
// for, else scratch - that holds a parent index y * W + x, or -1 where the cell is not selected.  The arithmetic is sf_components.h's,
// shared with tests/components_check.cpp.  Separate launches on the handle's stream, chunk by chunk; no workgroup waits for another:
//   k_comp_stage    a wave per row: the selected bits of the row (status mask and member plane), kept as a bit plane; every cell's
//                   first parent is the first cell of its horizontal run - bit arithmetic inside a word, one ballot across the words
//                   of a row -, so horizontal connectivity costs no atomic.  The selected cells counted.
//   k_comp_merge    a thread per word: a union only where a contact with the row above BEGINS (cc_contacts).  Lock-free (cc_unite):
//                   EVERY access to the label plane in this launch is an agent-scope atomic, loads included - workgroups on different
//                   XCDs share no L2 and a plain load may be served from a CU's L1.  A stale parent is still an ancestor, and the
//                   atomic minimum on a root either links it or reports who did; that is the whole correctness argument.  find halves
//                   paths with the same atomic minimum (a grandparent is an ancestor too), which keeps later walks short.
//   k_comp_heads    a thread per word: the first cell of every run takes its root (the only cells that can have become non-trivial).
//   k_comp_flatten  a wave per row: every other cell takes its run head's root, one hop; roots (parent == self) counted per row.  It and
//                   k_comp_assign skip the words of the bit plane that are 0.
//   k_comp_scan     a workgroup per environment: the rows' root counts become exclusive sums; count = their total.
//   k_comp_assign   a wave per row: a root's rank = its row's sum + the roots before it in the row, kept at the root's slot of the
//                   second plane; first[rank] = the root, which IS the component's first cell (the smallest index).
//   k_comp_relabel  every cell: label = rank of its root + 1, or 0; four cells per thread with 16-byte accesses where H * W % 4 == 0.
//   k_comp_stats    a thread per word, one turn per run: sizes of ALL components at slot label - 1 of the second plane (its first C
//                   slots zeroed behind k_comp_relabel by k_comp_zero), and cells / value / bbox / touch of the first max_components - integer atomics, one per run.
//   k_comp_largest  the maximum of (cells, lower number) over all C sizes: one 64-bit integer atomic per wave.
//   k_comp_finish   largest decoded, the label under each point.
// Arguments travel in the call block; nothing but the scratch and the outputs is written.  Part of the single translation unit
// simfire_hip.hip.
#pragma once
#include "sf_components.h"
#include "sf_query_dev.h"

namespace {

constexpr int kCompThreads = 256;
constexpr int kCompMaxWidth = 8192;                    // wider grids are refused (as the other queries do)
constexpr long long kCompScratchDefault = 3ll << 30;   // 256 environments of 1024 x 1024 are one chunk
static_assert(kCompMaxCap == SF_COMPONENTS_MAX, "the header's cap is the ABI's");

struct CompArgs {
    CellGeo g;
    CellPlanes pl;               // the status bytes, in whichever plane is current
    const int32_t *envs;         // the listed environments of this chunk [cn]
    const uint8_t *member;       // dense u8 [H * W] (mem_env = 0) or [E][H * W], or null
    long long mem_env;
    int mem_vec;                 // 16-byte loads of member (W % 16 == 0 and an aligned plane)
    uint32_t tlo, thi;           // select_mask as the table of one byte permute
    int conn8, WORDS, cap, k;
    uint8_t *scratch;            // [cn][scratch_env]: head | bits | rows | second plane | label plane (unless labels is)
    long long scratch_env, o_rows, o_aux, o_par;
    const int32_t *vals;         // the value plane int32 [1 or E][H][P], or null (no value output)
    long long val_env;
    const int32_t *points;       // this chunk's [cn][k][3] (column, row, id), or null
    int32_t *count, *selected, *labels, *cells;      // this chunk's part of the outputs (null: not asked for)
    long long *value;
    int32_t *first, *bbox, *touch, *largest, *point_label;
    int lab_vec;                 // 16-byte accesses of the label plane
};

__device__ __forceinline__ uint8_t *comp_env(const CompArgs &a, int i) { return a.scratch + (long long)i * a.scratch_env; }
__device__ __forceinline__ cc_word *comp_key(const CompArgs &a, int i) { return reinterpret_cast<cc_word *>(comp_env(a, i) + 8); }
__device__ __forceinline__ cc_word *comp_bits(const CompArgs &a, int i) { return reinterpret_cast<cc_word *>(comp_env(a, i) + cc_off_bits()); }
__device__ __forceinline__ int32_t *comp_rows(const CompArgs &a, int i) { return reinterpret_cast<int32_t *>(comp_env(a, i) + a.o_rows); }
__device__ __forceinline__ int32_t *comp_aux(const CompArgs &a, int i) { return reinterpret_cast<int32_t *>(comp_env(a, i) + a.o_aux); }
__device__ __forceinline__ int32_t *comp_lab(const CompArgs &a, int i)
{
    return a.labels ? a.labels + (long long)i * a.g.H * a.g.W : reinterpret_cast<int32_t *>(comp_env(a, i) + a.o_par);
}

// the label plane as cc_find / cc_unite take it: agent-scope atomics only
struct CompPlane {
    int32_t *p;
    __device__ __forceinline__ int load(int i) const { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ int fetch_min(int i, int v) const { return __hip_atomic_fetch_min(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ void store(int i, int v) const { __hip_atomic_store(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};
// the selected bits of word wi of row y of environment e: four status vectors through the mask, and the member plane
__device__ __forceinline__ cc_word comp_select(const CompArgs &a, int e, int y, int wi)
{
    cc_word w = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int v = wi * 4 + q;
        if (v >= a.g.PV || v * 16 >= a.g.W) break;
        uint32_t b = mask_bits16(a.tlo, a.thi, status_vec7(a.pl, a.g, e, y, v), a.g.W - v * 16);
        if (a.member) b &= dense_bits16(a.member + a.mem_env * e, a.mem_vec, a.g.W, y, v);
        w |= (cc_word)b << (16 * q);
    }
    return w;
}

__global__ __launch_bounds__(kCompThreads) void k_comp_stage(const CompArgs *__restrict__ ap)
{
    const CompArgs &a = *ap;
    const int i = blockIdx.y, e = a.envs[i], lane = threadIdx.x & 63, y = blockIdx.x * (kCompThreads / 64) + (threadIdx.x >> 6);
    const int W = a.g.W;
    if (y >= a.g.H) return;                            // (the whole wave)
    cc_word *bits = comp_bits(a, i) + (long long)y * a.WORDS;
    int32_t *lab = comp_lab(a, i) + (long long)y * W;
    int carry_in = 0, nsel = 0;
    bool top_in = false;
    for (int w0 = 0; w0 < a.WORDS; w0 += 64) {         // a turn: 64 words of the row, lane = word
        const int wi = w0 + lane;
        cc_word w = 0;
        if (wi < a.WORDS) { w = comp_select(a, e, y, wi); bits[wi] = w; }
        nsel += cc_popc(w);
        if (!top_in) carry_in = 64 * w0;
        const cc_word nonfull = __ballot(w != ~0ull);
        const int j = cc_carry_word(nonfull, lane);
        const int carry = cc_carry_col(j, __shfl(w, j < 0 ? 0 : j), 64 * w0, carry_in);
        const cc_word before = __shfl(w, lane ? lane - 1 : 0);
        const int prev_top = lane ? (int)(before >> 63) : (int)top_in;
        const int turns = a.WORDS - w0 < 64 ? a.WORDS - w0 : 64;
        for (int k = 0; k < turns; ++k) {              // the parents of word k: lane = cell
            const cc_word wk = __shfl(w, k);
            const int ck = __shfl(carry, k), pk = __shfl(prev_top, k), x = 64 * (w0 + k) + lane;
            if (x < W) lab[x] = ((wk >> lane) & 1ull) ? y * W + cc_first_col(wk, w0 + k, lane, pk != 0, ck) : -1;
        }
        const int j2 = cc_carry_word(nonfull, 64);     // what the next turn's word 0 sees
        carry_in = cc_carry_col(j2, __shfl(w, j2 < 0 ? 0 : j2), 64 * w0, carry_in);
        top_in = (__shfl(w, 63) >> 63) != 0;
    }
    nsel = wave_sum(nsel);
    if (lane == 0 && a.selected && nsel) atomicAdd(a.selected + i, nsel);
}

__global__ __launch_bounds__(kCompThreads) void k_comp_merge(const CompArgs *__restrict__ ap)
{
    const CompArgs &a = *ap;
    const int i = blockIdx.y, W = a.g.W, WORDS = a.WORDS;
    const long long idx = (long long)blockIdx.x * kCompThreads + threadIdx.x;
    if (idx >= (long long)a.g.H * WORDS) return;
    const int y = (int)(idx / WORDS), wi = (int)(idx - (long long)y * WORDS);
    if (y == 0) return;
    const cc_word *row = comp_bits(a, i) + (long long)y * WORDS, *above = row - WORDS;
    const cc_word cur = row[wi], up = above[wi];
    if (!cur) return;
    const bool cur_l = wi > 0 && (row[wi - 1] >> 63), up_l = wi > 0 && (above[wi - 1] >> 63), up_r = wi + 1 < WORDS && (above[wi + 1] & 1ull);
    const CcContacts c = cc_contacts(a.conn8, cur, up, cur_l, up_l, up_r);
    const CompPlane plane{comp_lab(a, i)};
    const int c0 = y * W + 64 * wi;
    for (int d = -1; d <= 1; ++d) {
        cc_word m = d < 0 ? c.up_left : (d == 0 ? c.up : c.up_right);
        while (m) {
            const int bit = cc_ctz(m);
            m &= m - 1;
            const int x = c0 + bit;
            // (both ends halved first: the walks of cc_unite start near the roots)
            cc_unite(plane, cc_find_halve(plane, x), cc_find_halve(plane, x - W + d));
        }
    }
}

__global__ __launch_bounds__(kCompThreads) void k_comp_heads(const CompArgs *__restrict__ ap)
{
    const CompArgs &a = *ap;
    const int i = blockIdx.y, W = a.g.W, WORDS = a.WORDS;
    const long long idx = (long long)blockIdx.x * kCompThreads + threadIdx.x;
    if (idx >= (long long)a.g.H * WORDS) return;
    const int y = (int)(idx / WORDS), wi = (int)(idx - (long long)y * WORDS);
    const cc_word *row = comp_bits(a, i) + (long long)y * WORDS;
    const cc_word w = row[wi];
    cc_word heads = w & ~((w << 1) | (cc_word)(wi > 0 && (row[wi - 1] >> 63)));
    const CompPlane plane{comp_lab(a, i)};
    while (heads) {
        const int x = y * W + 64 * wi + cc_ctz(heads);
        heads &= heads - 1;
        const int r = cc_find_halve(plane, x);
        if (r != x) plane.store(x, r);
    }
}

__global__ __launch_bounds__(kCompThreads) void k_comp_flatten(const CompArgs *__restrict__ ap)
{
    const CompArgs &a = *ap;
    const int i = blockIdx.y, lane = threadIdx.x & 63, y = blockIdx.x * (kCompThreads / 64) + (threadIdx.x >> 6), W = a.g.W;
    if (y >= a.g.H) return;
    int32_t *lab = comp_lab(a, i);
    const cc_word *bits = comp_bits(a, i) + (long long)y * a.WORDS;
    int roots = 0;
    for (int x0 = 0; x0 < W; x0 += 64) {
        if (!bits[x0 >> 6]) continue;                  // (the whole wave: nothing selected in these 64 cells)
        const int x = x0 + lane, c = y * W + x;
        bool root = false;
        if (x < W) {
            const int p = lab[c];
            if (p >= 0) {
                // a run head holds its root (k_comp_heads); any other cell holds a run head of its component - its own, or one further up
                // that path halving gave it: every parent in the plane is a run head
                const int r = p == c ? c : lab[p];
                root = r == c;
                if (r != p) lab[c] = r;
            }
        }
        roots += cc_popc(__ballot(root));
    }
    if (lane == 0) comp_rows(a, i)[y] = roots;
}

__global__ __launch_bounds__(kCompScanThreads) void k_comp_scan(const CompArgs *__restrict__ ap)
{
    __shared__ int part[kCompScanThreads];
    const CompArgs &a = *ap;
    const int i = blockIdx.x, t = threadIdx.x, H = a.g.H;
    int32_t *rows = comp_rows(a, i);
    const int lo = cc_seg_lo(H, t), hi = cc_seg_lo(H, t + 1);
    part[t] = cc_seg_sum(rows, lo, hi);
    __syncthreads();
    if (t == 0) {
        int s = 0;
        for (int j = 0; j < kCompScanThreads; ++j) { const int c = part[j]; part[j] = s; s += c; }
        rows[H] = s;
        if (a.count) a.count[i] = s;
    }
    __syncthreads();
    cc_seg_write(rows, lo, hi, part[t]);
}

__global__ __launch_bounds__(kCompThreads) void k_comp_assign(const CompArgs *__restrict__ ap)
{
    const CompArgs &a = *ap;
    const int i = blockIdx.y, lane = threadIdx.x & 63, y = blockIdx.x * (kCompThreads / 64) + (threadIdx.x >> 6), W = a.g.W;
    if (y >= a.g.H) return;
    const int32_t *lab = comp_lab(a, i);
    int32_t *aux = comp_aux(a, i);
    const cc_word *bits = comp_bits(a, i) + (long long)y * a.WORDS;
    int base = comp_rows(a, i)[y];
    for (int x0 = 0; x0 < W; x0 += 64) {
        if (!bits[x0 >> 6]) continue;                  // (the whole wave: no root among these 64 cells)
        const int x = x0 + lane, c = y * W + x;
        const bool root = x < W && lab[c] == c;
        const cc_word b = __ballot(root);
        if (root) {
            const int rank = base + cc_popc(b & cc_below(lane));
            aux[c] = rank;
            if (a.first && rank < a.cap) a.first[(long long)i * a.cap + rank] = c;
        }
        base += cc_popc(b);
    }
}

__global__ __launch_bounds__(kCompThreads) void k_comp_relabel(const CompArgs *__restrict__ ap)
{
    const CompArgs &a = *ap;
    const int i = blockIdx.y;
    const long long n = (long long)a.g.H * a.g.W, t = (long long)blockIdx.x * kCompThreads + threadIdx.x;
    int32_t *lab = comp_lab(a, i);
    const int32_t *aux = comp_aux(a, i);
    if (a.lab_vec) {
        if (t * 4 >= n) return;
        int4 p = *reinterpret_cast<const int4 *>(lab + t * 4);
        p.x = p.x < 0 ? 0 : aux[p.x] + 1; p.y = p.y < 0 ? 0 : aux[p.y] + 1; p.z = p.z < 0 ? 0 : aux[p.z] + 1; p.w = p.w < 0 ? 0 : aux[p.w] + 1;
        *reinterpret_cast<int4 *>(lab + t * 4) = p;
    } else {
        if (t >= n) return;
        const int p = lab[t];
        lab[t] = p < 0 ? 0 : aux[p] + 1;
    }
}

// seen[s]: the cells of word wi of row y (selected: w) with an unselected neighbour of status s, on the grid
__device__ __forceinline__ void comp_seen(const CompArgs &a, int i, int e, int y, int wi, cc_word w, cc_word (&seen)[6])
{
    const int W = a.g.W, WORDS = a.WORDS;
#pragma unroll
    for (int s = 0; s < 6; ++s) seen[s] = 0;
    for (int dr = -1; dr <= 1; ++dr) {
        const int r = y + dr;
        if (r < 0 || r >= a.g.H) continue;
        const cc_word *row = comp_bits(a, i) + (long long)r * WORDS;
        const cc_word sel = row[wi];
        uint4 s7[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int v = wi * 4 + q;
            s7[q] = (v < a.g.PV && v * 16 < W) ? status_vec7(a.pl, a.g, e, r, v) : make_uint4(0, 0, 0, 0);
        }
        const int xl = 64 * wi - 1, xr = 64 * wi + 64;
        int sl = -1, sr = -1;                          // the status of the unselected cell left / right of the word, -1: none
        if (wi > 0 && !(row[wi - 1] >> 63)) sl = *cell_status(a.pl, a.g, e, r, xl) & 7;
        if (xr < W && !(row[wi + 1] & 1ull)) sr = *cell_status(a.pl, a.g, e, r, xr) & 7;
#pragma unroll
        for (int s = 0; s < 6; ++s) {
            const uint32_t lo = s < 4 ? 1u << (8 * s) : 0u, hi = s < 4 ? 0u : 1u << (8 * (s - 4));
            cc_word m = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) m |= (cc_word)mask_bits16(lo, hi, s7[q], W - (wi * 4 + q) * 16) << (16 * q);
            seen[s] |= cc_touch_from(m & ~sel, sl == s, sr == s, dr == 0, a.conn8);
        }
    }
#pragma unroll
    for (int s = 0; s < 6; ++s) seen[s] &= w;
}

__global__ __launch_bounds__(kCompThreads) void k_comp_stats(const CompArgs *__restrict__ ap)
{
    const CompArgs &a = *ap;
    const int i = blockIdx.y, e = a.envs[i], W = a.g.W, WORDS = a.WORDS;
    const long long idx = (long long)blockIdx.x * kCompThreads + threadIdx.x;
    if (idx >= (long long)a.g.H * WORDS) return;
    const int y = (int)(idx / WORDS), wi = (int)(idx - (long long)y * WORDS);
    const cc_word w = comp_bits(a, i)[idx];
    if (!w) return;
    const int32_t *lab = comp_lab(a, i) + (long long)y * W;
    int32_t *sizes = comp_aux(a, i);
    cc_word seen[6], border = 0;
    if (a.touch) { comp_seen(a, i, e, y, wi, w, seen); border = cc_border(a.g.H, W, y, wi); }
    for (cc_word rest = w; rest;) {
        const cc_word run = cc_next_run(rest);
        rest &= ~run;
        const int x0 = 64 * wi + cc_ctz(run), len = cc_popc(run), x1 = x0 + len - 1, L = lab[x0];
        if (L <= 0) continue;                          // (cannot happen: the run is selected)
        if (a.largest) atomicAdd(sizes + (L - 1), len);
        if (L > a.cap) continue;
        const long long row = (long long)i * a.cap + (L - 1);
        if (a.cells) atomicAdd(a.cells + row, len);
        if (a.value) {
            const int32_t *vals = a.vals + a.val_env * e + (long long)y * a.g.P;
            long long sum = 0;
            for (int x = x0; x <= x1; ++x) sum += vals[x];
            if (sum) atomicAdd(reinterpret_cast<unsigned long long *>(a.value + row), (unsigned long long)sum);
        }
        if (a.bbox) {                                  // (x0, y0 start at -1 = the largest unsigned; x1, y1 at -1)
            // a look first: the four words only ever move one way, so a value seen that the run cannot improve - however stale - means
            // the atomic would change nothing; the runs of a large component then cost four loads, not four contended atomics
            int32_t *b = a.bbox + row * 4;
            if ((unsigned int)__hip_atomic_load(b + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > (unsigned int)x0) atomicMin(reinterpret_cast<unsigned int *>(b + 0), (unsigned int)x0);
            if ((unsigned int)__hip_atomic_load(b + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > (unsigned int)y) atomicMin(reinterpret_cast<unsigned int *>(b + 1), (unsigned int)y);
            if (__hip_atomic_load(b + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < x1) atomicMax(b + 2, x1);
            if (__hip_atomic_load(b + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < y) atomicMax(b + 3, y);
        }
        if (a.touch) {
            const int t = cc_touch_run(seen, border, run);
            if (t) atomicOr(a.touch + row, t);
        }
    }
}

// the sizes of all components start at 0: slots 0 .. C - 1 of the second plane, whose ranks k_comp_relabel has used up
__global__ __launch_bounds__(kCompThreads) void k_comp_zero(const CompArgs *__restrict__ ap)
{
    const CompArgs &a = *ap;
    const int i = blockIdx.y, C = comp_rows(a, i)[a.g.H];
    int32_t *sizes = comp_aux(a, i);
    for (long long j = (long long)blockIdx.x * kCompThreads + threadIdx.x; j < C; j += (long long)gridDim.x * kCompThreads) sizes[j] = 0;
}

__global__ __launch_bounds__(kCompThreads) void k_comp_largest(const CompArgs *__restrict__ ap)
{
    const CompArgs &a = *ap;
    const int i = blockIdx.y, C = comp_rows(a, i)[a.g.H];
    const int32_t *sizes = comp_aux(a, i);
    cc_word key = 0;
    for (long long j = (long long)blockIdx.x * kCompThreads + threadIdx.x; j < C; j += (long long)gridDim.x * kCompThreads) {
        const cc_word k = cc_largest_key((int)j + 1, sizes[j]);
        key = k > key ? k : key;
    }
    key = wave_max(key);
    if ((threadIdx.x & 63) == 0 && key) atomicMax(comp_key(a, i), key);
}

__global__ __launch_bounds__(kCompThreads) void k_comp_finish(const CompArgs *__restrict__ ap, int cn)
{
    const CompArgs &a = *ap;
    const long long t = (long long)blockIdx.x * kCompThreads + threadIdx.x;
    if (t >= (long long)cn * (a.k + 1)) return;
    const int i = (int)(t / (a.k + 1)), j = (int)(t - (long long)i * (a.k + 1));
    if (j == a.k) {
        if (a.largest) {
            const cc_word key = *comp_key(a, i);
            a.largest[2 * i] = cc_key_number(key);
            a.largest[2 * i + 1] = cc_key_cells(key);
        }
        return;
    }
    const long long at = (long long)i * a.k + j;
    const QueryPoint p = query_point(a.points, at, a.g.W, a.g.H);
    a.point_label[at] = p.ok ? comp_lab(a, i)[(long long)p.y * a.g.W + p.x] : -1;
}

}  // namespace
