// Fire influence (sf_influence): how much of the fire passes through a cell.  Every cell has at most one parent,
// a code 0..7 into SRC_OFFSETS (c_dx / c_dy: the R table's plane order, the convention of the travel forecast's pred plane); the codes
// come from a caller's plane or from the ignition tree of the episode (the spread-graph parent masks narrowed to ONE parent by the
// arrival plane: the newest neighbour that burned strictly earlier, ties to the lowest code - acyclic by construction).  For a cell c,
// D(c) is the set of cells whose parent chain reaches c; the outputs are sum of w over D(c) for two weights, w1 (1, or an include
// plane) and wv (an int32 weight where w1 is set), all in integers: integer addition commutes, so no bit depends on scheduling.
// Four kernels per chunk of listed environments, a thread per cell (k_infl_points: per point), stream-ordered:
//   k_infl_stage   the codes derived (history) or read (plane), sanitised - anything but 0..7 with the neighbour on the grid is "no
//                  parent" -, kept as int8 in scratch and in the pred output; accumulators zeroed; every forest cell adds 1 to its
//                  parent's counter (zeroed by the host in front of the launch).
//   k_infl_walk    the bottom-up refit: a forest cell whose counter is still exactly 0 has no child and starts a walker.  A walker
//                  adds its cell's finished sums + own weights to the parent's accumulators, then adds 15 to the parent's counter:
//                  the low four bits count the children still out (at most 8), the bits above the children that have arrived, so a
//                  counter that walkers have touched is never 0 again and no late thread mistakes a finished cell for a leaf.  The
//                  walker whose add found the low bits at 1 was the last child: it alone carries on from the parent; every other
//                  walker ends.  No waiting, no spinning, no barrier between workgroups: the pass cannot hang on any input.  On a
//                  cycle every cell keeps one child that never arrives, so no walker enters it and its low bits stay positive.
//                  Words shared between walkers (counters, accumulators) are touched by agent-scope atomics only: the counter RMW is
//                  acq_rel - it releases the sums added in front of it and acquires those of the siblings -, the finished sums are
//                  read with atomic loads (a plain load may be served from the CU's L1, and the XCDs' L2s are not coherent).
//   k_infl_finish  low bits still positive: the cell lies on a cycle (cells SF_INFLUENCE_CYCLE, value 0); else the inclusive term;
//                  forest / roots / cyclic counted per wave, one atomic add each (a parentless cell with a counter != 0 is a root).
//   k_infl_points  the plane values at each point's cell and the route up the parent chain, bounded by max_route.
// Part of the single translation unit simfire_hip.hip.  Nothing but the scratch and the outputs is written.
#pragma once
#include "sf_query_dev.h"

namespace {

constexpr int kInflThreads = 256;
constexpr int kInflMaxWidth = 8192;                   // wider grids are refused (as the other queries do)
constexpr int kInflMaxRoute = 1 << 20;
constexpr long long kInflScratchDefault = 1ll << 30;
constexpr int kInflArrive = 15;                       // a walker's add to its parent's counter: one child fewer out (- 1), one more in (+ 16)

struct InflArgs {
    int H, W, P;                 // the grid; P: row pitch of the handle's planes (parents, arrival, value plane)
    long long plane_env;         // elements between two environments' planes of the handle
    const int32_t *envs;         // the listed environments of this chunk
    int source;                  // SF_INFLUENCE_PRED_PLANE / SF_INFLUENCE_PRED_HISTORY
    const int8_t *pred_in;       // this chunk's part of the caller's plane (pred_env = H * W per LISTED environment, or 0: one for all)
    long long pred_env;
    const uint8_t *parents;      // [E][H][P] spread-graph parent masks (history)
    const uint32_t *arrival;     // [E][H][P] update + 1, 0 = never (history)
    const uint8_t *include;      // dense u8 [H * W] (inc_env = 0) or [E][H * W] by environment number, or null
    long long inc_env;
    const int32_t *weights;      // the handle's value plane (pitch P) or the caller's (pitch W), or null: no wv
    long long w_env;             // elements between two environments' weights, by environment number (0: one for all)
    int w_pitch;
    int inclusive;
    uint8_t *scratch;            // this chunk's scratch, scratch_env bytes per listed environment: codes | counters | accumulators not asked for
    long long scratch_env, o_cnt, o_acc_c, o_acc_v;      // byte offsets inside an environment's scratch (o_acc_*: -1 = the output is the accumulator)
    int32_t *cells;              // this chunk's part of the outputs (null: not asked for)
    long long *value;
    int8_t *pred_out;
    int32_t *forest, *roots, *cyclic;
    const int32_t *points;       // this chunk's [cn][k][3] = (column, row, id), or null
    int k, max_route;
    int32_t *point_cells, *point_route, *point_hops;
    long long *point_value;
};

// bytes of scratch per listed environment: the codes, the counters, and the accumulator of cells / value where that is no output
__host__ __device__ inline long long infl_round(long long b) { return (b + 255) / 256 * 256; }
__host__ __device__ inline long long infl_env_bytes(int H, int W, bool cells_out, bool weighted, bool value_out)
{
    const long long n = (long long)H * W;
    return infl_round(n) + infl_round(4 * n) + (cells_out ? 0 : infl_round(4 * n)) + (weighted && !value_out ? infl_round(8 * n) : 0);
}

__device__ __forceinline__ int8_t *infl_codes(const InflArgs &a, int i) { return reinterpret_cast<int8_t *>(a.scratch + (long long)i * a.scratch_env); }
__device__ __forceinline__ int32_t *infl_counters(const InflArgs &a, int i)
{
    return reinterpret_cast<int32_t *>(a.scratch + (long long)i * a.scratch_env + a.o_cnt);
}
__device__ __forceinline__ int32_t *infl_acc_c(const InflArgs &a, int i)
{
    return a.o_acc_c < 0 ? a.cells + (long long)i * a.H * a.W : reinterpret_cast<int32_t *>(a.scratch + (long long)i * a.scratch_env + a.o_acc_c);
}
__device__ __forceinline__ long long *infl_acc_v(const InflArgs &a, int i)      // null: no weights
{
    if (!a.weights) return nullptr;
    return a.o_acc_v < 0 ? a.value + (long long)i * a.H * a.W : reinterpret_cast<long long *>(a.scratch + (long long)i * a.scratch_env + a.o_acc_v);
}
__device__ __forceinline__ int infl_w1(const InflArgs &a, int e, long long c) { return !a.include || a.include[a.inc_env * e + c] != 0; }
__device__ __forceinline__ long long infl_wv(const InflArgs &a, int e, int y, int x)
{
    return (long long)a.weights[a.w_env * e + (long long)y * a.w_pitch + x];
}

// The code of cell (y, x) of environment e from the episode's history: the candidate parents are the neighbours the parent mask names
// (bit j = neighbour j of graph.py's adj_locs order) that are on the grid and burned strictly earlier; the newest wins, ties to the
// lowest code.  -1: never burned, or no candidate (a root).
__device__ __forceinline__ int infl_history_code(const InflArgs &a, int e, int y, int x)
{
    constexpr int kBitOfCode[8] = {1, 2, 3, 0, 4, 7, 6, 5};        // SRC_OFFSETS index -> bit of the parent mask
    const long long base = (long long)e * a.plane_env;
    const uint32_t a1 = a.arrival[base + (long long)y * a.P + x];
    if (a1 == 0u) return -1;
    const uint32_t mask = a.parents[base + (long long)y * a.P + x];
    int best = -1;
    uint32_t best_a = 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (!((mask >> kBitOfCode[k]) & 1u)) continue;
        const int nx = x + c_dx[k], ny = y + c_dy[k];
        if (nx < 0 || nx >= a.W || ny < 0 || ny >= a.H) continue;
        const uint32_t an = a.arrival[base + (long long)ny * a.P + nx];
        if (an != 0u && an < a1 && an > best_a) { best_a = an; best = k; }
    }
    return best;
}

__global__ __launch_bounds__(kInflThreads) void k_infl_stage(InflArgs a)
{
    const int i = blockIdx.y, e = a.envs[i];
    const long long n = (long long)a.H * a.W, c = (long long)blockIdx.x * kInflThreads + threadIdx.x;
    if (c >= n) return;
    const int y = (int)(c / a.W), x = (int)(c - (long long)y * a.W);
    int code;
    if (a.source == SF_INFLUENCE_PRED_HISTORY) {
        code = infl_history_code(a, e, y, x);
    } else {
        code = a.pred_in[a.pred_env * i + c];
        if (code < 0 || code > 7) code = -1;
        else {
            const int nx = x + c_dx[code], ny = y + c_dy[code];
            if (nx < 0 || nx >= a.W || ny < 0 || ny >= a.H) code = -1;
        }
    }
    infl_codes(a, i)[c] = (int8_t)code;
    if (a.pred_out) a.pred_out[(long long)i * n + c] = (int8_t)code;
    infl_acc_c(a, i)[c] = 0;
    long long *av = infl_acc_v(a, i);
    if (av) av[c] = 0;
    if (code >= 0) {
        const long long p = c + (long long)c_dy[code] * a.W + c_dx[code];
        __hip_atomic_fetch_add(infl_counters(a, i) + p, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(kInflThreads) void k_infl_walk(InflArgs a)
{
    const int i = blockIdx.y, e = a.envs[i];
    const long long n = (long long)a.H * a.W;
    long long c = (long long)blockIdx.x * kInflThreads + threadIdx.x;
    if (c >= n) return;
    const int8_t *codes = infl_codes(a, i);
    int32_t *cnt = infl_counters(a, i);
    int32_t *ac = infl_acc_c(a, i);
    long long *av = infl_acc_v(a, i);
    int code = codes[c];
    if (code < 0) return;
    if (__hip_atomic_load(cnt + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return;      // has children, or had: not a leaf
    int32_t sum_c = 0;
    long long sum_v = 0;
    for (;;) {
        const int w1 = infl_w1(a, e, c);
        const long long p = c + (long long)c_dy[code] * a.W + c_dx[code];
        const int32_t add_c = sum_c + w1;
        if (add_c) __hip_atomic_fetch_add(ac + p, add_c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (av) {
            const int y = (int)(c / a.W), x = (int)(c - (long long)y * a.W);
            const long long add_v = sum_v + (w1 ? infl_wv(a, e, y, x) : 0ll);
            if (add_v) __hip_atomic_fetch_add(av + p, add_v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        const int32_t old = __hip_atomic_fetch_add(cnt + p, kInflArrive, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if ((old & 15) != 1) return;                  // a sibling is still out (or p lies on a cycle): whoever arrives last carries on
        c = p;
        code = codes[c];
        if (code < 0) return;                         // a root: its sums are complete
        sum_c = __hip_atomic_load(ac + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (av) sum_v = __hip_atomic_load(av + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(kInflThreads) void k_infl_finish(InflArgs a)
{
    const int i = blockIdx.y, e = a.envs[i];
    const long long n = (long long)a.H * a.W, c = (long long)blockIdx.x * kInflThreads + threadIdx.x;
    const bool in = c < n;
    bool forest = false, root = false, cyc = false;
    if (in) {
        const int code = infl_codes(a, i)[c];
        const int32_t cnt = infl_counters(a, i)[c];
        forest = code >= 0;
        cyc = (cnt & 15) != 0;
        root = code < 0 && cnt != 0;
        int32_t *ac = infl_acc_c(a, i);
        long long *av = infl_acc_v(a, i);
        const int w1 = a.inclusive ? infl_w1(a, e, c) : 0;
        if (cyc) ac[c] = SF_INFLUENCE_CYCLE;
        else if (w1) ac[c] += 1;
        if (av) {
            if (cyc) av[c] = 0;
            else if (w1) {
                const int y = (int)(c / a.W), x = (int)(c - (long long)y * a.W);
                av[c] += infl_wv(a, e, y, x);
            }
        }
    }
    const int nf = __popcll(__ballot(forest)), nr = __popcll(__ballot(root)), nc = __popcll(__ballot(cyc));
    if ((threadIdx.x & 63) == 0) {
        if (a.forest && nf) atomicAdd(a.forest + i, nf);
        if (a.roots && nr) atomicAdd(a.roots + i, nr);
        if (a.cyclic && nc) atomicAdd(a.cyclic + i, nc);
    }
}

__global__ __launch_bounds__(kInflThreads) void k_infl_points(InflArgs a, int cn)
{
    const long long t = (long long)blockIdx.x * kInflThreads + threadIdx.x;
    if (t >= (long long)cn * a.k) return;
    const int i = (int)(t / a.k);
    const QueryPoint p = query_point(a.points, t, a.W, a.H);
    const bool ok = p.ok;
    long long c = (long long)p.y * a.W + p.x;
    if (a.point_cells) a.point_cells[t] = ok ? infl_acc_c(a, i)[c] : -1;
    if (a.point_value) a.point_value[t] = ok ? infl_acc_v(a, i)[c] : 0ll;
    if (a.max_route > 0) {
        int32_t *route = a.point_route + t * a.max_route;
        int r = 0, hops = -1;
        if (ok) {
            const int8_t *codes = infl_codes(a, i);
            for (;;) {
                route[r++] = (int32_t)c;
                const int code = codes[c];
                if (code < 0) { hops = r - 1; break; }
                if (r == a.max_route) { hops = -2; break; }
                c += (long long)c_dy[code] * a.W + c_dx[code];
            }
        }
        for (; r < a.max_route; ++r) route[r] = -1;
        a.point_hops[t] = hops;
    }
}

}  // namespace
