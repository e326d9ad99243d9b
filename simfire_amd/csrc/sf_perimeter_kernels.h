// Perimeters of the fire (sf_perimeter): where the edge of a set S of cells runs - its length in cell edges, the
// cells of S that lie on it, and the edge itself as ordered polygons on the lattice of cell corners.  All integers.  Part of the
// single translation unit simfire_hip.hip.  S is read from whichever cell plane is current (a status mask), from a caller's plane
// (member) or from the arrival plane (at_update); nothing but the scratch and the caller's outputs is written.
// Two kernels.  k_perim_summary (no scratch): ONE streaming launch for the whole list - 64-cell words of S, popcounts of the words'
// differences, the front plane.  k_perim_trace: one workgroup per listed environment, resident until that environment is done; it
// ranks the directed crack edges in id order, builds the predecessor permutation and finds every loop by pointer doubling - no lane
// ever walks a loop, so a serpentine of 3.3 x 10^4 edges costs 16 rounds, not 3.3 x 10^4 steps.  Every output is decided by ranks
// and scans: no bit depends on scheduling.
//   vertex (vx, vy), 0 <= vx <= W, 0 <= vy <= H; cells around it: NW (vx - 1, vy - 1), NE (vx, vy - 1), SW (vx - 1, vy), SE (vx, vy)
//   edge d leaves the vertex towards 0: +x, 1: +y, 2: -x, 3: -y and exists iff its right cell is in S and its left cell is not:
//   d = 0: SE & ~NE, 1: SW & ~SE, 2: NW & ~SW, 3: NE & ~NW.  Its id is (vy * (W + 1) + vx) * 4 + d; the kernel orders by
//   (vy * VP + vx) * 4 + d with VP = 16 * ceil((W + 1) / 16), which is the same order: 16 vertices x 4 directions fill a 64-bit word.
#pragma once
#include "sf_bands.h"
#include "sf_query_dev.h"

namespace {

constexpr int kPerimThreads = 256;            // k_perim_summary
constexpr int kPerimTraceThreads = 1024;      // k_perim_trace: one workgroup fills a CU (16 waves hide the latency of the doubling's gathers)
constexpr int kPerimStrip = 8;                // rows per item of k_perim_summary (it reads 10 rows for 8)
constexpr int kPerimMaxWidth = 8192;
constexpr int kPerimArrays = 8;               // int32 arrays of max_edges in an environment's scratch
constexpr long long kPerimScratchDefault = 1ll << 30;      // bytes of scratch a call uses unless it names a budget

struct PerimArgs {
    CellGeo g;
    CellPlanes pl;             // the status bytes, in whichever plane is current
    const uint8_t *member;     // source 1: dense [H * W] u8, mem_env bytes between two environments' planes (0: one for all)
    long long mem_env;
    const uint32_t *arrival;   // source 2: the raw arrival plane [E][H][P], update + 1, 0 = never
    uint32_t at;               // source 2: the horizon (an update)
    int source;                // 0: status mask, 1: member, 2: arrival
    uint32_t tlo, thi;         // source 0: the mask as the table of one byte permute (mask_sel01)
    const int32_t *envs;       // the listed environments of this launch [n]
    int n;
    int conn8, simplify;
    int max_edges, max_vertices, max_loops;
    int BW, EW;                // 64-bit words per row of S = ceil(W / 64); edge words per vertex row = ceil((W + 1) / 16)
    int32_t *edges, *ncells;   // [n] (k_perim_summary: zeroed in front of the launch)
    uint8_t *front;            // [n][H][W] dense
    int front_vec;             // W % 16 == 0 and front aligned to 16 bytes: 16-byte stores
    int32_t *loops, *holes, *n_vertices;      // [n]
    int32_t *vertices;         // [n][max_vertices][2]
    int32_t *loop_start;       // [n][max_loops + 1]
    int32_t *loop_area, *loop_edges;          // [n][max_loops]
    uint8_t *scratch;          // k_perim_trace: scratch_env bytes per listed environment of the launch
    long long scratch_env;
    long long blocks_env;      // k_perim_summary: item blocks per listed environment = ceil(ceil(H / kPerimStrip) * BW / kPerimThreads)
    long long total;           // n * blocks_env
};

// Bytes of scratch k_perim_trace needs per listed environment: the bit plane of S (8 * H * BW), the edge words and their ranks
// (12 * (H + 1) * EW) and kPerimArrays int32 arrays of max_edges, rounded up to 256.
__host__ __device__ inline long long perim_env_bytes(int H, int W, int max_edges)
{
    const long long BW = (W + 63) / 64, EW = (W + 16) / 16;
    return (8ll * H * BW + 12ll * (H + 1) * EW + 4ll * kPerimArrays * max_edges + 255) / 256 * 256;
}

// bit j: cell (16 v + j, y) is on the grid and in S; 0 <= y < H, v >= 0
__device__ __forceinline__ uint32_t perim_vec16(const PerimArgs &a, int e, int y, int v)
{
    const CellGeo &g = a.g;
    const int in = g.W - v * 16;                 // cells of the vector on the grid (the rest is pitch padding: never in S)
    if (in <= 0) return 0u;
    uint32_t m = 0u;
    if (a.source == 0) {             // (not mask_bits16: the last line is the grid mask of all three sources, and with both the kernels need more registers)
        m = pack16(mask_sel01(a.tlo, a.thi, status_vec7(a.pl, g, e, y, v)));
    } else if (a.source == 1) {      // (decided by the address, vector by vector - not dense_vec16, whose flag holds for a whole plane)
        const uint8_t *p = a.member + (long long)e * a.mem_env + (long long)y * g.W + v * 16;
        if (in >= 16 && !((uintptr_t)p & 15)) {
            m = pack16(nz01x16(*reinterpret_cast<const uint4 *>(p)));
        } else {
            const int k = in < 16 ? in : 16;
            for (int j = 0; j < k; ++j) m |= p[j] ? 1u << j : 0u;
        }
    } else {
        const uint4 *p = reinterpret_cast<const uint4 *>(a.arrival + (long long)e * g.plane_env + (long long)y * g.P + v * 16);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint4 q = p[k];                // (0 = never: 0 - 1 wraps past every horizon)
            m |= ((q.x - 1u <= a.at ? 1u : 0u) | (q.y - 1u <= a.at ? 2u : 0u) | (q.z - 1u <= a.at ? 4u : 0u) | (q.w - 1u <= a.at ? 8u : 0u)) << (4 * k);
        }
    }
    return in >= 16 ? m : m & ((1u << in) - 1u);
}

// the cells 64 w .. 64 w + 63 of row y as a word; rows off the grid are empty
__device__ __forceinline__ unsigned long long perim_word(const PerimArgs &a, int e, int y, int w)
{
    if ((unsigned)y >= (unsigned)a.g.H) return 0ull;
    return (unsigned long long)perim_vec16(a, e, y, 4 * w) | ((unsigned long long)perim_vec16(a, e, y, 4 * w + 1) << 16) |
           ((unsigned long long)perim_vec16(a, e, y, 4 * w + 2) << 32) | ((unsigned long long)perim_vec16(a, e, y, 4 * w + 3) << 48);
}

// The summary form.  A grid-stride loop over (listed environment, block of kPerimThreads items); an item is (strip of kPerimStrip
// rows, 64-cell word).  Per row: cells = popc(w); the cracks above the row = popc(w ^ row above) - row -1 is empty, and the last row
// adds popc(w) for the border below -; the cracks left of each cell = popc(w ^ (w << 1 | carry)), where bit W, which is empty, closes
// the row - or, where W is a multiple of 64, the last word's top bit does.  front = w & ~(above & below & left & right).
__global__ __launch_bounds__(kPerimThreads) void k_perim_summary(PerimArgs a)
{
    __shared__ uint32_t s_red[2];
    const CellGeo &g = a.g;
    const int t = threadIdx.x;
    const int items = (g.H + kPerimStrip - 1) / kPerimStrip * a.BW;
    if (t < 2) s_red[t] = 0u;
    __syncthreads();
    for (long long wi = blockIdx.x; wi < a.total; wi += gridDim.x) {
        const int i = (int)(wi / a.blocks_env);
        const int item = (int)(wi - (long long)i * a.blocks_env) * kPerimThreads + t;
        const int e = a.envs[i];
        uint32_t ne = 0u, nc = 0u;
        if (item < items) {
            const int s = item / a.BW, w = item - s * a.BW;
            const int y0 = s * kPerimStrip, y1 = min(y0 + kPerimStrip, g.H);
            const bool last = w == a.BW - 1;
            unsigned long long up = perim_word(a, e, y0 - 1, w), cur = perim_word(a, e, y0, w);
            for (int y = y0; y < y1; ++y) {
                const unsigned long long dn = perim_word(a, e, y + 1, w);
                const unsigned long long cl = w ? (perim_vec16(a, e, y, 4 * w - 1) >> 15) & 1u : 0u;
                const unsigned long long l = (cur << 1) | cl;
                nc += (uint32_t)__popcll(cur);
                ne += (uint32_t)__popcll(cur ^ up) + (uint32_t)__popcll(cur ^ l);
                if (y == g.H - 1) ne += (uint32_t)__popcll(cur);
                if (last && (g.W & 63) == 0) ne += (uint32_t)(cur >> 63);
                if (a.front) {
                    const unsigned long long cr = last ? 0ull : perim_vec16(a, e, y, 4 * w + 4) & 1u;
                    const unsigned long long f = cur & ~(up & dn & l & ((cur >> 1) | (cr << 63)));
                    uint8_t *o = a.front + ((long long)i * g.H + y) * g.W + 64 * w;
                    if (a.front_vec) {
#pragma unroll
                        for (int v = 0; v < 4; ++v) {
                            if (64 * w + 16 * v >= g.W) break;
                            uint32_t d[4];
                            bits_bytes16((uint32_t)(f >> (16 * v)) & 0xFFFFu, d);
                            *reinterpret_cast<uint4 *>(o + 16 * v) = make_uint4(d[0], d[1], d[2], d[3]);
                        }
                    } else {
                        const int k = min(64, g.W - 64 * w);
                        for (int j = 0; j < k; ++j) o[j] = (uint8_t)((f >> j) & 1u);
                    }
                }
                up = cur; cur = dn;
            }
        }
        // integer sums: a wave, the workgroup's two LDS slots, one atomic each per item block
        if (a.edges || a.ncells) {
            ne = wave_sum(ne); nc = wave_sum(nc);
            if ((t & 63) == 0) { if (ne) atomicAdd(&s_red[0], ne); if (nc) atomicAdd(&s_red[1], nc); }
            __syncthreads();
            if (t < 2) {
                const uint32_t v = s_red[t];
                if (v) {
                    if (t == 0) { if (a.edges) atomicAdd(a.edges + i, (int)v); }
                    else if (a.ncells) atomicAdd(a.ncells + i, (int)v);
                    s_red[t] = 0u;
                }
            }
            __syncthreads();
        }
    }
}

// In-place scan of p[0 .. n) by the whole workgroup, a tile of one element per thread at a time (coalesced); returns the total.
// Every thread calls it with the same n; it ends behind a barrier.  s_w: one int per wave.
template <bool INCL>
__device__ int perim_scan(int32_t *p, int n, int32_t *s_w)
{
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, nw = (int)blockDim.x >> 6;
    int carry = 0;
    for (int base = 0; base < n; base += (int)blockDim.x) {
        const int idx = base + t;
        const int v = idx < n ? p[idx] : 0;
        int x = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(x, o); if (lane >= o) x += u; }
        if (lane == 63) s_w[wv] = x;
        __syncthreads();
        int before = 0, tot = 0;
        for (int k = 0; k < nw; ++k) { const int s = s_w[k]; tot += s; before += k < wv ? s : 0; }
        if (idx < n) p[idx] = carry + before + (INCL ? x : x - v);
        carry += tot;
        __syncthreads();
    }
    return carry;
}

// 16 bits -> every fourth bit of a word
__device__ __forceinline__ unsigned long long perim_spread(uint32_t m)
{
    unsigned long long x = m & 0xFFFFu;
    x = (x | (x << 24)) & 0x000000FF000000FFull;
    x = (x | (x << 12)) & 0x000F000F000F000Full;
    x = (x | (x << 6)) & 0x0303030303030303ull;
    x = (x | (x << 3)) & 0x1111111111111111ull;
    return x;
}

struct PerimPlane {
    const unsigned long long *B;     // [H][BW]
    int H, W, BW;
    __device__ __forceinline__ bool in(int x, int y) const
    {
        return (unsigned)x < (unsigned)W && (unsigned)y < (unsigned)H && ((B[y * BW + (x >> 6)] >> (x & 63)) & 1ull);
    }
    // 17 bits: bit k = cell (16 j - 1 + k, y)
    __device__ __forceinline__ uint32_t window(int y, int j) const
    {
        if ((unsigned)y >= (unsigned)H) return 0u;
        const int wi = j >> 2, sh = (j & 3) * 16;
        const unsigned long long wd = wi < BW ? B[y * BW + wi] : 0ull;
        const uint32_t prev = j == 0 ? 0u : (sh ? (uint32_t)(wd >> (sh - 1)) & 1u : (uint32_t)(B[y * BW + wi - 1] >> 63));
        return (((uint32_t)(wd >> sh) & 0xFFFFu) << 1) | prev;
    }
};

// The trace form: one workgroup per listed environment.  Its scratch: B, the bit plane of S | EWD, the edge words [H + 1][EW] | PF,
// the edges in front of each word (the exclusive scan of the words' popcounts: an edge's rank in id order is PF[word] + the set bits
// below it) | kPerimArrays int32 arrays of max_edges.  Steps, a barrier between any two:
//   1  B and |S|;  2  EWD, PF and the number of edges - more than max_edges ends the environment with -1 in the three counts;
//   3  id[r] and prv[succ(r)] = r: the successor's direction from the two cells ahead of the head, its rank from EWD and PF;
//   4  the least rank of every cycle by pointer doubling along prv, (ptr, mn) <- (ptr[ptr], min(mn, mn[ptr])), double-buffered: an
//      edge's leader, the loop's smallest id;  5  a second doubling that stops at the leader: hops back to it = position in the loop;
//   6  scans of the leader flags (loop numbers, already in canonical order) and of the loops' lengths (where a loop begins in
//      (loop, position) order);  7  x * dy of every edge scattered into that order and scanned: a loop's signed area is a difference
//      of two prefix sums;  8  the corner flags likewise: vertex numbers;  9  the counts, and the lists where they fit.
__global__ __launch_bounds__(kPerimTraceThreads) void k_perim_trace(PerimArgs a)
{
    __shared__ int32_t s_w[kPerimTraceThreads / 64];
    __shared__ int s_cnt[2];
    const CellGeo &g = a.g;
    const int t = threadIdx.x, T = (int)blockDim.x;
    const int i = blockIdx.x, e = a.envs[i];
    const int H = g.H, W = g.W, BW = a.BW, EW = a.EW, VP = EW * 16, ME = a.max_edges;
    const int NB = H * BW, NW = (H + 1) * EW;
    uint8_t *sc = a.scratch + (long long)i * a.scratch_env;
    unsigned long long *B = reinterpret_cast<unsigned long long *>(sc);
    unsigned long long *EWD = B + NB;
    int32_t *PF = reinterpret_cast<int32_t *>(EWD + NW);
    int32_t *A0 = PF + NW;
    const auto arr = [&](int k) { return A0 + (long long)k * ME; };
    const PerimPlane S{B, H, W, BW};

    if (t < 2) s_cnt[t] = 0;
    __syncthreads();
    // 1
    {
        uint32_t nc = 0u;
        for (int idx = t; idx < NB; idx += T) {
            const int y = idx / BW;
            const unsigned long long v = perim_word(a, e, y, idx - y * BW);
            B[idx] = v;
            nc += (uint32_t)__popcll(v);
        }
        nc = wave_sum(nc);
        if ((t & 63) == 0 && nc) atomicAdd(&s_cnt[0], (int)nc);
    }
    __syncthreads();
    // 2
    for (int idx = t; idx < NW; idx += T) {
        const int vy = idx / EW, j = idx - vy * EW;
        const uint32_t up = S.window(vy - 1, j), dn = S.window(vy, j);
        const uint32_t nw = up & 0xFFFFu, ne = (up >> 1) & 0xFFFFu, sw = dn & 0xFFFFu, se = (dn >> 1) & 0xFFFFu;
        const unsigned long long wd = perim_spread(se & ~ne) | (perim_spread(sw & ~se) << 1) | (perim_spread(nw & ~sw) << 2) | (perim_spread(ne & ~nw) << 3);
        EWD[idx] = wd;
        PF[idx] = __popcll(wd);
    }
    __syncthreads();
    const int n_e = perim_scan<false>(PF, NW, s_w);
    if (t == 0) {
        if (a.edges) a.edges[i] = n_e;
        if (a.ncells) a.ncells[i] = s_cnt[0];
    }
    if (n_e > ME) {                              // (uniform: every thread has the same total)
        if (t == 0) {
            if (a.loops) a.loops[i] = -1;
            if (a.holes) a.holes[i] = -1;
            if (a.n_vertices) a.n_vertices[i] = -1;
        }
        return;
    }
    int32_t *id = arr(0), *prv = arr(1);
    // 3  (prv starts as the identity: whatever happens, every entry is a rank)
    for (int r = t; r < n_e; r += T) prv[r] = r;
    __syncthreads();
    for (int idx = t; idx < NW; idx += T) {
        unsigned long long wd = EWD[idx];
        int r = PF[idx];
        const int vy = idx / EW, j = idx - vy * EW;
        while (wd) {
            const int b = __ffsll((long long)wd) - 1;
            wd &= wd - 1ull;
            const int d = b & 3, vx = j * 16 + (b >> 2);
            const int hx = vx + (d == 0) - (d == 2), hy = vy + (d == 1) - (d == 3);
            // the cells ahead of the head: on the right and on the left of an edge that leaves it in direction d
            const int rx = hx - (d == 1 || d == 2), ry = hy - (d == 2 || d == 3);
            const int lx = hx - (d == 2 || d == 3), ly = hy - (d == 0 || d == 3);
            const bool ar = S.in(rx, ry), al = S.in(lx, ly);
            const int turn = a.conn8 ? (al ? 3 : (ar ? 0 : 1)) : (!ar ? 1 : (!al ? 0 : 3));
            const int spid = ((hy * VP + hx) << 2) | ((d + turn) & 3);
            const int sw = spid >> 6;
            int sr = PF[sw] + __popcll(EWD[sw] & ((1ull << (spid & 63)) - 1ull));
            sr = min(sr, n_e - 1);
            id[r] = (idx << 6) | b;
            prv[sr] = r;
            ++r;
        }
    }
    __syncthreads();
    // 4
    int32_t *pc = arr(2), *pn = arr(3), *mc = arr(4), *mn = arr(5);
    for (int r = t; r < n_e; r += T) {
        const int p = prv[r];
        pc[r] = prv[p];
        mc[r] = min(r, p);
    }
    __syncthreads();
    for (int span = 2; span < n_e; span <<= 1) {
        for (int r = t; r < n_e; r += T) {
            const int p = pc[r];
            pn[r] = pc[p];
            mn[r] = min(mc[r], mc[p]);
        }
        __syncthreads();
        int32_t *x = pc; pc = pn; pn = x;
        x = mc; mc = mn; mn = x;
    }
    const int32_t *leader = mc;
    // 5  (free: pc, pn, mn and array 6)
    int32_t *jc = pc, *jn = pn, *dc = mn, *dn = arr(6);
    for (int r = t; r < n_e; r += T) {
        const bool lead = leader[r] == r;
        jc[r] = lead ? r : prv[r];
        dc[r] = lead ? 0 : 1;
    }
    __syncthreads();
    for (int span = 1; span < n_e; span <<= 1) {
        for (int r = t; r < n_e; r += T) {
            const int j = jc[r];
            dn[r] = dc[r] + dc[j];
            jn[r] = jc[j];
        }
        __syncthreads();
        int32_t *x = jc; jc = jn; jn = x;
        x = dc; dc = dn; dn = x;
    }
    const int32_t *pos = dc;
    // 6  (free: jc, jn, dn and array 7)
    int32_t *lno = jc, *off = jn, *tq = dn, *cq = arr(7);
    for (int r = t; r < n_e; r += T) {
        const bool lead = leader[r] == r;
        lno[r] = lead ? 1 : 0;
        off[r] = lead ? pos[prv[r]] + 1 : 0;
    }
    __syncthreads();
    const int n_l = perim_scan<false>(lno, n_e, s_w);
    perim_scan<false>(off, n_e, s_w);
    // 7, 8
    for (int r = t; r < n_e; r += T) {
        const int q = min(off[leader[r]] + pos[r], n_e - 1);
        const int d = id[r] & 3, vx = (id[r] >> 2) % VP;
        tq[q] = d == 1 ? vx : (d == 3 ? -vx : 0);
        cq[q] = a.simplify ? ((id[prv[r]] & 3) != d ? 1 : 0) : 1;
    }
    __syncthreads();
    perim_scan<true>(tq, n_e, s_w);
    const int n_v = perim_scan<false>(cq, n_e, s_w);
    // 9
    const bool fits = n_v <= a.max_vertices && n_l <= a.max_loops;
    int nh = 0;
    for (int r = t; r < n_e; r += T) {
        const int ld = leader[r];
        const int o = off[ld];
        if (fits && a.vertices) {
            const int d = id[r] & 3;
            if (!a.simplify || (id[prv[r]] & 3) != d) {
                const int v = id[r] >> 2;
                int32_t *vp = a.vertices + ((long long)i * a.max_vertices + cq[min(o + pos[r], n_e - 1)]) * 2;
                vp[0] = v % VP;
                vp[1] = v / VP;
            }
        }
        if (ld != r) continue;
        const int len = pos[prv[r]] + 1;
        const int area = tq[min(o + len - 1, n_e - 1)] - (o ? tq[o - 1] : 0);
        nh += area < 0 ? 1 : 0;
        if (fits) {
            const int l = lno[r];
            if (a.loop_start) a.loop_start[(long long)i * (a.max_loops + 1) + l] = cq[o];
            if (a.loop_area) a.loop_area[(long long)i * a.max_loops + l] = area;
            if (a.loop_edges) a.loop_edges[(long long)i * a.max_loops + l] = len;
        }
    }
    nh = (int)wave_sum((uint32_t)nh);
    if ((t & 63) == 0 && nh) atomicAdd(&s_cnt[1], nh);
    __syncthreads();
    if (t == 0) {
        if (a.loops) a.loops[i] = n_l;
        if (a.holes) a.holes[i] = s_cnt[1];
        if (a.n_vertices) a.n_vertices[i] = n_v;
        if (fits && a.loop_start) a.loop_start[(long long)i * (a.max_loops + 1) + n_l] = n_v;
    }
}

}  // namespace
