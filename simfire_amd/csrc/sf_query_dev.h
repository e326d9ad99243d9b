// What the spatial queries (sf_distance ... sf_influence) share on the device: status masks as byte-permute tables, the caller's
// points, wave reductions, the caller's dense u8 planes, 16 cells as 16 bits, and what the two band searches read.  With sf_cells.h
// (where the status bytes are) the starting point of a new query's kernels, as sf_host_query.h is of its host side.  Part of the
// single translation unit simfire_hip.hip.
#pragma once
#include "sf_common.h"

namespace {

// ---- status masks.  A mask over BurnStatus 0..7 travels as the table of one byte permute: byte s of (hi : lo) = 1 if the mask
// selects status s (mask_tables, sf_host_query.h).  q: four dwords of status bytes, already & 7.
__device__ __forceinline__ uint4 and44(uint4 a, uint4 b) { return make_uint4(a.x & b.x, a.y & b.y, a.z & b.z, a.w & b.w); }
// 0/1 per byte: the status is selected
__device__ __forceinline__ uint4 mask_sel01(uint32_t lo, uint32_t hi, uint4 q)
{
    return make_uint4(__builtin_amdgcn_perm(hi, lo, q.x), __builtin_amdgcn_perm(hi, lo, q.y), __builtin_amdgcn_perm(hi, lo, q.z), __builtin_amdgcn_perm(hi, lo, q.w));
}
// 0/1 per byte for the first `in` (<= 0: none, >= 16: all) of 16 cells: the cells of a vector that lie on the grid
__device__ __forceinline__ uint4 first01x16(int in) { return make_uint4(first01(in), first01(in - 4), first01(in - 8), first01(in - 12)); }
// sixteen 0/1 bytes -> 16 bits, cell j at bit j
__device__ __forceinline__ uint32_t pack16(uint4 b01) { return pack4(b01.x) | (pack4(b01.y) << 4) | (pack4(b01.z) << 8) | (pack4(b01.w) << 12); }

// ---- points.  Entry `index` of a [..][3] = (column, row, id) list: an id <= 0 or a position off the grid is not a point (ok = false;
// what is written for it is the query's own)
struct QueryPoint {
    int x, y;
    bool ok;
};
__device__ __forceinline__ QueryPoint query_point(const int32_t *points, long long index, int W, int H)
{
    const int32_t *p = points + index * 3;
    QueryPoint q;
    q.x = p[0]; q.y = p[1];
    q.ok = p[2] > 0 && q.x >= 0 && q.x < W && q.y >= 0 && q.y < H;
    return q;
}

// ---- reductions over the 64 lanes of a wave: every lane gets the result
template <class T> __device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
template <class T> __device__ __forceinline__ T wave_max(T v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const T u = __shfl_xor(v, o); v = u > v ? u : v; }
    return v;
}
template <class T> __device__ __forceinline__ T wave_min(T v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const T u = __shfl_xor(v, o); v = v < u ? v : u; }
    return v;
}

// ---- the caller's dense planes.  The 16 bytes of vector v in row y of a dense u8 plane of pitch W; vec: W % 16 == 0 and the plane
// is aligned to 16 bytes - one load; else byte by byte, the bytes past the row's end 0
__device__ __forceinline__ uint4 dense_vec16(const uint8_t *plane, int vec, int W, int y, int v)
{
    const uint8_t *p = plane + (long long)y * W + v * 16;
    if (vec) return *reinterpret_cast<const uint4 *>(p);
    uint32_t w[4] = {0, 0, 0, 0};
    const int in = W - v * 16;
#pragma unroll
    for (int c = 0; c < 16; ++c)
        if (c < in) w[c >> 2] |= (uint32_t)p[c] << (8 * (c & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}
__device__ __forceinline__ uint4 nz01x16(uint4 q) { return make_uint4(nz01(q.x), nz01(q.y), nz01(q.z), nz01(q.w)); }

// ---- 16 cells as 16 bits: bit j = cell 16 v + j of row y (0 <= y < H, 0 <= v < PV) lies on the grid and ...
// ... the mask (lo, hi) selects its status: the vector's status bytes & 7 (one load, however many masks), then the bits a mask selects among its `in` cells on the grid
template <class G> __device__ __forceinline__ uint4 status_vec7(CellPlanes pl, const G &g, int e, int y, int v) { return and4(*reinterpret_cast<const uint4 *>(cell_status_vec(pl, g, e, y, v)), 0x07070707u); }
__device__ __forceinline__ uint32_t mask_bits16(uint32_t lo, uint32_t hi, uint4 s7, int in) { return pack16(mask_sel01(lo, hi, s7)) & (in >= 16 ? 0xFFFFu : (1u << (in < 0 ? 0 : in)) - 1u); }
// ... its byte of a caller's dense plane is not 0 (dense_vec16 gives 0 for the bytes past the row's end)
__device__ __forceinline__ uint32_t dense_bits16(const uint8_t *plane, int vec, int W, int y, int v) { return pack16(nz01x16(dense_vec16(plane, vec, W, y, v))); }

// ---- the band searches (sf_bands.h).  What both read alike; each one's Args begins with one
struct BandArgs {
    Geo g;
    CellPlanes pl;               // the status bytes, in whichever plane is current
    const int32_t *envs;         // the listed environments of this chunk [cn]
    const uint8_t *passable;     // dense u8 [H * W] (pass_env = 0) or [E][H * W], or null
    long long pass_env;
    int pass_vec;                // 16-byte loads of passable (W % 16 == 0 and an aligned plane)
    const int32_t *points;       // this chunk's [cn][k][3] (column, row, id), or null
    int k;
    uint8_t *scratch;            // [cn][scratch_env]: the search's bit planes, then its halos
    long long scratch_env;
    uint32_t slo, shi, tlo, thi; // the mask of the cells a search starts from / goes through, as tables of one byte permute
    int conn8;
    int WORDS, BR, nb;           // words per row, band rows, bands = BR * WORDS
};
// The start and the open bits of word wi of row y: four status vectors through both masks, passable, and `also` - environment e's dense
// plane of further start cells (also_vec: 16-byte loads), or null; rows past the height, vectors past the pitch and the pitch padding give 0.
__device__ __forceinline__ void band_stage(const BandArgs &a, int e, int y, int wi, const uint8_t *also, int also_vec, unsigned long long &sd, unsigned long long &op)
{
    const Geo &g = a.g;
    sd = 0; op = 0;
    if (y >= g.H) return;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int v = wi * 4 + q;
        if (v >= g.PV) break;
        const uint4 s7 = status_vec7(a.pl, g, e, y, v);
        uint32_t s = mask_bits16(a.slo, a.shi, s7, g.W - v * 16), o = mask_bits16(a.tlo, a.thi, s7, g.W - v * 16);
        if (also) s |= dense_bits16(also, also_vec, g.W, y, v);
        if (a.passable) o &= dense_bits16(a.passable + a.pass_env * e, a.pass_vec, g.W, y, v);
        sd |= (unsigned long long)s << (16 * q);
        op |= (unsigned long long)o << (16 * q);
    }
}

}  // namespace
