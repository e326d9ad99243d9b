// What the spatial queries (sf_distance ... sf_influence) share on the device: status masks as byte-permute tables, the caller's
// points, wave reductions and the caller's dense u8 planes.  With sf_cells.h (where the status bytes are) the starting point of a
// new query's kernels, as sf_host_query.h is of its host side.  Part of the single translation unit simfire_hip.hip.
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
__device__ __forceinline__ uint32_t mask_sel16(uint32_t lo, uint32_t hi, uint4 q) { return pack16(mask_sel01(lo, hi, q)); }

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

}  // namespace
