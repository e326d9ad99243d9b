// Environment state: fork inside a handle (k_env_copy), snapshot into a caller buffer and restore from it (k_state_pack /
// k_state_unpack), and the vector bitmap of a restored environment (k_state_vbits).  Part of simfire_hip.hip only (the run units do
// not include it); the host side is sf_copy_envs / sf_save_state / sf_load_state there, the blob format is DESIGN.md section 11.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sf_common.h"
#include "sf_env_segs.h"

namespace {

// ------------------------------------------------------------------------------------------ fork
constexpr int kCopyPairs = 128;     // (src, dst) pairs per launch: they travel as kernel arguments, so an enqueued launch owns them
struct CopyList {
    EnvSeg seg[kEnvSegs];
    int n_seg;
    int32_t src[kCopyPairs], dst[kCopyPairs];
};

// blockIdx.y = pair, blockIdx.x with the grid's x extent strides over every slice (env_seg_walk, sf_env_segs.h).
__global__ __launch_bounds__(256) void k_env_copy(CopyList L)
{
    const int p = blockIdx.y;
    const long long gtid = (long long)blockIdx.x * blockDim.x + threadIdx.x, gstride = (long long)gridDim.x * blockDim.x;
    const long long se = L.src[p], de = L.dst[p];
    for (int k = 0; k < L.n_seg; ++k) {
        const EnvSeg c = L.seg[k];
        env_seg_walk<true>(c.base + de * c.stride, c.base + se * c.stride, c.len, gtid, gstride);
    }
}

// ------------------------------------------------------------------------------- snapshot / restore
// The blob of one environment (sf_save_state), whatever layout the handle has current:
//   [0, 128)     StateHeader
//   [128, 152)   EnvState (commit)          [160, 192) result row (8 x int32)     [192, 200) elapsed_time (f64)
//   from 256, each section rounded up to 16 bytes: status u8 [H][W] (raw bytes), sprite masks [H][W] x ab bytes (little endian),
//   burn f64 [H][W] (the stored value: attenuation still owed is in settled), settled u32 [H][W] (attenuation on), parents u8 [H][W]
//   (spread graph on), arrival u32 [H][W] (arrival recording on: update + 1, 0 = never)
constexpr uint32_t kStateMagic = 0x54534653u;      // "SFST"
constexpr uint32_t kStateVersion = 1u;
struct StateHeader {
    uint32_t magic, version;
    int64_t bytes;                                 // the whole blob
    int32_t H, W, md, ab;
    int32_t diag, att, has_max_time, prune_after_quit;
    int32_t has_parents, fire_rows, has_arrival, reserved1;    // fire_rows: the saving handle's bound on the fire's height (0 = none)
    double max_time, update_rate, pixel_scale;
    uint8_t pad[40];
};
static_assert(sizeof(StateHeader) == 128, "StateHeader is 128 bytes");
constexpr long long kStateFixed = 256;
__host__ __device__ inline long long st_round(long long b) { return (b + 15) / 16 * 16; }
struct StateLayout {
    long long status, age, burn, settled, parents, arrival, bytes;
};
__host__ __device__ inline StateLayout state_layout(const Geo &g, bool parents, bool arrival)
{
    const long long n = (long long)g.H * g.W;
    StateLayout l;
    l.status = kStateFixed;
    l.age = l.status + st_round(n);
    l.burn = l.age + st_round(n * g.ab);
    l.settled = l.burn + st_round(n * 8);
    l.parents = l.settled + (g.att ? st_round(n * 4) : 0);
    l.arrival = l.parents + (parents ? st_round(n) : 0);
    l.bytes = l.arrival + (arrival ? st_round(n * 4) : 0);
    return l;
}

constexpr int kStateEnvs = 128;     // environments per launch (their numbers travel as kernel arguments)
struct StateArgs {
    Geo g;
    CellPlanesMut pl;                              // the status bytes - and, blocked, the sprite masks - in whichever plane is current
    uint8_t *age;                                  // the row-major sprite masks
    double *burn;
    uint32_t *settled;
    uint8_t *parents;
    uint32_t *arrival;                             // null: arrival recording is off
    unsigned long long *vbits;
    EnvState *commit;
    int32_t *res_block, *res_sink;
    double *res_elapsed;
    uint8_t *blob;                                 // blob of list entry i at blob + i * stride
    long long stride;
    StateLayout lay;
    StateHeader hdr;                               // (pack) written in front of every blob
    int n;
    int32_t env[kStateEnvs];
};

// One thread per cell of row blockIdx.y, environment entry blockIdx.z; the first workgroup of an entry also writes the header and
// the EnvState / result row / elapsed_time.
__global__ __launch_bounds__(256) void k_state_pack(StateArgs a)
{
    const Geo &g = a.g;
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, i = blockIdx.z, e = a.env[i];
    uint8_t *b = a.blob + (long long)i * a.stride;
    if (blockIdx.x == 0 && y == 0) {
        const int t = threadIdx.x;
        if (t < 32) reinterpret_cast<uint32_t *>(b)[t] = reinterpret_cast<const uint32_t *>(&a.hdr)[t];
        else if (t < 38) reinterpret_cast<uint32_t *>(b + 128)[t - 32] = reinterpret_cast<const uint32_t *>(a.commit + e)[t - 32];
        else if (t < 40) reinterpret_cast<uint32_t *>(b + 128)[t - 32] = 0u;
        else if (t < 48) reinterpret_cast<int32_t *>(b + 160)[t - 40] = a.res_block[(long long)e * 8 + t - 40];
        else if (t == 48) *reinterpret_cast<double *>(b + 192) = a.res_elapsed[e];
        else if (t >= 50 && t < 64) reinterpret_cast<uint32_t *>(b + 200)[t - 50] = 0u;      // [200, 256)
        else if (t == 64) {      // the padding behind every section: a blob holds nothing but the state (two saves of one state are equal)
            const long long n = (long long)g.H * g.W;
            const long long ends[6] = {a.lay.status + n, a.lay.age + n * g.ab, a.lay.burn + n * 8, g.att ? a.lay.settled + n * 4 : a.lay.parents,
                                       a.parents ? a.lay.parents + n : a.lay.arrival, a.arrival ? a.lay.arrival + n * 4 : a.lay.bytes};
            const long long nexts[6] = {a.lay.age, a.lay.burn, a.lay.settled, a.lay.parents, a.lay.arrival, a.lay.bytes};
            for (int k = 0; k < 6; ++k)
                for (long long q = ends[k]; q < nexts[k]; ++q) b[q] = 0u;
        }
    }
    if (x >= g.W) return;
    const long long c = (long long)y * g.W + x, o = (long long)e * g.plane_env + (long long)y * g.P + x;
    uint8_t st;
    uint32_t m;
    if (a.pl.cells) {
        const uint8_t *sp = bl_status(a.pl.cells, g, e, y, x);
        m = *bl_mask_beside(sp);
        st = *sp;
    } else {
        m = age_load(g, a.age + (long long)e * g.age_env * g.ab, (long long)y * g.P + x);
        st = a.pl.status[o];
    }
    b[a.lay.status + c] = st;
    uint8_t *ma = b + a.lay.age + c * g.ab;
    for (int k = 0; k < g.ab; ++k) ma[k] = (uint8_t)(m >> (8 * k));
    reinterpret_cast<double *>(b + a.lay.burn)[c] = a.burn[o];
    if (g.att) reinterpret_cast<uint32_t *>(b + a.lay.settled)[c] = a.settled[o];
    if (a.parents) b[a.lay.parents + c] = a.parents[o];
    if (a.arrival) reinterpret_cast<uint32_t *>(b + a.lay.arrival)[c] = a.arrival[o];
}

// The reverse, into the layout that is current.  The caller has zeroed the environment's cell planes (guard rows / quads and pitch
// padding stay zero); threads past W write the zero padding of burn / settled / parents.
__global__ __launch_bounds__(256) void k_state_unpack(StateArgs a)
{
    const Geo &g = a.g;
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, i = blockIdx.z, e = a.env[i];
    const uint8_t *b = a.blob + (long long)i * a.stride;
    if (blockIdx.x == 0 && y == 0) {
        const int t = threadIdx.x;
        if (t < 6) reinterpret_cast<uint32_t *>(a.commit + e)[t] = reinterpret_cast<const uint32_t *>(b + 128)[t];
        else if (t >= 8 && t < 16) {
            const int32_t v = reinterpret_cast<const int32_t *>(b + 160)[t - 8];
            a.res_block[(long long)e * 8 + t - 8] = v;
            if (a.res_sink) a.res_sink[(long long)e * 8 + t - 8] = v;
        } else if (t == 16) a.res_elapsed[e] = *reinterpret_cast<const double *>(b + 192);
    }
    if (x >= g.P) return;
    const long long o = (long long)e * g.plane_env + (long long)y * g.P + x;
    if (x >= g.W) {
        a.burn[o] = 0.0;
        if (g.att) a.settled[o] = 0u;
        if (a.parents) a.parents[o] = 0u;
        if (a.arrival) a.arrival[o] = 0u;
        return;
    }
    const long long c = (long long)y * g.W + x;
    const uint8_t st = b[a.lay.status + c];
    const uint8_t *ma = b + a.lay.age + c * g.ab;
    uint32_t m = 0;
    for (int k = 0; k < g.ab; ++k) m |= (uint32_t)ma[k] << (8 * k);
    if (a.pl.cells) {
        uint8_t *sp = bl_status(a.pl.cells, g, e, y, x);
        *bl_mask_beside(sp) = (uint8_t)m;
        *sp = st;
    } else {
        age_store(g, a.age + (long long)e * g.age_env * g.ab, (long long)y * g.P + x, m);
        a.pl.status[o] = st;
    }
    a.burn[o] = reinterpret_cast<const double *>(b + a.lay.burn)[c];
    if (g.att) a.settled[o] = reinterpret_cast<const uint32_t *>(b + a.lay.settled)[c];
    if (a.parents) a.parents[o] = b[a.lay.parents + c];
    if (a.arrival) a.arrival[o] = reinterpret_cast<const uint32_t *>(b + a.lay.arrival)[c];
}

// The three planes of the vector bitmap of a restored environment, from the blob's sprite masks (so that the blocked plane and the
// row-major planes are served alike): one wave per (row, 64-vector word), as k_rebuild_vbits.
__global__ __launch_bounds__(64) void k_state_vbits(StateArgs a)
{
    const Geo &g = a.g;
    const int w = blockIdx.x, y = blockIdx.y, i = blockIdx.z, e = a.env[i], lane = threadIdx.x;
    const int v = w * 64 + lane;
    const uint8_t *ma = a.blob + (long long)i * a.stride + a.lay.age + (long long)y * g.W * g.ab;
    bool any = false, first = false, last = false;
    if (v < g.PV)
        for (int j = 0; j < 16; ++j) {
            const int x = v * 16 + j;
            if (x >= g.W) break;
            bool nz = false;
            for (int k = 0; k < g.ab; ++k) nz |= ma[(long long)x * g.ab + k] != 0;
            any |= nz;
            if (j == 0) first = nz;
            if (j == 15) last = nz;
        }
    const unsigned long long bb = __ballot(any), f = __ballot(first), l = __ballot(last);
    if (lane == 0) {
        const long long o = (long long)e * g.vb_env + (long long)y * g.VW + w, plane = (long long)g.E * g.vb_env;
        a.vbits[o] = bb; a.vbits[plane + o] = f; a.vbits[2 * plane + o] = l;      // any sprite bit / in the first cell / in the last cell
    }
}

}  // namespace
