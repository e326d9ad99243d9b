// The per-environment slices of a handle's buffers: what a fork copies, a reset zeroes and a restore clears, described once per call
// (env_segs in simfire_hip.hip enumerates them for the layout that is current; DESIGN.md section 11 says what each is).  Part of
// simfire_hip.hip only; k_env_copy (sf_state_kernels.h) and k_reset_envs (sf_reset_kernels.h) walk them with env_seg_walk.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

// One slice: environment e's bytes are [base + e * stride, base + e * stride + len).
struct EnvSeg {
    uint8_t *base;
    long long stride, len;
};
// What a slice is (a bit each, so that a caller names the set it wants).  In the order env_segs lists them, with the slices of each:
enum EnvKind : unsigned {
    kSegCells = 1u << 0,        // the cells of the current layout: the blocked plane (1), or status + the sprite-mask plane (2)
    kSegBurn = 1u << 1,         // burn (1)
    kSegSettled = 1u << 2,      // settled, attenuation on (1)
    kSegParents = 1u << 3,      // spread-graph parent masks, where they exist (1)
    kSegSnap = 1u << 4,         // the map as the host last saw it, where it exists (1)
    kSegState = 1u << 5,        // EnvState in commit[] (1)
    kSegResult = 1u << 6,       // result row, elapsed_dev entry, the caller's sink row where there is one (3)
    kSegTflags = 1u << 7,       // both rings of the tile activity map (2)
    kSegVbits = 1u << 8,        // the three planes of the vector bitmap (3)
    kSegSeam = 1u << 9,         // seam columns (1)
    kSegHist = 1u << 10,        // tile histograms: tdirty + thist (2)
    kSegHint = 1u << 11,        // window advice win_hint (1)
    kSegCost = 1u << 12,        // launch-order cost run_cost (1)
    kSegTerrain = 1u << 13,     // per table: rt, lay_all, the cell-major rtc where it exists (3)
};
// The largest selections: a fork copies the state and everything derived from it (22 slices with the terrain), a batched reset
// zeroes these (14; the ignition, the state and the result row are written behind the zeroing).  Callers take kinds off by their
// own conditions.
constexpr unsigned kForkKinds = kSegCells | kSegBurn | kSegSettled | kSegParents | kSegState | kSegResult | kSegTflags | kSegVbits | kSegSeam |
                                kSegHist | kSegHint | kSegCost | kSegTerrain;
constexpr unsigned kResetKinds = kSegCells | kSegBurn | kSegSettled | kSegParents | kSegSnap | kSegTflags | kSegVbits | kSegSeam | kSegHist;
constexpr int kEnvSegs = 24;        // slices a kernel argument holds: enough for every selection (tests/test_reset_batch_cpu.py counts them)

// The bytes of one slice [dst, dst + len), spread over the launch's lanes (gtid of gstride).  A slice whose ends sit on 16-byte
// boundaries goes in 16-byte vectors, numbered from the 128-byte line dst starts in: the 8 lanes of a line write it whole (or the
// part of it that belongs to the slice - the neighbour environment's bytes are never touched), the ragged last vector byte by byte.
// Other slices (the 24-byte EnvState, per-environment words, the tile flag planes) are a few hundred bytes and go byte by byte.
// COPY: the bytes come from src (which must be 16-byte aligned too for the vector path); else zeros are stored and nothing is read.
template <bool COPY>
__device__ __forceinline__ void env_seg_walk(uint8_t *dst, const uint8_t *src, long long len, long long gtid, long long gstride)
{
    if ((((COPY ? (uintptr_t)src : 0) | (uintptr_t)dst) & 15) == 0) {
        const long long head = (long long)((uintptr_t)dst & 127);          // bytes of the first line in front of the slice
        const long long units = (head + len + 15) >> 4;
        for (long long u = gtid; u < units; u += gstride) {
            const long long o = u * 16 - head;                              // slice offset of this vector (16-aligned, may be < 0)
            if (o < 0) continue;
            if (o + 16 <= len) {
                *reinterpret_cast<uint4 *>(dst + o) = COPY ? *reinterpret_cast<const uint4 *>(src + o) : make_uint4(0u, 0u, 0u, 0u);
            } else {
                for (long long b = o; b < len; ++b) dst[b] = COPY ? src[b] : (uint8_t)0;
            }
        }
    } else {
        for (long long b = gtid; b < len; b += gstride) dst[b] = COPY ? src[b] : (uint8_t)0;
    }
}

}  // namespace
