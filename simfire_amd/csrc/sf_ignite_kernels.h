// Ignitions during an episode (sf_ignite, sf_ignite_device): new sprites written into environments that are
// running, many cells and environments in one launch, from rows in device memory.  A writer in front of the step kernels, like the
// control-line scatter (k_mitigate_*, sf_aux_kernels.h): no step kernel knows about it.  Part of simfire_hip.hip only.
//
// The reference keeps its sprites in a list ordered by age and, inside an age, by (y, x) (fire.py:102-103, 566-587); a sprite of
// duration 0 inserted there between two update() calls cannot be told from one the last update() created.  The sprite masks are indexed
// by ABSOLUTE ignition step (sf_common.h, make_masks), so that sprite is bit slot_of(t, N) of its cell's mask with t = commit[e].steps,
// the updates the episode has made: the bit k_reset_ignite sets for t = 0 (sf_reset_kernels.h), and per cell taken this kernel writes
// what that one writes for its cell.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sf_common.h"

namespace {

struct IgniteArgs {
    Geo g;
    const int32_t *pts;                  // [n][4] = (env, column, row, reserved = 0), 16-byte aligned
    int n;
    CellPlanesMut pl;                    // the status bytes - and, blocked, the sprite masks - in whichever plane is current
    uint8_t *age;                        // the row-major sprite masks
    const EnvState *commit;              // current: the call has folded the step rings
    uint8_t *tflags;                     // null unless the tile activity map is kept (row-major planes current, map valid)
    int ring;
    uint8_t *seam;                       // null unless the map is kept and the sprite plane is 1 byte wide
    uint8_t *tdirty;                     // null unless the tile histograms are known
    unsigned long long *vbits;           // null unless plane 0 of the vector bitmap matches the masks
    unsigned long long *win_hint;
};

// One lane per row.  A row is skipped when a field is out of range or reserved != 0 (the host form has refused those), when its
// environment is not running or its cell is not UNBURNED.  Rows of one launch that name the same cell store the same bytes, whichever
// of them finds the cell UNBURNED; rows that share a bitmap word meet in atomicOr.  A structure that is not valid is not written: its
// rebuild finds the cell in the masks.  Neither EnvState nor the result row is written.
__global__ __launch_bounds__(256) void k_ignite(IgniteArgs a)
{
    const Geo &g = a.g;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const int4 q = reinterpret_cast<const int4 *>(a.pts)[i];
    const int e = q.x, x = q.y, y = q.z;
    if (q.w != 0 || e < 0 || e >= g.E || x < 0 || x >= g.W || y < 0 || y >= g.H) return;
    if (a.commit[e].running != 1) return;               // finished, or QUIT and still pruning
    const uint32_t bit = 1u << slot_of(a.commit[e].steps, g.N);      // the sprite update `steps` would have created
    const long long o = (long long)y * g.P + x;
    if (a.pl.cells) {                   // the blocked cell plane is the current one (1-byte sprite masks)
        uint8_t *sp = bl_status(a.pl.cells, g, e, y, x);
        if (*sp != SF_UNBURNED) return;
        *sp = SF_BURNING;
        uint8_t *mp = bl_mask_beside(sp);
        *mp = (uint8_t)(*mp | bit);     // OR-ed: sf_load_fire_map can leave an old bit under an UNBURNED byte
    } else {
        uint8_t *sp = cell_status(a.pl, g, e, y, x);
        if (*sp != SF_UNBURNED) return;
        *sp = SF_BURNING;
        uint8_t *base = a.age + (long long)e * g.age_env * g.ab;
        age_store(g, base, o, age_load(g, base, o) | bit);
    }
    const int tyw = y / (g.LR * g.RB), tx = (x / 16) / g.LC;
    if (a.tdirty) a.tdirty[((long long)e * g.TY + tyw) * g.TX + tx] = 1;
    if (a.seam) {                       // the copies of the sprite columns either side of a chunk boundary (k_rebuild_seams)
        const int cw = g.LC * 16;
        int b = -1, side = 0;
        if ((x + 1) % cw == 0) { b = (x + 1) / cw; side = 0; }
        else if (x % cw == 0) { b = x / cw; side = 1; }
        if (b >= 1 && b < g.chunks_x) {
            uint8_t *sm = a.seam + (long long)e * g.seam_env + (long long)(b * 2 + side) * g.Hs + y + kSeamPad;
            *sm = (uint8_t)(*sm | bit);
        }
    }
    if (a.tflags) {                     // all edge bits: conservative, and OR-ed - the tile may hold the old fire
        uint8_t *tf = a.tflags + (((long long)a.ring * g.E + e) * g.TYp + tyw + 1) * g.TXp + tx + 1;
        *tf = (uint8_t)(*tf | (1 | 4 | 8 | 16 | 32));
    }
    if (a.vbits) {                      // (planes 1 / 2 may be stale on rows of several words: a team launch rebuilds all three then)
        const long long w = (long long)e * g.vb_env + (long long)y * g.VW + (x >> 10), plane = (long long)g.E * g.vb_env;
        const unsigned long long vb = 1ull << ((x >> 4) & 63);
        atomicOr(a.vbits + w, vb);
        if ((x & 15) == 0) atomicOr(a.vbits + plane + w, vb);
        if ((x & 15) == 15) atomicOr(a.vbits + 2 * plane + w, vb);
    }
    a.win_hint[e] = 0ull;               // (where the window stood says nothing about a fire with this cell in it)
}

}  // namespace
