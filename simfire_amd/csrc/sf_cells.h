// The cell planes as every kernel off the step path reads and writes them: the arithmetic of the blocked plane, and the accessors that
// find a cell's status byte in whichever plane is current.  The only place that knows the blocked layout.  Plain C++17, no HIP:
// tests/cells_check.cpp drives it on its own (SF_HD is plain `inline` under a host compiler).
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__HIP__)
#define SF_HD __host__ __device__ inline __attribute__((always_inline))      // (inlined before anything is optimised: a kernel compiles as if written out)
#else
#define SF_HD inline
#endif

namespace {

// ------------------------------------------------------------------------------------------
// Blocked cell plane of the resident launch (k_run).  A 16-cell vector visit needs the sprite masks of rows y - 1, y, y + 1
// and the status bytes of row y: four 64-byte sectors in four different lines of the row-major planes.  Here a SECTOR holds,
// for one 16-cell vector and one PAIR of rows (2p, 2p + 1):  [mask row 2p | mask row 2p + 1 | status row 2p | status row 2p + 1],
// and the two pairs of a row quad share a 128-byte line (the lines of a quad row run along x).  A visit then touches exactly
// two sectors - the pair of y, and the pair above (y even) or below (y odd) - in one line (y mod 4 = 1, 2) or two.
// One guard quad above and below every environment (row -1 and row H are zero for ever); offsets count from quad 0.
// PV: 16-cell vectors per row (Geo).
SF_HD constexpr int bl_vec(int PV, int y, int v)      // byte offset of the sector of (row pair of y, vector v)
{
    return ((y >> 2) * PV + v) * 128 + ((y >> 1) & 1) * 64;
}
SF_HD constexpr int bl_cell(int PV, int y, int x)     // sprite mask of cell (y, x); its status byte is kBlStatus further
{
    return bl_vec(PV, y, x >> 4) + (y & 1) * 16 + (x & 15);
}
constexpr int kBlStatus = 32;      // status row = mask row + 32 inside a sector
SF_HD long long bl_env_bytes(int H, int PV)      // bytes of the plane per environment, guard quads included (Geo's cells_env)
{
    return (long long)((H + 3) / 4 + 2) * PV * 128;
}

// What the accessors below need of Geo.  They take "anything with these fields": a kernel that carries a whole Geo passes that.
struct CellGeo {
    int H, W, P, PV;                     // the grid, the row pitch and its 16-cell vectors
    long long plane_env, cells_env;      // cells of a row-major plane, bytes of the blocked plane per environment
};
template <class G> inline CellGeo cell_geo(const G &g) { return CellGeo{g.H, g.W, g.P, g.PV, g.plane_env, g.cells_env}; }

// The status bytes of every environment: the row-major plane, and the blocked plane when IT is the current one (else null).
template <class B> struct CellView {
    B *status, *cells;
};
typedef CellView<const uint8_t> CellPlanes;
typedef CellView<uint8_t> CellPlanesMut;

// ---- the blocked plane alone (cells != null): sprite masks and status bytes of one-byte cells
template <class B, class G> SF_HD B *bl_mask_vec(B *cells, const G &g, int e, int y, int v)      // the 16 masks of vector v in row y
{
    return cells + (long long)e * g.cells_env + bl_vec(g.PV, y, v) + (y & 1) * 16;
}
template <class B, class G> SF_HD B *bl_mask(B *cells, const G &g, int e, int y, int x)
{
    return cells + (long long)e * g.cells_env + bl_cell(g.PV, y, x);
}
template <class B, class G> SF_HD B *bl_status_vec(B *cells, const G &g, int e, int y, int v)
{
    return cells + (long long)e * g.cells_env + bl_vec(g.PV, y, v) + (y & 1) * 16 + kBlStatus;
}
template <class B, class G> SF_HD B *bl_status(B *cells, const G &g, int e, int y, int x)
{
    return cells + (long long)e * g.cells_env + bl_cell(g.PV, y, x) + kBlStatus;
}
template <class B> SF_HD B *bl_mask_beside(B *status_byte) { return status_byte - kBlStatus; }      // the same cell's sprite mask

// ---- whichever plane is current
template <class B, class G> SF_HD B *cell_status(CellView<B> p, const G &g, int e, int y, int x)      // the status byte of cell (y, x)
{
    return p.cells ? bl_status(p.cells, g, e, y, x) : p.status + (long long)e * g.plane_env + (long long)y * g.P + x;
}
// the 16 status bytes of vector v in row y (16-byte aligned).  y, v: int, or the 64-bit row and vector of a window that may lie off
// the grid (k_observe) - on the grid when this is called, and the row-major offset is then made from the 64-bit values as they are
template <class B, class G, class Y, class V> SF_HD B *cell_status_vec(CellView<B> p, const G &g, int e, Y y, V v)
{
    return p.cells ? bl_status_vec(p.cells, g, e, (int)y, (int)v) : p.status + (long long)e * g.plane_env + (long long)y * g.P + v * 16;
}
// the aligned dword that holds the status byte of cell (y, x), at byte x & 3 of it (the atomics of the mitigation kernels).
// o = e * plane_env + y * P + x, the cell's offset in a row-major plane: those kernels hold it for burn[] and settled[]
template <class G> SF_HD uint32_t *cell_status_word(CellPlanesMut p, const G &g, int e, int y, int x, long long o)
{
    return reinterpret_cast<uint32_t *>(p.cells ? bl_status(p.cells, g, e, y, x & ~3) : p.status + (o & ~3ll));
}

}  // namespace
