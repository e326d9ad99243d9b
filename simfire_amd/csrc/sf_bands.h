// The band scheme of the bit-plane searches (the flood fill of DESIGN.md section 23, the breadth-first levels of section 24): all of
// it that is arithmetic.  One bit per cell, 64 cells per word, ceil(P / 64) words per row.  A BAND is one word column times kBandRows
// consecutive rows; a thread owns a band, keeps its words in registers and sees its eight neighbours through a HALO: every band
// publishes its first row, its last row and its two edge columns, and reads the neighbours' between two rounds.  Planes are
// band-major, so a band's words are neighbours in memory.  Plain C++17, no HIP: tests/bands_check.cpp emulates a workgroup with it on
// the host (SF_HD is plain `inline` under a host compiler, as in sf_cells.h).
#pragma once
#include <cstdint>

#if !defined(SF_HD) && (defined(__HIPCC__) || defined(__HIP__))
#define SF_HD __host__ __device__ inline __attribute__((always_inline))      // (inlined before anything is optimised: a kernel compiles as if written out)
#elif !defined(SF_HD)
#define SF_HD inline
#endif
// A scheduling barrier of the device compiler and its unroll pragma; nothing anywhere else
#if defined(__HIP_DEVICE_COMPILE__)
#define SF_BAND_SCHED_BARRIER() __builtin_amdgcn_sched_barrier(0)
#define SF_BAND_UNROLL _Pragma("unroll")
#else
#define SF_BAND_SCHED_BARRIER() ((void)0)
#define SF_BAND_UNROLL
#endif

namespace {

typedef unsigned long long band_word;
constexpr int kBandRows = 16;                 // rows of a band: its words are 16 x 2 = 32 VGPRs
constexpr int kBandThreads = 1024;            // the workgroup of a search: grids of at most as many bands have one band per thread
constexpr int kBandLdsRow = kBandRows + 1;    // a thread's 16 words in LDS and one of padding: the 8-byte reads of a wave's lanes fall on all banks

// ---- geometry
SF_HD int band_words(int P) { return (P + 63) / 64; }                            // words per row of a pitch of P cells
SF_HD int band_rows(int H) { return (H + kBandRows - 1) / kBandRows; }           // band rows of H rows; bands = band rows * words
// bytes of scratch per environment: `planes` bit planes of whole bands, and per halo two words and one edge dword per band
SF_HD long long band_env_bytes(long long nb, int planes, int halos) { return (nb * kBandRows * 8 * planes + nb * 20 * halos + 255) / 256 * 256; }
// Where word wi of row y lies in a bit plane: band-major - the 16 words of a band are neighbours, so a thread reads and writes its
// band with 16-byte accesses at constant offsets from one address
SF_HD long long band_at(int WORDS, int y, int wi) { return ((long long)(y / kBandRows) * WORDS + wi) * kBandRows + (y % kBandRows); }

// ---- bits
SF_HD band_word band_brev(band_word x)       // bit i <-> bit 63 - i
{
#if defined(__has_builtin) && __has_builtin(__builtin_bitreverse64)
    return __builtin_bitreverse64(x);
#else
    x = ((x >> 1) & 0x5555555555555555ull) | ((x & 0x5555555555555555ull) << 1);
    x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    x = ((x >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
    return __builtin_bswap64(x);
#endif
}
// 4 bits -> 4 bytes of 0 / 1, and 16 bits -> 16 such bytes
SF_HD uint32_t bits_bytes4(uint32_t n) { return ((n & 0xFu) * 0x00204081u) & 0x01010101u; }
SF_HD void bits_bytes16(uint32_t b, uint32_t (&d)[4]) { d[0] = bits_bytes4(b); d[1] = bits_bytes4(b >> 4); d[2] = bits_bytes4(b >> 8); d[3] = bits_bytes4(b >> 12); }

// What row y takes from a neighbouring row w: the row itself, and with diagonals its two shifts - l / r: bit 63 of the word to the
// left / bit 0 of the word to the right of w
SF_HD band_word band_spread(band_word w, band_word l, band_word r, int conn8) { return conn8 ? (w | (w << 1) | (w >> 1) | l | (r << 63)) : w; }
// The fill along a row inside one word: every run of open bits that holds or touches a bit of w is filled.  Towards the higher bits
// the carry of ONE add runs through a run of open bits (o + G clears the run from the generator up; the generators themselves are
// or-ed back in); towards the lower bits the same on the reversed words.  cl / cr: the neighbouring words' bit 63 / bit 0.
SF_HD band_word band_fill(band_word w, band_word o, band_word cl, band_word cr)
{
    const band_word gu = (w | (w << 1) | cl) & o;
    w |= (((o + gu) ^ o) & o) | gu;
    const band_word gd = (w | (w >> 1) | (cr << 63)) & o;
    const band_word ro = band_brev(o), rg = band_brev(gd);
    w |= band_brev(((ro + rg) ^ ro) & ro) | gd;
    return w;
}
// bit 0 of the band's rows in bits 0..15, bit 63 of them in bits 16..31
SF_HD uint32_t band_edges(const band_word (&f)[kBandRows])
{
    uint32_t ed = 0;
    SF_BAND_UNROLL
    for (int j = 0; j < kBandRows; ++j) ed |= ((uint32_t)f[j] & 1u) << j | (uint32_t)(f[j] >> 63) << (16 + j);
    return ed;
}

// ---- a band in memory.  base[bytes / sizeof(T)] with a 32-bit byte offset (a plane of one environment is far below 4 GiB): one
// uniform base and one 32-bit register per access instead of a 64-bit address each
template <class T> SF_HD T &band_ref(T *base, uint32_t bytes) { return *(T *)((char *)base + bytes); }
// the 16 words of band b of a plane, to and from f[0 .. 15] (registers, or a thread's row in LDS)
SF_HD void band_load(band_word *f, const band_word *plane, int b)
{
    SF_BAND_UNROLL
    for (int j = 0; j < kBandRows; ++j) f[j] = band_ref(plane, (uint32_t)b * (kBandRows * 8u) + j * 8u);
}
SF_HD void band_store(band_word *plane, int b, const band_word *f)
{
    SF_BAND_UNROLL
    for (int j = 0; j < kBandRows; ++j) band_ref(plane, (uint32_t)b * (kBandRows * 8u) + j * 8u) = f[j];
}

// ---- the halo: three arrays of one entry per band.  What band b shows its neighbours ...
SF_HD void band_publish(band_word *h_top, band_word *h_bot, uint32_t *h_edge, int b, const band_word (&f)[kBandRows])
{
    band_ref(h_top, (uint32_t)b * 8u) = f[0]; band_ref(h_bot, (uint32_t)b * 8u) = f[kBandRows - 1]; band_ref(h_edge, (uint32_t)b * 4u) = band_edges(f);
}
struct BandHalo {            // ... and what band (br, wi) reads of its eight neighbours: 0 past the grid
    band_word top, bot;      // the row above its first / below its last row, its own word column
    uint32_t el, er;         // rows -1 .. 16 of the column to its left (bit 63 of that word) / to its right (bit 0): bit j + 1 = row j
};
SF_HD BandHalo band_halo(int WORDS, int BR, const band_word *h_top, const band_word *h_bot, const uint32_t *h_edge, int br, int wi)
{
    const int b = br * WORDS + wi;
    const bool up = br > 0, dn = br + 1 < BR, lf = wi > 0, rt = wi + 1 < WORDS;
    BandHalo h;
    const uint32_t b8 = (uint32_t)b * 8u, W8 = (uint32_t)WORDS * 8u;
    h.top = up ? band_ref(h_bot, b8 - W8) : 0;
    h.bot = dn ? band_ref(h_top, b8 + W8) : 0;
    const uint32_t edl = lf ? band_ref(h_edge, (uint32_t)b * 4u - 4u) : 0, edr = rt ? band_ref(h_edge, (uint32_t)b * 4u + 4u) : 0;
    const band_word tl = up && lf ? band_ref(h_bot, b8 - W8 - 8u) : 0, tr = up && rt ? band_ref(h_bot, b8 - W8 + 8u) : 0;
    const band_word bl = dn && lf ? band_ref(h_top, b8 + W8 - 8u) : 0, brw = dn && rt ? band_ref(h_top, b8 + W8 + 8u) : 0;
    h.el = (edl >> 16) << 1 | (uint32_t)(tl >> 63) | (uint32_t)(bl >> 63) << 17;
    h.er = (edr & 0xFFFFu) << 1 | ((uint32_t)tr & 1u) | ((uint32_t)brw & 1u) << 17;
    return h;
}

// ---- the flood fill.  One round of a band: the sweep down, the sweep up (Gauss-Seidel: row y takes spread(row y -+ 1) & open, then
// fills along the row).  The band's open words are read where they are used (ob[j]: LDS, or the scratch plane) - only F stays in
// registers.  Returns whether a bit was added.  (Without the scheduling barriers every row's read of ob and bit reversal is hoisted to the top of the sweep: spills.)
SF_HD bool band_round(band_word (&f)[kBandRows], const band_word *ob, const BandHalo &h, int conn8)
{
    band_word changed = 0;
    SF_BAND_UNROLL
    for (int j = 0; j < kBandRows; ++j) {
        const band_word o = ob[j];
        const band_word prev = j == 0 ? h.top : f[j - 1];
        band_word w = f[j] | (band_spread(prev, (h.el >> j) & 1u, (h.er >> j) & 1u, conn8) & o);
        w = band_fill(w, o, (h.el >> (j + 1)) & 1u, (h.er >> (j + 1)) & 1u);
        changed |= w ^ f[j];
        f[j] = w;
        if (j & 1) SF_BAND_SCHED_BARRIER();
    }
    SF_BAND_UNROLL
    for (int j = kBandRows - 1; j >= 0; --j) {
        const band_word o = ob[j];
        const band_word next = j == kBandRows - 1 ? h.bot : f[j + 1];
        band_word w = f[j] | (band_spread(next, (h.el >> (j + 2)) & 1u, (h.er >> (j + 2)) & 1u, conn8) & o);
        w = band_fill(w, o, (h.el >> (j + 1)) & 1u, (h.er >> (j + 1)) & 1u);
        changed |= w ^ f[j];
        f[j] = w;
        if (j & 1) SF_BAND_SCHED_BARRIER();
    }
    return changed != 0;
}

// ---- the breadth-first search.  One level of a band, in place: f (the front) becomes dilate(f) & U, and those cells leave U (ub:
// the band's 16 words of U, LDS or the scratch plane).  Jacobi: every row is dilated from the OLD rows - the one above is carried in
// prev, the one below is still untouched.  Returns whether a cell was added.
SF_HD bool band_level(band_word (&f)[kBandRows], band_word *ub, const BandHalo &h, int conn8)
{
    band_word any = 0, prev = h.top;
    SF_BAND_UNROLL
    for (int j = 0; j < kBandRows; ++j) {
        const band_word cur = f[j], next = j == kBandRows - 1 ? h.bot : f[j + 1];
        band_word w = (cur << 1) | (cur >> 1) | (band_word)((h.el >> (j + 1)) & 1u) | (band_word)((h.er >> (j + 1)) & 1u) << 63;
        w |= band_spread(prev, (h.el >> j) & 1u, (h.er >> j) & 1u, conn8) | band_spread(next, (h.el >> (j + 2)) & 1u, (h.er >> (j + 2)) & 1u, conn8);
        const band_word u = ub[j], nw = w & u;
        if (nw) ub[j] = u & ~nw;
        f[j] = nw;
        prev = cur;
        any |= nw;
        if ((j & 3) == 3) SF_BAND_SCHED_BARRIER();       // (keeps the U reads of all rows from being hoisted to the top)
    }
    return any != 0;
}

// ---- the growing set (the escape search of DESIGN.md section 30).  One level of a band: the WHOLE set a, not a front, is dilated -
// n = dilate(a) & U row by row, those cells join a and leave U (ub: the band's 16 words of U, LDS or the scratch plane; a and U are
// disjoint).  Jacobi as band_level: every row is dilated from the OLD rows.  added(j, n) is called for every row j that gained the
// cells n (the caller numbers them: no second array of rows is kept); returns whether a cell was added.
template <class Added>
SF_HD bool band_grow(band_word (&a)[kBandRows], band_word *ub, const BandHalo &h, int conn8, Added &&added)
{
    band_word any = 0, prev = h.top;
    SF_BAND_UNROLL
    for (int j = 0; j < kBandRows; ++j) {
        const band_word cur = a[j], next = j == kBandRows - 1 ? h.bot : a[j + 1];
        band_word w = (cur << 1) | (cur >> 1) | (band_word)((h.el >> (j + 1)) & 1u) | (band_word)((h.er >> (j + 1)) & 1u) << 63;
        w |= band_spread(prev, (h.el >> j) & 1u, (h.er >> j) & 1u, conn8) | band_spread(next, (h.el >> (j + 2)) & 1u, (h.er >> (j + 2)) & 1u, conn8);
        const band_word u = ub[j], n = w & u;
        if (n) {
            ub[j] = u & ~n;
            a[j] = cur | n;
            added(j, n);
        }
        prev = cur;
        any |= n;
        if ((j & 3) == 3) SF_BAND_SCHED_BARRIER();
    }
    return any != 0;
}

}  // namespace
