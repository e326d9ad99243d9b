// Connected components (sf_components): all of it that is arithmetic.  One bit per selected cell, 64 cells per
// word, ceil(W / 64) words per row (row-major: word wi of row y at y * WORDS + wi); a label plane of one int32 per cell, dense, that
// holds a parent index y * W + x or -1.  Here: the runs of a word and the carry of a run across words (phase 1), where a contact with
// the row above BEGINS (phase 2), the union and the find as the kernel does them, the scan that ranks the roots (phase 4), the runs a
// stats lane walks and the touch word of a run (phase 5).  Plain C++17, no HIP: tests/components_check.cpp emulates the phases with it
// on the host (SF_HD is plain `inline` under a host compiler, as in sf_cells.h).  The starting point of a query whose answer is a
// partition; sf_bands.h is that of one whose answer is a set.
#pragma once
#include <cstdint>

#if !defined(SF_HD) && (defined(__HIPCC__) || defined(__HIP__))
#define SF_HD __host__ __device__ inline __attribute__((always_inline))
#elif !defined(SF_HD)
#define SF_HD inline
#endif

namespace {

typedef unsigned long long cc_word;
constexpr int kCompMaxCap = 4096;             // max_components at most
constexpr int kCompScanThreads = 256;         // the threads that share the scan over the rows' root counts

// ---- geometry
SF_HD int cc_words(int W) { return (W + 63) / 64; }
SF_HD long long cc_round(long long b) { return (b + 255) / 256 * 256; }
// bytes of scratch per listed environment: the head (counters), the selected bits, the rows' root counts, the second plane (ranks,
// then sizes) and - unless the caller's labels output is the label plane - the label plane
constexpr int kCompHeadBytes = 256;           // the u64 key of the largest component at byte 8 (zeroed per chunk); the rest is padding
SF_HD long long cc_env_bytes(int H, int W, bool labels_out)
{
    const long long n = (long long)H * W;
    return kCompHeadBytes + cc_round((long long)H * cc_words(W) * 8) + cc_round(4ll * (H + 1)) + cc_round(4 * n) + (labels_out ? 0 : cc_round(4 * n));
}
SF_HD long long cc_off_bits() { return kCompHeadBytes; }
SF_HD long long cc_off_rows(int H, int W) { return cc_off_bits() + cc_round((long long)H * cc_words(W) * 8); }
SF_HD long long cc_off_aux(int H, int W) { return cc_off_rows(H, W) + cc_round(4ll * (H + 1)); }
SF_HD long long cc_off_par(int H, int W) { return cc_off_aux(H, W) + cc_round(4ll * H * W); }

// ---- bits
SF_HD int cc_popc(cc_word w) { return __builtin_popcountll(w); }
SF_HD int cc_ctz(cc_word w) { return __builtin_ctzll(w); }          // w != 0
SF_HD int cc_clz(cc_word w) { return __builtin_clzll(w); }          // w != 0
SF_HD cc_word cc_below(int bit) { return bit >= 64 ? ~0ull : (1ull << bit) - 1ull; }      // the bits under `bit` (0..64)
// the bits of a word that lie on the grid: the first `in` (W - 64 * wi; <= 0: none, >= 64: all)
SF_HD cc_word cc_on_grid(int in) { return in <= 0 ? 0ull : cc_below(in); }

// ---- phase 1: runs.  The bit at which the run of set bits that holds `bit` begins inside w (bit set); 0 when the run reaches bit 0 -
// then it may have begun in an earlier word (cc_enters)
SF_HD int cc_run_start(cc_word w, int bit)
{
    const cc_word zeros = ~w & cc_below(bit);
    return zeros ? 64 - cc_clz(zeros) : 0;
}
// bit 0 of w belongs to a run that comes in from the word before (whose bit 63 is `prev_top`)
SF_HD bool cc_enters(cc_word w, bool prev_top) { return (w & 1ull) && prev_top; }
// where the run that leaves a word at bit 63 begins inside it: 0..63, or 64 when bit 63 is clear (nothing leaves).  0 for a full word:
// the run came in (or begins at bit 0)
SF_HD int cc_tail_start(cc_word w)
{
    const cc_word zeros = ~w;
    return zeros ? 64 - cc_clz(zeros) : 0;
}
// The carry across words, as a wave takes it: among the words 0 .. lane - 1 of a turn (lane <= 64), `nonfull` has bit j set where word j
// is not all ones.  The last such word before `lane`, or -1: every word before is full and the run comes from the turn's carry-in.
SF_HD int cc_carry_word(cc_word nonfull, int lane)
{
    const cc_word m = nonfull & cc_below(lane);
    return m ? 63 - cc_clz(m) : -1;
}
// The column at which the run entering word `lane` of a turn at bit 0 begins.  j = cc_carry_word, wj = word j (any value for j < 0),
// col0 = the column of the turn's word 0, carry_in = the column at which the run entering the turn's word 0 begins (col0 if none does)
SF_HD int cc_carry_col(int j, cc_word wj, int col0, int carry_in) { return j < 0 ? carry_in : col0 + 64 * j + cc_tail_start(wj); }
// the parent a cell starts with: the first cell of its horizontal run.  x = 64 * wi + bit, set in w; carry = cc_carry_col of word wi
SF_HD int cc_first_col(cc_word w, int wi, int bit, bool prev_top, int carry)
{
    const int s = cc_run_start(w, bit);
    return (s == 0 && cc_enters(w, prev_top)) ? carry : 64 * wi + s;
}

// ---- phase 2: where a contact begins.  cur: a word of row y; up: the same word of row y - 1; cur_l / up_l: bit 63 of the words to
// their left (0 at wi == 0), up_r: bit 0 of the word to the right of up (0 past the row).  A contact is a pair (x, u) of a selected
// cell x of row y and a selected cell u of row y - 1 with u = x (4) or u in {x - 1, x, x + 1} (8).  A contact is SKIPPED when an
// earlier one, in the order of (x, u), joins the same two runs: (x, u - 1) if u - 1 is selected and a neighbour of x; (x - 1, u) if
// x - 1 is selected and u its neighbour.  Every skip names a strictly earlier contact of the same pair of runs, so the first contact
// of every pair is kept, and that is all the merge needs.
struct CcContacts {
    cc_word up_left, up, up_right;      // bit x: cell x of the word unites with its neighbour above at x - 1 / x / x + 1
};
SF_HD CcContacts cc_contacts(int conn8, cc_word cur, cc_word up, bool cur_l, bool up_l, bool up_r)
{
    const cc_word cl = (cur << 1) | (cc_word)cur_l, ul = (up << 1) | (cc_word)up_l, ur = (up >> 1) | ((cc_word)up_r << 63);
    CcContacts c;
    if (conn8) {
        c.up_left = cur & ul & ~cl;
        c.up = cur & up & ~ul & ~cl;
        c.up_right = cur & ur & ~up;
    } else {
        c.up_left = 0; c.up_right = 0;
        c.up = cur & up & ~(cl & ul);
    }
    return c;
}

// The union of two cells over a label plane, lock-free: find both roots, write the smaller index into the larger root with an atomic
// minimum, go on with what stood there until both ends meet.  Parents only ever decrease, so it ends, and the root of a component is
// its smallest index in whatever order the unions come.  P gives the plane's accesses: load(i), fetch_min(i, v) -> the old value.  A
// stale parent is still an ancestor (parents are only ever replaced by smaller members of the same component), which is all find needs.
template <class P> SF_HD int cc_find(P &p, int x)
{
    for (;;) {
        const int q = p.load(x);
        if (q == x) return x;
        x = q;
    }
}
// find with path halving: a cell on the way takes its grandparent where that is smaller - an atomic minimum too, for a grandparent is an
// ancestor and parents only decrease.  It keeps the walks of later unions short.
template <class P> SF_HD int cc_find_halve(P &p, int x)
{
    for (;;) {
        const int q = p.load(x);
        if (q == x) return x;
        const int gp = p.load(q);
        if (gp < q) p.fetch_min(x, gp);
        x = q;
    }
}
template <class P> SF_HD void cc_unite(P &p, int a, int b)
{
    for (;;) {
        a = cc_find(p, a);
        b = cc_find(p, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }       // a: the larger root
        const int old = p.fetch_min(a, b);
        if (old == a) return;                               // a was still a root: linked
        a = old;                                            // someone linked a first: what it pointed at joins b's side too
    }
}

// ---- phase 4: the rank scan.  counts[0 .. H) (roots per row) become exclusive sums and counts[H] the total, shared by kCompScanThreads
// workers: worker t owns rows [cc_seg_lo(H, t), cc_seg_lo(H, t + 1)); it sums them, the sums are scanned, it writes its rows.
SF_HD int cc_seg_lo(int H, int t)
{
    const int per = (H + kCompScanThreads - 1) / kCompScanThreads;
    const long long lo = (long long)per * t;
    return lo < H ? (int)lo : H;
}
SF_HD int cc_seg_sum(const int32_t *counts, int lo, int hi)
{
    int s = 0;
    for (int y = lo; y < hi; ++y) s += counts[y];
    return s;
}
SF_HD void cc_seg_write(int32_t *counts, int lo, int hi, int base)
{
    for (int y = lo; y < hi; ++y) { const int c = counts[y]; counts[y] = base; base += c; }
}

// ---- phase 5: runs of a word, one after another: the lowest run of `rest` as a mask; the caller clears it from rest
SF_HD cc_word cc_next_run(cc_word rest)
{
    const cc_word low = rest & (~rest + 1ull);        // the run's first bit
    const cc_word sum = rest + low;                   // the carry clears the run and sets the bit behind it
    return rest & ~sum;
}
// Touch.  For one status s: `m` = the unselected cells of that status in the word (wi) of row r, l / r_ = the same for the cell left of
// bit 0 / right of bit 63.  What the selected cells of the word in row y see of it: row y itself gives its two side neighbours, a row
// above or below the cell over it and - with diagonals - its two sides
SF_HD cc_word cc_touch_from(cc_word m, bool l, bool r_, bool same_row, int conn8)
{
    const cc_word sides = (m << 1) | (cc_word)l | (m >> 1) | ((cc_word)r_ << 63);
    return same_row ? sides : (conn8 ? (m | sides) : m);
}
// the touch word of a run: seen[s] = the cells of the word that have an unselected neighbour of status s; border = the cells of the
// word on the grid's border
SF_HD int cc_touch_run(const cc_word (&seen)[6], cc_word border, cc_word run)
{
    int t = 0;
    for (int s = 0; s < 6; ++s) t |= (seen[s] & run) ? 1 << s : 0;
    return t | ((border & run) ? 64 : 0);
}
// the cells of word wi of row y that lie on the border of an H x W grid
SF_HD cc_word cc_border(int H, int W, int y, int wi)
{
    const cc_word on = cc_on_grid(W - 64 * wi);
    if (y == 0 || y == H - 1) return on;
    cc_word b = 0;
    if (wi == 0) b |= 1ull;
    if ((W - 1) / 64 == wi) b |= 1ull << ((W - 1) & 63);
    return b & on;
}
// the largest component as one key an integer maximum orders: more cells first, then the LOWER number; 0: no component
SF_HD cc_word cc_largest_key(int number, int cells) { return ((cc_word)(uint32_t)cells << 32) | (cc_word)(0xFFFFFFFFu - (uint32_t)number); }
SF_HD int cc_key_number(cc_word key) { return key ? (int)(0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull)) : 0; }
SF_HD int cc_key_cells(cc_word key) { return (int)(key >> 32); }

}  // namespace
