// The arithmetic of sf_components (simfire_amd/csrc/sf_components.h) on the host: the five phases of DESIGN.md section 31 emulated with
// the header's own functions - the runs of a word and the carry across words as a wave of 64 lanes takes it, the contacts that begin,
// the unions one after another in several shuffled orders, the flattening, the rank scan shared by 256 workers, the runs and the touch
// word of the stats pass - and compared with a fill this file states itself over a byte grid.  Shapes: those of the scenes (9 x 9,
// 33 x 17, 40 x 130, 64 x 64, 70 x 1030) and a row of more than 64 words (3 x 4200); both connectivities; random maps of three densities,
// the empty and the full grid, a checkerboard, a comb.  Built by tests/test_components_cpu.py with the address and undefined-behaviour
// sanitizers and run as a program of its own.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <queue>
#include <random>
#include <vector>

#include "../simfire_amd/csrc/sf_components.h"

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { if (g_fail++ < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

struct Grid {
    int H, W;
    std::vector<uint8_t> status, sel;      // status 0..5; sel 0 / 1
    bool on(int y, int x) const { return y >= 0 && y < H && x >= 0 && x < W; }
};

// ---- the yardstick: a fill in row-major order of first cells
struct Want {
    int C = 0;
    std::vector<int> lab, cells, touch, box;
};
static Want fill(const Grid &g, int conn8)
{
    Want w;
    w.lab.assign((size_t)g.H * g.W, 0);
    for (int s = 0; s < g.H * g.W; ++s) {
        if (!g.sel[s] || w.lab[s]) continue;
        const int c = ++w.C;
        w.cells.push_back(0); w.touch.push_back(0);
        w.box.insert(w.box.end(), {g.W, g.H, -1, -1});
        std::queue<int> q;
        q.push(s); w.lab[s] = c;
        while (!q.empty()) {
            const int at = q.front(), y = at / g.W, x = at % g.W;
            q.pop();
            w.cells[c - 1]++;
            int *b = &w.box[4 * (c - 1)];
            b[0] = std::min(b[0], x); b[1] = std::min(b[1], y); b[2] = std::max(b[2], x); b[3] = std::max(b[3], y);
            if (y == 0 || x == 0 || y == g.H - 1 || x == g.W - 1) w.touch[c - 1] |= 64;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    if ((!dy && !dx) || (!conn8 && dy && dx) || !g.on(y + dy, x + dx)) continue;
                    const int nb = (y + dy) * g.W + x + dx;
                    if (!g.sel[nb]) w.touch[c - 1] |= 1 << g.status[nb];
                    else if (!w.lab[nb]) { w.lab[nb] = c; q.push(nb); }
                }
        }
    }
    return w;
}

// ---- the emulation
struct HostPlane {
    std::vector<int32_t> &p;
    int load(int i) const { return p[i]; }
    int fetch_min(int i, int v) const { const int old = p[i]; p[i] = std::min(old, v); return old; }
};
static cc_word word_of(const Grid &g, const std::vector<uint8_t> &bytes, int y, int wi, int equals)      // bit x: bytes[y][64 wi + x] == equals
{
    cc_word w = 0;
    for (int b = 0; b < 64; ++b) {
        const int x = 64 * wi + b;
        if (x < g.W && bytes[(size_t)y * g.W + x] == equals) w |= 1ull << b;
    }
    return w;
}

static void emulate(const Grid &g, int conn8, unsigned seed, const Want &want, const char *tag)
{
    const int H = g.H, W = g.W, WORDS = cc_words(W);
    std::vector<cc_word> bits((size_t)H * WORDS);
    for (int y = 0; y < H; ++y)
        for (int wi = 0; wi < WORDS; ++wi) bits[(size_t)y * WORDS + wi] = word_of(g, g.sel, y, wi, 1);
    // phase 1: a wave per row, turns of 64 words
    std::vector<int32_t> lab((size_t)H * W, -1);
    for (int y = 0; y < H; ++y) {
        int carry_in = 0;
        bool top_in = false;
        for (int w0 = 0; w0 < WORDS; w0 += 64) {
            cc_word w[64], nonfull = 0;
            for (int lane = 0; lane < 64; ++lane) {
                w[lane] = w0 + lane < WORDS ? bits[(size_t)y * WORDS + w0 + lane] : 0;
                if (w[lane] != ~0ull) nonfull |= 1ull << lane;
            }
            if (!top_in) carry_in = 64 * w0;
            for (int k = 0; k < std::min(64, WORDS - w0); ++k) {
                const int j = cc_carry_word(nonfull, k);
                const int carry = cc_carry_col(j, w[j < 0 ? 0 : j], 64 * w0, carry_in);
                const bool prev_top = k ? (w[k - 1] >> 63) != 0 : top_in;
                for (int lane = 0; lane < 64; ++lane) {
                    const int x = 64 * (w0 + k) + lane;
                    if (x < W && ((w[k] >> lane) & 1ull)) lab[(size_t)y * W + x] = y * W + cc_first_col(w[k], w0 + k, lane, prev_top, carry);
                }
            }
            const int j2 = cc_carry_word(nonfull, 64);
            carry_in = cc_carry_col(j2, w[j2 < 0 ? 0 : j2], 64 * w0, carry_in);
            top_in = (w[63] >> 63) != 0;
        }
    }
    for (int c = 0; c < H * W; ++c) {       // a cell's first parent is the first cell of its run
        if (!g.sel[c]) { CHECK(lab[c] == -1, "%s: unselected cell %d has parent %d", tag, c, lab[c]); continue; }
        int s = c;
        while (s % W && g.sel[s - 1]) --s;
        CHECK(lab[c] == s, "%s: cell %d starts with parent %d, its run begins at %d", tag, c, lab[c], s);
    }
    // phase 2: the contacts that begin, united one after another in a shuffled order
    std::vector<std::pair<int, int>> unions;
    for (int y = 1; y < H; ++y)
        for (int wi = 0; wi < WORDS; ++wi) {
            const cc_word *row = &bits[(size_t)y * WORDS], *above = row - WORDS;
            const CcContacts c = cc_contacts(conn8, row[wi], above[wi], wi > 0 && (row[wi - 1] >> 63), wi > 0 && (above[wi - 1] >> 63),
                                             wi + 1 < WORDS && (above[wi + 1] & 1ull));
            for (int d = -1; d <= 1; ++d) {
                cc_word m = d < 0 ? c.up_left : (d == 0 ? c.up : c.up_right);
                for (; m; m &= m - 1) {
                    const int x = y * W + 64 * wi + cc_ctz(m);
                    CHECK(g.sel[x] && g.sel[x - W + d] && (64 * wi + cc_ctz(m) + d >= 0) && (64 * wi + cc_ctz(m) + d < W), "%s: a contact off the selection at %d", tag, x);
                    unions.push_back({x, x - W + d});
                }
            }
        }
    std::mt19937 rng(seed);
    std::shuffle(unions.begin(), unions.end(), rng);
    HostPlane plane{lab};
    for (const auto &u : unions) cc_unite(plane, cc_find_halve(plane, u.first), cc_find_halve(plane, u.second));      // (as k_comp_merge calls it)
    // phase 3: run heads take their root, the other cells their head's
    for (int c = 0; c < H * W; ++c)
        if (g.sel[c] && (c % W == 0 || !g.sel[c - 1])) lab[c] = cc_find(plane, c);
    for (int c = 0; c < H * W; ++c)
        if (g.sel[c] && lab[c] != c) lab[c] = lab[lab[c]];
    // phase 4: roots per row, the scan shared by the workers, ranks
    std::vector<int32_t> rows(H + 1, 0), aux((size_t)H * W, 0);
    for (int c = 0; c < H * W; ++c) rows[c / W] += lab[c] == c;
    int part[kCompScanThreads], total = 0;
    for (int t = 0; t < kCompScanThreads; ++t) part[t] = cc_seg_sum(rows.data(), cc_seg_lo(H, t), cc_seg_lo(H, t + 1));
    for (int t = 0; t < kCompScanThreads; ++t) { const int c = part[t]; part[t] = total; total += c; }
    for (int t = 0; t < kCompScanThreads; ++t) cc_seg_write(rows.data(), cc_seg_lo(H, t), cc_seg_lo(H, t + 1), part[t]);
    CHECK(total == want.C, "%s: %d components, the fill has %d", tag, total, want.C);
    for (int y = 0; y < H; ++y) {
        int base = rows[y];
        for (int x = 0; x < W; ++x)
            if (lab[(size_t)y * W + x] == y * W + x) aux[(size_t)y * W + x] = base++;
    }
    // phase 5: relabel, then the stats of every run of every word
    for (int c = 0; c < H * W; ++c) lab[c] = lab[c] < 0 ? 0 : aux[lab[c]] + 1;
    for (int c = 0; c < H * W; ++c) CHECK(lab[c] == want.lab[c], "%s: cell %d has label %d, the fill says %d", tag, c, lab[c], want.lab[c]);
    if (total != want.C) return;
    std::vector<int> cells(total, 0), touch(total, 0), box;
    for (int c = 0; c < total; ++c) box.insert(box.end(), {W, H, -1, -1});
    for (int y = 0; y < H; ++y)
        for (int wi = 0; wi < WORDS; ++wi) {
            const cc_word w = bits[(size_t)y * WORDS + wi];
            cc_word seen[6] = {0, 0, 0, 0, 0, 0};
            for (int dr = -1; dr <= 1; ++dr) {
                const int r = y + dr;
                if (r < 0 || r >= H) continue;
                for (int s = 0; s < 6; ++s) {
                    const cc_word m = word_of(g, g.status, r, wi, s) & ~bits[(size_t)r * WORDS + wi];
                    const int xl = 64 * wi - 1, xr = 64 * wi + 64;
                    const bool l = xl >= 0 && !g.sel[(size_t)r * W + xl] && g.status[(size_t)r * W + xl] == s;
                    const bool rr = xr < W && !g.sel[(size_t)r * W + xr] && g.status[(size_t)r * W + xr] == s;
                    seen[s] |= cc_touch_from(m, l, rr, dr == 0, conn8);
                }
            }
            for (int s = 0; s < 6; ++s) seen[s] &= w;
            const cc_word border = cc_border(H, W, y, wi);
            cc_word covered = 0;
            for (cc_word rest = w; rest;) {
                const cc_word run = cc_next_run(rest);
                rest &= ~run;
                CHECK(run && !(run & covered), "%s: runs overlap in word %d of row %d", tag, wi, y);
                covered |= run;
                const int x0 = 64 * wi + cc_ctz(run), len = cc_popc(run), L = lab[(size_t)y * W + x0];
                for (int x = x0; x < x0 + len; ++x) CHECK(lab[(size_t)y * W + x] == L, "%s: a run with two labels at row %d column %d", tag, y, x);
                cells[L - 1] += len;
                touch[L - 1] |= cc_touch_run(seen, border, run);
                int *b = &box[4 * (L - 1)];
                b[0] = std::min(b[0], x0); b[1] = std::min(b[1], y); b[2] = std::max(b[2], x0 + len - 1); b[3] = std::max(b[3], y);
            }
            CHECK(covered == w, "%s: the runs do not cover word %d of row %d", tag, wi, y);
        }
    cc_word key = 0, want_key = 0;
    for (int c = 0; c < total; ++c) {
        CHECK(cells[c] == want.cells[c], "%s: component %d has %d cells, the fill says %d", tag, c + 1, cells[c], want.cells[c]);
        CHECK(touch[c] == want.touch[c], "%s: component %d touches %d, the fill says %d", tag, c + 1, touch[c], want.touch[c]);
        for (int k = 0; k < 4; ++k) CHECK(box[4 * c + k] == want.box[4 * c + k], "%s: component %d box[%d]", tag, c + 1, k);
        key = std::max(key, cc_largest_key(c + 1, cells[c]));
        if (want.cells[c] > cc_key_cells(want_key)) want_key = cc_largest_key(c + 1, want.cells[c]);      // (the first of equal sizes)
    }
    CHECK(key == want_key && (total == 0 || (cc_key_number(key) >= 1 && cells[cc_key_number(key) - 1] == cc_key_cells(key))), "%s: the largest component", tag);
}

static void run(const Grid &g, const char *name)
{
    char tag[128];
    for (int conn8 = 0; conn8 <= 1; ++conn8) {
        const Want want = fill(g, conn8);
        for (unsigned seed = 1; seed <= 3; ++seed) {
            std::snprintf(tag, sizeof tag, "%s %dx%d conn %d order %u", name, g.H, g.W, conn8 ? 8 : 4, seed);
            emulate(g, conn8, seed, want, tag);
        }
    }
}

int main()
{
    // literals
    CHECK(cc_run_start(0xF0ull, 6) == 4 && cc_run_start(0xFFull, 6) == 0 && cc_run_start(~0ull, 63) == 0 && cc_run_start(1ull << 63, 63) == 63, "cc_run_start");
    CHECK(cc_tail_start(~0ull) == 0 && cc_tail_start(0ull) == 64 && cc_tail_start(3ull << 62) == 62 && cc_tail_start(1ull) == 64, "cc_tail_start");
    CHECK(cc_carry_word(0ull, 5) == -1 && cc_carry_word(0x5ull, 2) == 0 && cc_carry_word(0x5ull, 3) == 2 && cc_carry_word(~0ull, 64) == 63, "cc_carry_word");
    CHECK(cc_next_run(0x6ull) == 0x6ull && cc_next_run(0xDull) == 0x1ull && cc_next_run(1ull << 63) == 1ull << 63 && cc_next_run(0xC000000000000001ull) == 1ull, "cc_next_run");
    CHECK(cc_border(5, 70, 2, 0) == 1ull && cc_border(5, 70, 2, 1) == 1ull << 5 && cc_border(5, 70, 0, 1) == 0x3Full && cc_border(5, 64, 1, 0) == (1ull | 1ull << 63), "cc_border");
    CHECK(cc_key_number(cc_largest_key(7, 9)) == 7 && cc_key_cells(cc_largest_key(7, 9)) == 9 && cc_largest_key(2, 9) > cc_largest_key(3, 9) &&
          cc_largest_key(3, 10) > cc_largest_key(2, 9) && cc_key_number(0) == 0, "cc_largest_key");
    CHECK(cc_seg_lo(9, 0) == 0 && cc_seg_lo(9, 9) == 9 && cc_seg_lo(9, 256) == 9 && cc_seg_lo(1030, 256) == 1030 && cc_seg_lo(1030, 1) == 5, "cc_seg_lo");
    {
        const CcContacts c4 = cc_contacts(0, 0xFull, 0x6ull, false, false, false), c8 = cc_contacts(1, 0x9ull, 0x6ull, false, false, false);
        CHECK(c4.up == 0x2ull && !c4.up_left && !c4.up_right, "cc_contacts 4");
        CHECK(c8.up_right == 0x1ull && c8.up_left == 0x8ull && !c8.up, "cc_contacts 8");
    }
    const int shapes[][2] = {{9, 9}, {33, 17}, {40, 130}, {64, 64}, {70, 1030}, {3, 4200}, {1, 1}, {2, 65}};
    std::mt19937 rng(31);
    for (const auto &hw : shapes) {
        Grid g{hw[0], hw[1], {}, {}};
        const size_t n = (size_t)g.H * g.W;
        g.status.assign(n, 0);
        g.sel.assign(n, 0);
        run(g, "empty");
        g.sel.assign(n, 1);
        run(g, "full");
        for (size_t c = 0; c < n; ++c) { g.sel[c] = ((c / g.W) + (c % g.W)) % 2 == 0; g.status[c] = g.sel[c] ? 1 : (uint8_t)(c % 6); }
        run(g, "checkerboard");
        for (size_t c = 0; c < n; ++c) { g.sel[c] = (c % g.W) % 2 == 0 || (int)(c / g.W) == g.H - 1; g.status[c] = g.sel[c] ? 0 : 3; }
        run(g, "comb");
        for (double density : {0.3, 0.5, 0.6}) {
            std::uniform_real_distribution<double> u(0.0, 1.0);
            for (size_t c = 0; c < n; ++c) {
                g.sel[c] = u(rng) < density;
                g.status[c] = (uint8_t)(g.sel[c] ? rng() % 2 : 2 + rng() % 4);          // (unselected cells of a selected status: a member plane took them out)
                if (!g.sel[c] && rng() % 16 == 0) g.status[c] = 0;
            }
            run(g, "random");
        }
    }
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("ok\n");
    return 0;
}
