// The band scheme of simfire_amd/csrc/sf_bands.h, checked on its own (tests/test_bands_cpu.py builds this with the address and
// undefined-behaviour sanitizers and runs it).  A workgroup is emulated on the host as the kernels run it: per round every band reads
// its halo (band_halo), then every band runs its round or level, then every band publishes; the planes are laid out with band_at.
// The yardsticks are stated here, not taken from the code under test: a flood fill and a breadth-first search over a byte grid.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../simfire_amd/csrc/sf_bands.h"

namespace {

int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++failures <= 20) { std::printf("%s:%d: %s: ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

// ---- a map: open and seed bytes of an H x W grid (a seed is never open)
struct Map {
    int H, W;
    std::vector<uint8_t> open, seed;
    const char *name;
};
uint32_t rng_state = 12345u;
uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }      // fixed seed: the same maps every run

Map make_map(int H, int W, const char *name)
{
    Map m{H, W, std::vector<uint8_t>((size_t)H * W, 0), std::vector<uint8_t>((size_t)H * W, 0), name};
    return m;
}
Map random_map(int H, int W, double density)
{
    Map m = make_map(H, W, "random");
    for (size_t i = 0; i < m.open.size(); ++i) {
        m.open[i] = rng() % 1000 < (uint32_t)(density * 1000);
        if (rng() % 100 < 2) { m.seed[i] = 1; m.open[i] = 0; }
    }
    return m;
}
Map corner_map(int H, int W)
{
    Map m = make_map(H, W, "all open, corner seed");
    for (auto &o : m.open) o = 1;
    m.seed[0] = 1; m.open[0] = 0;
    return m;
}
// a corridor along the even rows, joined at alternating ends by one cell of the odd rows: it crosses every word and band border
Map serpentine_map(int H, int W)
{
    Map m = make_map(H, W, "serpentine");
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            m.open[(size_t)y * W + x] = y % 2 == 0 || x == ((y / 2) % 2 == 0 ? W - 1 : 0);
    m.seed[0] = 1; m.open[0] = 0;
    return m;
}

const int kDx8[8] = {0, 0, -1, 1, -1, 1, -1, 1}, kDy8[8] = {-1, 1, 0, 0, -1, -1, 1, 1};

// the yardstick of both searches: BFS distance from the seeds through open cells (-1: not reached; seeds 0)
std::vector<int> naive_bfs(const Map &m, int conn8)
{
    std::vector<int> d((size_t)m.H * m.W, -1);
    std::vector<int> front, next;
    for (int i = 0; i < m.H * m.W; ++i) if (m.seed[i]) { d[i] = 0; front.push_back(i); }
    for (int level = 1; !front.empty(); ++level) {
        next.clear();
        for (int i : front) {
            const int y = i / m.W, x = i % m.W;
            for (int n = 0; n < (conn8 ? 8 : 4); ++n) {
                const int ny = y + kDy8[n], nx = x + kDx8[n];
                if (ny < 0 || ny >= m.H || nx < 0 || nx >= m.W) continue;
                const int j = ny * m.W + nx;
                if (m.open[j] && d[j] < 0) { d[j] = level; next.push_back(j); }
            }
        }
        front.swap(next);
    }
    return d;
}

// ---- the emulated workgroup
struct Bands {
    int H, W, WORDS, BR, nb;
    std::vector<band_word> top, bot;
    std::vector<uint32_t> edge;
    Bands(int H_, int W_) : H(H_), W(W_), WORDS(band_words(W_)), BR(band_rows(H_)), nb(BR * WORDS), top(nb), bot(nb), edge(nb) {}
    std::vector<band_word> plane(const std::vector<uint8_t> &bytes) const      // a band-major bit plane of a byte grid
    {
        std::vector<band_word> p((size_t)nb * kBandRows, 0);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x)
                if (bytes[(size_t)y * W + x]) p[(size_t)band_at(WORDS, y, x >> 6)] |= 1ull << (x & 63);
        return p;
    }
    bool bit(const std::vector<band_word> &p, int y, int x) const { return (p[(size_t)band_at(WORDS, y, x >> 6)] >> (x & 63)) & 1u; }
    // bits off the grid: rows past H, columns past W
    bool clean(const std::vector<band_word> &p) const
    {
        for (int y = 0; y < BR * kBandRows; ++y)
            for (int wi = 0; wi < WORDS; ++wi) {
                const band_word w = p[(size_t)band_at(WORDS, y, wi)];
                const int in = W - wi * 64;
                if (y >= H ? w != 0 : (in < 64 && (w >> in) != 0)) return false;
            }
        return true;
    }
    void publish_all(const std::vector<band_word> &f)
    {
        for (int b = 0; b < nb; ++b) {
            band_word r[kBandRows];
            band_load(r, f.data(), b);
            band_publish(top.data(), bot.data(), edge.data(), b, r);
        }
    }
    std::vector<BandHalo> halos() const
    {
        std::vector<BandHalo> h((size_t)nb);
        for (int b = 0; b < nb; ++b) h[b] = band_halo(WORDS, BR, top.data(), bot.data(), edge.data(), b / WORDS, b % WORDS);
        return h;
    }
};

void check_geometry(int H, int W)
{
    const int WORDS = band_words(W), BR = band_rows(H);
    CHECK(WORDS == (W + 63) / 64 && BR == (H + 15) / 16, "%d x %d: %d words, %d band rows", H, W, WORDS, BR);
    const long long nb = (long long)WORDS * BR;
    CHECK(band_env_bytes(nb, 2, 1) == (nb * (16 * 16 + 20) + 255) / 256 * 256, "reach scratch of %lld bands", nb);
    CHECK(band_env_bytes(nb, 3, 2) == (nb * (16 * 24 + 40) + 255) / 256 * 256, "walk scratch of %lld bands", nb);
    std::vector<int> seen((size_t)nb * 16, 0);
    for (int y = 0; y < BR * 16; ++y)
        for (int wi = 0; wi < WORDS; ++wi) {
            const long long at = band_at(WORDS, y, wi);      // the definition: band (y / 16, wi), row y % 16 inside it, bands row-major
            CHECK(at == ((long long)(y / 16) * WORDS + wi) * 16 + y % 16, "band_at(%d, %d, %d) = %lld", WORDS, y, wi, at);
            if (at >= 0 && at < nb * 16) seen[(size_t)at]++;
        }
    for (int s : seen) CHECK(s == 1, "%d x %d: band_at is no bijection", H, W);
}

void check_reach(const Map &m, int conn8)
{
    Bands B(m.H, m.W);
    const std::vector<int> dist = naive_bfs(m, conn8);
    std::vector<uint8_t> truth_bytes(dist.size());
    long long n_open = 0;
    for (size_t i = 0; i < dist.size(); ++i) { truth_bytes[i] = dist[i] >= 0; n_open += m.open[i]; }
    const std::vector<band_word> truth = B.plane(truth_bytes), open = B.plane(m.open);
    std::vector<band_word> f = B.plane(m.seed);
    B.publish_all(f);
    long long rounds = 0;
    for (;;) {
        ++rounds;
        const std::vector<BandHalo> h = B.halos();
        bool changed = false;
        std::vector<uint8_t> band_changed((size_t)B.nb, 0);
        for (int b = 0; b < B.nb; ++b) {
            band_word r[kBandRows];
            band_load(r, f.data(), b);
            band_changed[b] = band_round(r, open.data() + (size_t)b * kBandRows, h[b], conn8);
            band_store(f.data(), b, r);
            changed |= band_changed[b] != 0;
        }
        for (int b = 0; b < B.nb; ++b)
            if (band_changed[b]) { band_word r[kBandRows]; band_load(r, f.data(), b); band_publish(B.top.data(), B.bot.data(), B.edge.data(), b, r); }
        bool subset = true;
        for (size_t i = 0; i < f.size(); ++i) subset &= (f[i] & ~truth[i]) == 0;
        CHECK(subset, "%s %d x %d conn8 %d: round %lld left the truth", m.name, m.H, m.W, conn8, rounds);
        CHECK(B.clean(f), "%s %d x %d conn8 %d: round %lld set a bit off the grid", m.name, m.H, m.W, conn8, rounds);
        if (!changed) break;
        if (rounds > n_open + 1) break;
    }
    CHECK(rounds <= n_open + 1, "%s %d x %d conn8 %d: %lld rounds for %lld open cells", m.name, m.H, m.W, conn8, rounds, n_open);
    CHECK(f == truth, "%s %d x %d conn8 %d: the fixed point is not the flood fill", m.name, m.H, m.W, conn8);
}

void check_walk(const Map &m, int conn8)
{
    Bands B(m.H, m.W);
    const std::vector<int> dist = naive_bfs(m, conn8);
    int deepest = 0;
    for (int d : dist) deepest = d > deepest ? d : deepest;
    std::vector<band_word> f = B.plane(m.seed), u = B.plane(m.open);      // the front (at the start the targets), U
    B.publish_all(f);
    int L = 0;
    for (;;) {
        const std::vector<BandHalo> h = B.halos();
        bool added = false;
        for (int b = 0; b < B.nb; ++b) {
            band_word r[kBandRows];
            band_load(r, f.data(), b);
            added |= band_level(r, u.data() + (size_t)b * kBandRows, h[b], conn8);
            band_store(f.data(), b, r);
        }
        B.publish_all(f);
        CHECK(B.clean(f) && B.clean(u), "%s %d x %d conn8 %d: level %d set a bit off the grid", m.name, m.H, m.W, conn8, L + 1);
        bool exact = true;
        for (int y = 0; y < m.H; ++y)
            for (int x = 0; x < m.W; ++x) exact &= B.bit(f, y, x) == (dist[(size_t)y * m.W + x] == L + 1);
        CHECK(exact, "%s %d x %d conn8 %d: the cells added at level %d are not the cells at distance %d", m.name, m.H, m.W, conn8, L + 1, L + 1);
        if (!added) break;
        ++L;
        if (L > m.H * m.W) break;
    }
    CHECK(L == deepest, "%s %d x %d conn8 %d: the search stopped behind level %d, the farthest cell is %d moves away", m.name, m.H, m.W, conn8, L, deepest);
    for (int y = 0; y < m.H; ++y)      // what is left of U is what no walk reaches
        for (int x = 0; x < m.W; ++x) {
            const size_t i = (size_t)y * m.W + x;
            CHECK(B.bit(u, y, x) == (m.open[i] && dist[i] < 0), "%s %d x %d conn8 %d: U at (%d, %d)", m.name, m.H, m.W, conn8, y, x);
        }
}

// ---- edge cases, as literals
void check_literals()
{
    const band_word ALL = ~0ull, TOP = 1ull << 63;
    CHECK(band_brev(1ull) == TOP && band_brev(0x00000000000000F0ull) == 0x0F00000000000000ull && band_brev(ALL) == ALL, "band_brev");
    CHECK(bits_bytes4(0x0u) == 0u && bits_bytes4(0xFu) == 0x01010101u && bits_bytes4(0x5u) == 0x00010001u && bits_bytes4(0x1Au) == 0x01000100u, "bits_bytes4");
    uint32_t d[4];
    bits_bytes16(0x8421u, d);
    CHECK(d[0] == 0x00000001u && d[1] == 0x00000100u && d[2] == 0x00010000u && d[3] == 0x01000000u, "bits_bytes16");
    // band_fill(w, o, cl, cr): runs of o that hold or touch a bit of w, or that a carry enters at bit 0 (cl) or bit 63 (cr)
    CHECK(band_fill(0, ALL, 0, 0) == 0, "nothing to fill from");
    CHECK(band_fill(0, ALL, 1, 0) == ALL && band_fill(0, ALL, 0, 1) == ALL, "a carry fills an all-open word");
    CHECK(band_fill(1ull << 20, ALL, 0, 0) == ALL, "one bit fills an all-open word");
    CHECK(band_fill(0, 0x0Full, 1, 0) == 0x0Full && band_fill(0, 0x0Full, 0, 1) == 0, "cl enters the run at bit 0 only");
    CHECK(band_fill(0, 0xF0ull << 56, 0, 1) == 0xF0ull << 56 && band_fill(0, 0xF0ull << 56, 1, 0) == 0, "cr enters the run at bit 63 only");
    CHECK(band_fill(0, 0x0Eull, 1, 0) == 0 && band_fill(0, 0x70ull << 56, 0, 1) == 0, "a run that does not touch the border takes no carry");
    CHECK(band_fill(1ull << 4, 0x0Full | 0xE0ull, 0, 0) == ((1ull << 4) | 0x0Full | 0xE0ull), "a closed bit of w fills the runs on both sides");
    CHECK(band_fill(1ull << 8, 0x0Full | 0xF000ull, 0, 0) == (1ull << 8), "a bit two cells from a run does not reach it");
    CHECK(band_fill(0x4ull, 0x0Full | 0xF0ull << 56, 0, 0) == (0x0Full), "only the run that holds the bit is filled");
    CHECK(band_fill(TOP, ALL & ~(1ull << 32), 0, 0) == (ALL << 33), "downwards from bit 63 to the gap");
    CHECK(band_fill(1ull, ALL & ~(1ull << 32), 0, 0) == ((1ull << 32) - 1), "upwards from bit 0 to the gap");
    // band_spread
    CHECK(band_spread(0x10ull, 0, 0, 0) == 0x10ull && band_spread(0x10ull, 0, 0, 1) == 0x38ull, "band_spread inside a word");
    CHECK(band_spread(0, 1, 0, 1) == 1ull && band_spread(0, 0, 1, 1) == TOP && band_spread(0, 1, 1, 0) == 0, "band_spread across the word borders");
    // band_edges: bit 0 of row j at bit j, bit 63 of row j at bit 16 + j
    band_word f[kBandRows] = {};
    f[0] = 1ull; f[3] = TOP; f[15] = TOP | 1ull;
    CHECK(band_edges(f) == (1u | 1u << 15 | 1u << (16 + 3) | 1u << (16 + 15)), "band_edges %08x", band_edges(f));
    // band_halo on a 3 x 3 field of bands: el bit j + 1 = bit 63 of row j of the band to the left, bit 0 / 17 the corners
    const int WORDS = 3, BR = 3, nb = 9;
    std::vector<band_word> top(nb, 0), bot(nb, 0);
    std::vector<uint32_t> edge(nb, 0);
    std::vector<band_word> pl((size_t)nb * kBandRows, 0);
    const auto set = [&](int y, int x) { pl[(size_t)band_at(WORDS, y, x >> 6)] |= 1ull << (x & 63); };
    set(15, 63); set(15, 70); set(15, 128);      // the row above the centre band: left corner, inside, right corner
    set(32, 63); set(32, 127); set(32, 128);     // the row below it
    set(16, 63); set(20, 63); set(31, 63);       // the column to its left: rows 0, 4, 15
    set(17, 128); set(31, 128);                  // the column to its right: rows 1, 15
    set(16, 0); set(16, 62);                     // (bits that no neighbour of the centre sees)
    for (int b = 0; b < nb; ++b) { band_word r[kBandRows]; band_load(r, pl.data(), b); band_publish(top.data(), bot.data(), edge.data(), b, r); }
    const BandHalo h = band_halo(WORDS, BR, top.data(), bot.data(), edge.data(), 1, 1);
    CHECK(h.top == (1ull << 6) && h.bot == TOP, "halo rows %016llx %016llx", h.top, h.bot);
    CHECK(h.el == (1u | 1u << 1 | 1u << 5 | 1u << 16 | 1u << 17), "halo el %08x", h.el);
    CHECK(h.er == (1u | 1u << 2 | 1u << 16 | 1u << 17), "halo er %08x", h.er);
    const BandHalo c = band_halo(WORDS, BR, top.data(), bot.data(), edge.data(), 0, 0);      // a corner band: nothing past the grid
    CHECK(c.top == 0 && c.el == 0 && c.bot == pl[(size_t)band_at(WORDS, 16, 0)] && c.er == 0, "halo of the corner band");
}

}  // namespace

int main()
{
    check_literals();
    const int Hs[] = {1, 15, 16, 17, 33}, Ws[] = {1, 63, 64, 65, 130};
    const double densities[] = {0.3, 0.6, 0.9};
    for (int H : Hs)
        for (int W : Ws) {
            check_geometry(H, W);
            std::vector<Map> maps;
            for (double dns : densities) maps.push_back(random_map(H, W, dns));
            maps.push_back(make_map(H, W, "empty"));
            maps.push_back(corner_map(H, W));
            maps.push_back(serpentine_map(H, W));
            for (const Map &m : maps)
                for (int conn8 = 0; conn8 < 2; ++conn8) {
                    check_reach(m, conn8);
                    check_walk(m, conn8);
                }
        }
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
