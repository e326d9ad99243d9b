// band_grow of simfire_amd/csrc/sf_bands.h, checked on its own (tests/test_escape_cpu.py builds this plainly and with the address and
// undefined-behaviour sanitizers and runs it).  A workgroup of the escape search is emulated on the host as
// the kernel runs it: the safe set A is flooded from the targets through the NEVER cells (band_round), then the levels fall from the
// largest deadline - the cells of the level's bucket are set in U, every band reads its halo, every band grows, every band publishes.
// The yardstick is stated here, not taken from the code under test: the recurrence S(c) = min(D(c) - 1, max_n S(n) - 1) iterated
// cell by cell from below until nothing changes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../simfire_amd/csrc/sf_bands.h"

namespace {

int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++failures <= 20) { std::printf("%s:%d: %s: ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

constexpr int kSafe = 2147483647, kLost = -1, kBlocked = -2, kNever = 2147483647;
uint32_t rng_state = 4711u;
uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

struct Map {
    int H, W;
    std::vector<uint8_t> target, walk;       // a target is never walkable here
    std::vector<int> D;                      // deadlines of the walkable cells: 0 .. top, or kNever
    const char *name;
};

Map random_map(int H, int W, double walls, int top, const char *name)
{
    Map m{H, W, std::vector<uint8_t>((size_t)H * W, 0), std::vector<uint8_t>((size_t)H * W, 0), std::vector<int>((size_t)H * W, 0), name};
    for (size_t i = 0; i < m.walk.size(); ++i) {
        m.walk[i] = rng() % 1000 >= (uint32_t)(walls * 1000);
        if (rng() % 100 < 2) { m.target[i] = 1; m.walk[i] = 0; }
        m.D[i] = rng() % 5 == 0 ? kNever : (int)(rng() % (uint32_t)(top + 1));
    }
    return m;
}
// a cell with a small deadline beside cells that joined long before it opens
Map late_map(int H, int W)
{
    Map m = random_map(H, W, 0.0, 40, "late openers");
    for (size_t i = 0; i < m.D.size(); ++i) m.D[i] = i % 7 == 3 ? 2 : 40;
    return m;
}

const int kDx8[8] = {0, 0, -1, 1, -1, 1, -1, 1}, kDy8[8] = {-1, 1, 0, 0, -1, -1, 1, 1};

std::vector<int> naive_slack(const Map &m, int conn8)
{
    std::vector<int> S((size_t)m.H * m.W);
    for (size_t i = 0; i < S.size(); ++i) S[i] = m.target[i] ? kSafe : (m.walk[i] ? kLost : kBlocked);
    for (bool changed = true; changed;) {
        changed = false;
        for (int y = 0; y < m.H; ++y)
            for (int x = 0; x < m.W; ++x) {
                const size_t i = (size_t)y * m.W + x;
                if (!m.walk[i]) continue;
                int best = kLost;
                for (int n = 0; n < (conn8 ? 8 : 4); ++n) {
                    const int ny = y + kDy8[n], nx = x + kDx8[n];
                    if (ny < 0 || ny >= m.H || nx < 0 || nx >= m.W) continue;
                    const int s = S[(size_t)ny * m.W + nx];
                    if (s > best) best = s;
                }
                const int via = best == kSafe ? kSafe : (best >= 0 ? best - 1 : kLost), own = m.D[i] == kNever ? kSafe : m.D[i] - 1;
                int s = via < own ? via : own;
                if (s < kLost) s = kLost;
                if (s > S[i]) { S[i] = s; changed = true; }
            }
    }
    return S;
}

struct Bands {
    int H, W, WORDS, BR, nb;
    std::vector<band_word> top, bot;
    std::vector<uint32_t> edge;
    Bands(int H_, int W_) : H(H_), W(W_), WORDS(band_words(W_)), BR(band_rows(H_)), nb(BR * WORDS), top(nb), bot(nb), edge(nb) {}
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

void check_escape(const Map &m, int conn8)
{
    Bands B(m.H, m.W);
    const std::vector<int> want = naive_slack(m, conn8);
    std::vector<band_word> a((size_t)B.nb * kBandRows, 0), u = a;
    std::vector<int> S((size_t)m.H * m.W);
    int top = 0;
    for (int y = 0; y < m.H; ++y)
        for (int x = 0; x < m.W; ++x) {
            const size_t i = (size_t)y * m.W + x, at = (size_t)band_at(B.WORDS, y, x >> 6);
            S[i] = m.target[i] ? kSafe : (m.walk[i] ? kLost : kBlocked);
            if (m.target[i]) a[at] |= 1ull << (x & 63);
            if (m.walk[i] && m.D[i] == kNever) u[at] |= 1ull << (x & 63);
            if (m.walk[i] && m.D[i] != kNever && m.D[i] > top) top = m.D[i];
        }
    const auto number = [&](int b, int j, band_word n, int val) {        // the cells n of row j of band b get val
        const int y = (b / B.WORDS) * kBandRows + j, x0 = (b % B.WORDS) * 64;
        for (int c = 0; c < 64; ++c)
            if ((n >> c) & 1u) {
                CHECK(y < m.H && x0 + c < m.W, "%s: a cell off the grid joined", m.name);
                if (y < m.H && x0 + c < m.W) {
                    CHECK(S[(size_t)y * m.W + x0 + c] == kLost, "%s: cell (%d, %d) joined twice or is not walkable", m.name, y, x0 + c);
                    S[(size_t)y * m.W + x0 + c] = val;
                }
            }
    };
    // phase 1: the flood through the NEVER cells
    B.publish_all(a);
    for (int rounds = 0;; ++rounds) {
        const std::vector<BandHalo> h = B.halos();
        bool changed = false;
        for (int b = 0; b < B.nb; ++b) {
            band_word r[kBandRows];
            band_load(r, a.data(), b);
            changed |= band_round(r, u.data() + (size_t)b * kBandRows, h[b], conn8);
            band_store(a.data(), b, r);
        }
        B.publish_all(a);
        if (!changed || rounds > m.H * m.W) break;
    }
    for (int b = 0; b < B.nb; ++b)
        for (int j = 0; j < kBandRows; ++j) {
            band_word &uw = u[(size_t)b * kBandRows + j];
            const band_word n = a[(size_t)b * kBandRows + j] & uw;
            uw &= ~n;
            number(b, j, n, kSafe);
        }
    // phase 2: the levels
    for (int v = top - 1; v >= 0; --v) {
        for (int y = 0; y < m.H; ++y)
            for (int x = 0; x < m.W; ++x) {
                const size_t i = (size_t)y * m.W + x;
                if (m.walk[i] && m.D[i] == v + 1) u[(size_t)band_at(B.WORDS, y, x >> 6)] |= 1ull << (x & 63);
            }
        const std::vector<BandHalo> h = B.halos();
        for (int b = 0; b < B.nb; ++b) {
            band_word r[kBandRows];
            band_load(r, a.data(), b);
            band_word gained = 0;
            const bool grew = band_grow(r, u.data() + (size_t)b * kBandRows, h[b], conn8, [&](int j, band_word n) { gained |= n; number(b, j, n, v); });
            CHECK(grew == (gained != 0), "%s: band_grow's return and its calls disagree", m.name);
            for (int j = 0; j < kBandRows; ++j)
                CHECK((r[j] & u[(size_t)b * kBandRows + j]) == 0, "%s: A and U overlap after a level", m.name);
            band_store(a.data(), b, r);
        }
        B.publish_all(a);
    }
    int bad = 0;
    for (size_t i = 0; i < S.size(); ++i) bad += S[i] != want[i];
    CHECK(bad == 0, "%s %d x %d conn8 %d: %d cells differ from the recurrence", m.name, m.H, m.W, conn8, bad);
}

}  // namespace

int main()
{
    const int Hs[] = {1, 15, 16, 17, 33}, Ws[] = {1, 63, 64, 65, 130};
    for (int H : Hs)
        for (int W : Ws) {
            std::vector<Map> maps;
            maps.push_back(random_map(H, W, 0.1, 12, "random, few walls"));
            maps.push_back(random_map(H, W, 0.4, 30, "random, many walls"));
            maps.push_back(random_map(H, W, 0.0, 200, "open field"));
            maps.push_back(late_map(H, W));
            for (const Map &m : maps)
                for (int conn8 = 0; conn8 < 2; ++conn8) check_escape(m, conn8);
        }
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
