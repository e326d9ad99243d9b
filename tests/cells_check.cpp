// The blocked cell plane and the accessors of simfire_amd/csrc/sf_cells.h, checked on their own (tests/test_cells_cpu.py builds this
// with the address and undefined-behaviour sanitizers and runs it).  The layout is restated here from its DEFINITION, not from the
// code under test: a 128-byte line per (row quad, 16-cell vector), the lines of a quad row running along x; two 64-byte sectors per
// line, one per row pair; a sector = [mask row 2p | mask row 2p + 1 | status row 2p | status row 2p + 1] in 16-byte parts; one guard
// quad above and one below every environment.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../simfire_amd/csrc/sf_cells.h"

namespace {

int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++failures <= 20) { std::printf("%s:%d: %s: ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

// what the accessors take of the library's Geo, among other fields in another order: "anything with these fields"
struct WideGeo {
    int E, H, W, P, PV;
    double other;
    long long age_env, plane_env;
    long long cells_env;
};

// the definition.  Offsets count from quad 0 of the environment (the guard quad above lies at negative offsets).
long long def_line(int PV, int y, int x) { return ((long long)(y / 4) * PV + x / 16) * 128; }
long long def_mask(int PV, int y, int x) { return def_line(PV, y, x) + ((y % 4) / 2) * 64 + (y % 2) * 16 + x % 16; }
long long def_status(int PV, int y, int x) { return def_line(PV, y, x) + ((y % 4) / 2) * 64 + (2 + y % 2) * 16 + x % 16; }
long long def_env_bytes(int H, int PV) { return (long long)((H + 3) / 4 + 2) * PV * 128; }

void check_grid(int H, int W, int PV)
{
    const int E = 2, P = PV * 16;
    const long long env = def_env_bytes(H, PV), guard = (long long)PV * 128;
    WideGeo wg{};
    wg.E = E; wg.H = H; wg.W = W; wg.P = P; wg.PV = PV; wg.plane_env = (long long)(H + 2) * P;
    wg.cells_env = bl_env_bytes(H, PV);
    CHECK(wg.cells_env == env, "H %d PV %d: %lld", H, PV, wg.cells_env);
    const CellGeo cg = cell_geo(wg);
    CHECK(cg.H == H && cg.W == W && cg.P == P && cg.PV == PV && cg.plane_env == wg.plane_env && cg.cells_env == env, "cell_geo");

    // ---- the byte map: injective, masks and status bytes apart, inside the environment past the guard quads
    std::vector<int> owner((size_t)env, 0);      // 0 free, else 1 + 2 * cell (+ 1 for a status byte)
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < P; ++x) {
            const long long m = bl_cell(PV, y, x), s = m + kBlStatus;
            CHECK(m == def_mask(PV, y, x) && s == def_status(PV, y, x), "(%d, %d) of H %d PV %d: mask %lld status %lld", y, x, H, PV, m, s);
            for (int k = 0; k < 2; ++k) {
                const long long at = guard + (k ? s : m);
                CHECK(at >= guard && at < env - guard, "(%d, %d) of H %d PV %d: offset %lld outside [%lld, %lld)", y, x, H, PV, at, guard, env - guard);
                if (at < 0 || at >= env) continue;
                CHECK(owner[(size_t)at] == 0, "(%d, %d) of H %d PV %d: byte %lld is taken", y, x, H, PV, at);
                owner[(size_t)at] = 1 + 2 * (y * P + x) + k;
            }
            if (x % 16 == 0) CHECK(bl_vec(PV, y, x / 16) + (y & 1) * 16 == m, "(%d, %d): the vector's offset is its first cell's", y, x);
        }

    // ---- the accessors on real planes (the sanitizer sees every access): blocked, base at quad 0 of environment 0
    std::vector<uint8_t> cells((size_t)(E * env), 0), status((size_t)(E * wg.plane_env), 0);
    const CellPlanesMut bl{status.data(), cells.data() + guard}, rm{status.data(), nullptr};
    const CellPlanes bl_c{bl.status, bl.cells}, rm_c{rm.status, nullptr};
    for (int e = 0; e < E; ++e)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < P; ++x) {
                uint8_t *sb = cell_status(bl, wg, e, y, x), *sr = cell_status(rm, cg, e, y, x);
                CHECK(sb - cells.data() == e * env + guard + def_status(PV, y, x), "blocked status byte of (%d, %d, %d)", e, y, x);
                CHECK(sr - status.data() == e * wg.plane_env + (long long)y * P + x, "row-major status byte of (%d, %d, %d)", e, y, x);
                CHECK(sb == bl_status(bl.cells, cg, e, y, x) && cell_status(bl_c, cg, e, y, x) == sb && cell_status(rm_c, wg, e, y, x) == sr, "forms of (%d, %d, %d)", e, y, x);
                CHECK(bl_mask_beside(sb) - cells.data() == e * env + guard + def_mask(PV, y, x) && bl_mask_beside(sb) == bl_mask(bl.cells, wg, e, y, x), "mask of (%d, %d, %d)", e, y, x);
                const long long o = e * wg.plane_env + (long long)y * P + x;
                const uint32_t *wb = cell_status_word(bl, wg, e, y, x, o), *wr = cell_status_word(rm, wg, e, y, x, o);
                CHECK((uintptr_t)wb % 4 == 0 && reinterpret_cast<const uint8_t *>(wb) + (x & 3) == sb, "blocked status word of (%d, %d, %d)", e, y, x);
                CHECK(reinterpret_cast<const uint8_t *>(wr) + (x & 3) == sr, "row-major status word of (%d, %d, %d)", e, y, x);
                if (x % 16 == 0) {
                    const int v = x / 16;
                    CHECK(cell_status_vec(bl, wg, e, y, v) == sb && cell_status_vec(rm, wg, e, y, v) == sr && bl_status_vec(bl.cells, wg, e, y, v) == sb &&
                          cell_status_vec(bl_c, cg, e, y, v) == sb, "status vector of (%d, %d, %d)", e, y, v);
                    CHECK(bl_mask_vec(bl.cells, wg, e, y, v) == bl_mask_beside(sb) && (uintptr_t)(sb - cells.data()) % 16 == 0, "mask vector of (%d, %d, %d)", e, y, v);
                }
                *sb = (uint8_t)(1 + (e + 3 * y + 7 * x) % 250);      // written through the mutable form ...
                *bl_mask_beside(sb) = (uint8_t)(1 + (e + 5 * y + 11 * x) % 250);
            }
    for (int e = 0; e < E; ++e)                                      // ... read back through the const one: nobody overwrote anybody
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < P; ++x) {
                CHECK(*cell_status(bl_c, wg, e, y, x) == (uint8_t)(1 + (e + 3 * y + 7 * x) % 250), "status of (%d, %d, %d) was overwritten", e, y, x);
                CHECK(*bl_mask(bl_c.cells, wg, e, y, x) == (uint8_t)(1 + (e + 5 * y + 11 * x) % 250), "mask of (%d, %d, %d) was overwritten", e, y, x);
            }
    long long used = 0;
    for (uint8_t b : cells) used += b != 0;
    CHECK(used == 2ll * E * H * P, "H %d PV %d: %lld bytes written for %d cells", H, PV, used, E * H * P);
    for (int e = 0; e < E; ++e)
        for (long long o = 0; o < guard; ++o)
            CHECK(cells[(size_t)(e * env + o)] == 0 && cells[(size_t)((e + 1) * env - guard + o)] == 0, "guard quad of environment %d was written", e);
}

}  // namespace

int main()
{
    const int Hs[] = {1, 2, 3, 4, 5, 9}, Ws[] = {1, 15, 16, 17, 33, 64};
    for (int H : Hs)
        for (int W : Ws) {
            check_grid(H, W, (W + 15) / 16);
            check_grid(H, W, (W + 15) / 16 + 1);      // a pitch with a whole vector of padding
        }
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
