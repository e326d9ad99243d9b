// Stand-alone check of PlaneBook (simfire_amd/csrc/sf_planes.h): a book driven through scripted sequences of host events, every query
// compared after every operation with literals written down from the rules the host code followed while the flags were ten loose
// fields of the handle (tests/test_planes_cpu.py builds this with the address and undefined-behaviour sanitizers and runs it).
//
// A book is written as nine digits - blocked, bits_valid, bits_cover_cells, tiles_valid, tiles_kept, hist_all_stale, row_fresh,
// committed, was_reset - then fire_rows and last_kind.  Every grid here has kH rows.
#include <cstdio>
#include <string>

#include "../simfire_amd/csrc/sf_planes.h"

static int g_failed = 0;
static const int kH = 64;

static std::string digits(const PlaneBook &b)
{
    std::string s;
    for (bool f : {b.blocked(), b.bits_valid(), b.bits_cover_cells(), b.tiles_valid(), b.tiles_kept(), b.hist_all_stale(), b.row_fresh(),
                   b.committed(), b.was_reset()})
        s += f ? '1' : '0';
    return s;
}

// what holds after every operation, whatever the sequence
static void invariants(int line, const PlaneBook &b)
{
    const char *what = nullptr;
    if (b.blocked() && b.tiles_valid()) what = "blocked and tiles_valid";
    else if (b.bits_cover_cells() && !b.blocked()) what = "bits_cover_cells without blocked";
    else if (b.bits_cover_cells() && !b.bits_valid()) what = "bits_cover_cells without bits_valid";
    else if (b.tiles_kept() != (!b.blocked() && b.tiles_valid())) what = "tiles_kept is not !blocked && tiles_valid";
    else if (b.fire_rows() < 0 || b.fire_rows() > kH) what = "fire_rows outside 0 .. H";
    if (!what) return;
    ++g_failed;
    std::printf("line %d: invariant broken: %s (%s %d %d)\n", line, what, digits(b).c_str(), b.fire_rows(), b.last_kind());
}
static void expect(int line, const PlaneBook &b, const char *flags, int fire_rows, int last_kind)
{
    invariants(line, b);
    if (digits(b) == flags && b.fire_rows() == fire_rows && b.last_kind() == last_kind) return;
    ++g_failed;
    std::printf("line %d: got %s %d %d, expected %s %d %d\n", line, digits(b).c_str(), b.fire_rows(), b.last_kind(), flags, fire_rows, last_kind);
}
#define EXPECT(...) expect(__LINE__, __VA_ARGS__)
// an event that changes status bytes (or what the result block is copied to): a fresh row does not survive it
#define ENDS_ROW(b, op) do { (b).op; if ((b).row_fresh()) { ++g_failed; std::printf("line %d: the row is still fresh behind " #op "\n", __LINE__); } } while (0)
static void check(int line, bool ok, const char *what)
{
    if (!ok) { ++g_failed; std::printf("line %d: %s\n", line, what); }
}
#define CHECK(ok) check(__LINE__, ok, #ok)

// The events of one handle's life on a 64 x 64 grid in automatic mode (tests/test_call_layers_gpu.py, "auto", reduced to its events):
// reset, step(1) + status pairs on the fused per-step kernel, the single update as the resident launch, a look at the map behind a
// per-step update, control lines inside the resident launch and as scatter + step pairs, a rollout.
static void auto_script()
{
    PlaneBook b;
    EXPECT(b, "000001010", 0, -1);             // a new handle: row-major, nothing built, every histogram stale, nothing to fold
    b.reset_layout(true);                      // sf_reset: nothing has stepped and the resident launch is the automatic choice
    EXPECT(b, "100001010", 0, -1);
    b.reset_written(true, true);
    EXPECT(b, "100000110", 0, -1);
    b.reset_done();
    EXPECT(b, "111000111", 1, -1);
    for (int pair = 0; pair < 2; ++pair) {     // step(1) on the fused kernel, status
        CHECK(b.call_begins() == true);
        EXPECT(b, pair ? "000110011" : "111000011", 1 + 2 * pair, pair ? 1 : -1);
        if (pair == 0) {                       // (ensure_tiles: back to the row-major planes, then the tiles)
            b.converted_to_rm();
            EXPECT(b, "010000011", 1, -1);
            b.tiles_rebuilt();
            EXPECT(b, "010110011", 1, -1);
        }
        b.per_step_enqueued(false, true, 1);
        EXPECT(b, "000110001", 1 + 2 * pair, 1);
        b.updates_made(1, kH);
        EXPECT(b, "000110001", 3 + 2 * pair, 1);
        b.rings_folded();                      // status: the rings, the dirty marks (none owed), the count from the histograms
        EXPECT(b, "000110011", 3 + 2 * pair, 1);
        b.hist_marked();
        EXPECT(b, "000110011", 3 + 2 * pair, 1);
        b.counted(true);
        EXPECT(b, "000110111", 3 + 2 * pair, 1);
    }
    CHECK(b.call_begins() == true);            // the single update as the resident launch (not a team)
    EXPECT(b, "000110011", 5, 1);
    b.bits_rebuilt();
    EXPECT(b, "010110011", 5, 1);
    b.converted_to_bl();                       // the tiles are not kept from here on
    EXPECT(b, "111000011", 5, 1);
    b.hist_marked();
    b.resident_done(true, false);
    EXPECT(b, "111000111", 5, 2);
    b.updates_made(1, kH);
    EXPECT(b, "111000111", 7, 2);              // (a status query now: the row is fresh, nothing to do)
    CHECK(b.call_begins() == true);            // step(1) on the per-step kernel again; the look at the map changes nothing
    b.converted_to_rm();
    b.tiles_rebuilt();
    EXPECT(b, "010110011", 7, 2);
    b.per_step_enqueued(false, true, 1);
    b.updates_made(1, kH);
    EXPECT(b, "000110001", 9, 1);
    CHECK(b.call_begins() == false);           // control lines inside the resident launch, two updates
    b.rings_folded();
    b.bits_rebuilt();
    b.converted_to_bl();
    EXPECT(b, "111000011", 9, 1);
    b.hist_marked();
    b.resident_done(true, false);
    b.updates_made(2, kH);
    EXPECT(b, "111000111", 13, 2);
    CHECK(b.call_begins() == true);            // control lines as scatter + step pairs (enqueue_pair, then the update's own call)
    ENDS_ROW(b, points_scattered());
    EXPECT(b, "111000011", 13, 2);
    CHECK(b.call_begins() == false);
    b.converted_to_rm();
    b.tiles_rebuilt();
    b.per_step_enqueued(false, false, 1);      // (k_select + k_step)
    b.updates_made(1, kH);
    EXPECT(b, "000110001", 15, 0);
    ENDS_ROW(b, points_scattered());           // the second pair: nothing to convert or rebuild
    CHECK(b.call_begins() == false);
    b.per_step_enqueued(false, false, 1);
    b.updates_made(1, kH);
    EXPECT(b, "000110001", 17, 0);
    CHECK(b.call_begins() == false);           // rollout(2): resident, k_win in front; the refresh behind it finds the row fresh
    b.rings_folded();
    b.bits_rebuilt();
    b.converted_to_bl();
    b.hist_marked();
    b.resident_done(true, true);
    b.updates_made(2, kH);
    EXPECT(b, "111000111", 21, 4);
    b.per_step_enqueued(false, true, 0);       // a call of no updates enqueues nothing
    b.updates_made(0, kH);
    EXPECT(b, "111000111", 21, 4);
}

// A whole reset into either layout behind each kind of last launch (sf_reset picks blocked where the resident launch is the handle's
// choice and it ran last, the blocked plane is current or nothing has stepped), and the partial reset.
static void resets()
{
    PlaneBook b;
    b.reset_layout(false);                     // a handle whose options rule the resident launch out
    b.reset_written(true, true);
    b.reset_done();
    EXPECT(b, "010110111", 1, -1);             // row-major: the reset writes the tiles too
    CHECK(b.call_begins() == true);
    b.per_step_enqueued(false, false, 3);
    b.updates_made(3, kH);
    EXPECT(b, "000110001", 7, 0);
    b.rings_folded();                          // sf_reset folds first
    b.reset_layout(false);                     // behind kind 0 / 1 on the row-major planes
    EXPECT(b, "000110011", 7, 0);
    b.reset_written(true, true);
    EXPECT(b, "000110111", 7, 0);
    b.reset_done();
    EXPECT(b, "010110111", 1, 0);
    b.family_switched();                       // behind the per-cell kernel: no histogram is known
    EXPECT(b, "010111111", 1, 0);
    CHECK(b.call_begins() == true);
    b.per_step_enqueued(true, false, 2);
    b.updates_made(2, kH);
    EXPECT(b, "000001001", 5, 3);
    b.rings_folded();
    b.reset_layout(false);
    b.reset_written(true, false);
    b.reset_done();
    EXPECT(b, "010111111", 1, 3);
    b.family_switched();                       // tiled again; a resident call, then a reset into the blocked plane (kind 2, blocked)
    CHECK(b.call_begins() == true);
    b.converted_to_bl();
    b.hist_marked();
    b.resident_done(true, false);
    b.updates_made(2, kH);
    EXPECT(b, "111000111", 5, 2);
    b.reset_layout(true);
    b.reset_written(true, true);
    b.reset_done();
    EXPECT(b, "111000111", 1, 2);
    CHECK(b.call_begins() == true);            // k_win in front without the result block, a count by k_counts' route back to row-major ...
    b.resident_done(false, true);
    b.updates_made(2, kH);
    EXPECT(b, "111000011", 5, 4);
    b.converted_to_rm();
    EXPECT(b, "010000011", 5, 4);
    b.reset_layout(false);                     // ... and behind kind 4 on the row-major planes the reset stays there: tiles written
    b.reset_written(true, true);
    b.reset_done();
    EXPECT(b, "010110111", 1, 4);
    b.reset_written(false, true);              // a partial reset: the histograms stay known, the row as it is
    EXPECT(b, "010110111", 1, 4);
    CHECK(b.call_begins() == true);
    b.reset_written(false, true);
    EXPECT(b, "010110011", 1, 4);
    b.family_switched();
    b.reset_written(false, false);             // ... nothing is known while every histogram is stale anyway
    EXPECT(b, "010111011", 1, 4);
    b.hist_marked();
    b.reset_written(false, true);
    EXPECT(b, "010110011", 1, 4);
    b.reset_layout(true);                      // blocked by itself ends the tiles (a reset that fails behind this leaves no "impossible" state)
    EXPECT(b, "111000011", 1, 4);              // (the bitmaps, valid before, say nothing of the tiles)
}

// The plain k_run on rows of several words keeps only plane 0 of the bitmap; a team launch behind it has the bitmap rebuilt.
static void wide_rows()
{
    PlaneBook b;
    b.reset_layout(true);
    b.reset_written(true, true);
    b.reset_done();
    (void)b.call_begins();
    b.team_launch_next();                      // all three planes valid: nothing to rebuild
    EXPECT(b, "111000011", 1, -1);
    b.plain_run_wide();
    EXPECT(b, "110000011", 1, -1);             // plane 0 still matches: the plain kernel goes on; the sparse passes may not
    b.resident_done(true, false);
    b.updates_made(4, kH);
    EXPECT(b, "110000111", 9, 2);
    CHECK(b.call_begins() == true);
    b.team_launch_next();
    EXPECT(b, "100000011", 9, 2);              // ensure_vbits has work
    b.bits_rebuilt();
    EXPECT(b, "111000011", 9, 2);
    b.resident_done(true, false);
    b.updates_made(4, kH);
    EXPECT(b, "111000111", 17, 2);
    (void)b.call_begins();                     // per-step launches in between: plane 0 is gone too, a rebuild restores all three
    b.converted_to_rm();
    b.tiles_rebuilt();
    b.per_step_enqueued(false, false, 1);
    b.updates_made(1, kH);
    EXPECT(b, "000110001", 19, 0);
    b.team_launch_next();
    EXPECT(b, "000110001", 19, 0);
    b.rings_folded();
    b.bits_rebuilt();
    b.converted_to_bl();
    EXPECT(b, "111000011", 19, 0);
}

// Changes from outside the step kernels, the two ways of counting, the closed loop, state blobs, the bound on the fires' rows.
static void outside_changes()
{
    PlaneBook b;
    b.reset_layout(false);
    b.reset_written(true, true);
    b.reset_done();
    EXPECT(b, "010110111", 1, -1);
    b.family_switched();                       // sf_set_generic(1)
    EXPECT(b, "010111111", 1, -1);
    CHECK(b.call_begins() == true);
    b.per_step_enqueued(true, false, 2);       // the per-cell kernel keeps neither bitmap nor tiles
    b.updates_made(2, kH);
    EXPECT(b, "000001001", 5, 3);
    b.rings_folded();
    b.counted(false);                          // k_counts: the row is left as it is (kept as found), every histogram stale
    EXPECT(b, "000001011", 5, 3);
    b.family_switched();                       // sf_set_generic(0): the tiles are rebuilt before the next tiled step
    EXPECT(b, "000001011", 5, 3);
    CHECK(b.call_begins() == false);
    b.tiles_rebuilt();
    b.per_step_enqueued(false, true, 1);
    b.updates_made(1, kH);
    EXPECT(b, "000111001", 7, 1);
    b.rings_folded();
    b.hist_marked();                           // the dirty marks are owed now
    EXPECT(b, "000110011", 7, 1);
    b.counted(true);
    EXPECT(b, "000110111", 7, 1);
    ENDS_ROW(b, geometry_changed());           // sf_set_rows_per_band
    EXPECT(b, "000001011", 7, 1);
    b.tiles_rebuilt();
    b.hist_marked();
    b.counted(true);
    EXPECT(b, "000110111", 7, 1);
    ENDS_ROW(b, sink_replaced());              // sf_set_result_sink
    EXPECT(b, "000110011", 7, 1);
    b.counted(true);
    ENDS_ROW(b, alias_handed_out());           // sf_fire_map_device on the row-major planes
    EXPECT(b, "000111011", 7, 1);
    b.hist_marked();
    b.counted(true);
    ENDS_ROW(b, map_loaded());                 // sf_load_fire_map: a fire of any size
    EXPECT(b, "000111011", 0, 1);
    b.updates_made(3, kH);                     // an unknown bound stays unknown
    EXPECT(b, "000111011", 0, 1);
    b.hist_marked();
    b.counted(true);
    EXPECT(b, "000110111", 0, 1);
    b.reset_written(true, true);               // a whole reset makes the bound known again
    b.reset_done();
    EXPECT(b, "010110111", 1, 1);
    b.bits_rebuilt();                          // sf_loop_start: bitmap, blocked plane, marks, the launch
    b.converted_to_bl();
    b.hist_marked();
    ENDS_ROW(b, loop_started());
    EXPECT(b, "111000011", 1, 2);
    b.updates_made(1, kH);                     // sf_loop_step, twice
    b.updates_made(1, kH);
    EXPECT(b, "111000011", 5, 2);
    b.loop_stopped();
    EXPECT(b, "111000111", 5, 2);
    b.state_loaded(9);                         // blobs with a larger bound, a smaller one, none
    EXPECT(b, "111000111", 9, 2);
    b.state_loaded(3);
    EXPECT(b, "111000111", 9, 2);
    b.state_loaded(0);
    EXPECT(b, "111000111", 0, 2);
    b.state_loaded(7);                         // (unknown stays unknown: other environments' fires are not the blobs')
    EXPECT(b, "111000111", 0, 2);
    b.reset_layout(true);
    b.reset_written(true, true);
    b.reset_done();
    b.updates_made(31, kH);                    // the bound saturates at the grid's height
    EXPECT(b, "111000111", 63, 2);
    b.updates_made(1, kH);
    EXPECT(b, "111000111", 64, 2);
    b.updates_made(1000000000, kH);
    EXPECT(b, "111000111", 64, 2);
    b.converted_to_rm();                       // the tiles on the row-major planes of a handle that was blocked: kept only once rebuilt
    EXPECT(b, "010000111", 64, 2);
    b.tiles_rebuilt();
    EXPECT(b, "010110111", 64, 2);
}

int main()
{
    auto_script();
    resets();
    wide_rows();
    outside_changes();
    if (g_failed) std::printf("FAILED: %d\n", g_failed);
    else std::printf("ok\n");
    return g_failed ? 1 : 0;
}
