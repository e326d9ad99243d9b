// Which representation of the fire state is current on a handle, which structures derived from it still match it, and the only code
// that changes either.  Plain C++17, no HIP: tests/planes_check.cpp drives it on its own.
//
// The cells live in one of two layouts: the row-major planes (status, sprite masks) of the per-step kernels or the blocked plane of the
// resident launch (blocked).  Derived from the sprite masks: the vector bitmap of the resident launch (bits_valid: plane 0 matches
// them - k_run and the resets keep it, the per-step kernels do not; bits_fl_valid: planes 1 / 2 too - k_run on rows of several words
// keeps only plane 0 unless it runs as teams, which need all three) and the tile activity map + seam planes of the tiled per-step
// kernels (tiles_valid: they keep them, k_run and the per-cell kernel do not).  Derived from the status bytes: the per-tile
// histograms (hist_all_stale: every one is stale and no dirty mark says so on the device yet) and the result block with the sink's
// copy (row_fresh: they hold the current rows; whoever changes a status byte ends that).  Beside them what a launch plan asks:
// committed (commit[] is current: no per-step launch since the rings were last folded), fire_rows (no environment's fire spans more rows:
// 1 after a whole reset, + 2 per update, a fire advances one row per update and side at most, fire.py:163-234; 0 = not known),
// last_kind (launch structure of the last stepping call: 0 k_select + k_step, 1 fused, 2 k_run, 3 per-cell, 4 k_win in front of
// k_run; -1 none yet) and was_reset.
// Held by the book itself: blocked => !tiles_valid (the tile bookkeeping is not kept while the blocked plane is current).
// A writer is one of the named transitions below, each the host event its comment names.
#pragma once
#include <algorithm>

namespace {      // (internal linkage: the library exports its C ABI and nothing else)

class PlaneBook {
public:
    bool blocked() const { return blocked_; }
    bool bits_valid() const { return bits_valid_; }
    bool bits_cover_cells() const { return blocked_ && bits_valid_ && bits_fl_valid_; }      // the sparse passes may walk the bitmap over the blocked plane
    bool tiles_valid() const { return tiles_valid_; }
    bool tiles_kept() const { return !blocked_ && tiles_valid_; }      // a change of single environments rebuilds theirs
    bool hist_all_stale() const { return hist_all_stale_; }
    bool row_fresh() const { return row_fresh_; }
    bool committed() const { return committed_; }
    int fire_rows() const { return fire_rows_; }
    int last_kind() const { return last_kind_; }
    bool was_reset() const { return was_reset_; }

    // ---- reset, load, restore
    // a whole reset is about to write every environment in this layout: nothing is converted (sf_reset, in front of its launches)
    void reset_layout(bool blocked) { blocked_ = blocked; if (blocked) tiles_valid_ = false; }
    // the launches of a reset are enqueued (reset_launch): the histograms of its environments are written if they were known; a full
    // one has written every result row
    void reset_written(bool full, bool hist_known) { hist_all_stale_ = !hist_known; if (full) row_fresh_ = true; }
    // the whole reset has been waited for (sf_reset): every environment is freshly written, with its bitmaps and - row-major - its tiles
    void reset_done() { was_reset_ = true; bits_valid_ = bits_fl_valid_ = true; tiles_valid_ = !blocked_; fire_rows_ = 1; }
    // a fire map from outside replaced an environment's (sf_load_fire_map): its fire may be of any size
    void map_loaded() { fire_rows_ = 0; row_fresh_ = false; hist_all_stale_ = true; }
    // state blobs were loaded (sf_load_state), bound = the largest fire_rows they carry, 0 if one carries none: the bound covers them too
    void state_loaded(int bound) { fire_rows_ = (fire_rows_ > 0 && bound > 0) ? std::max(fire_rows_, bound) : 0; }

    // ---- changes from outside the step kernels
    void points_scattered() { row_fresh_ = false; }      // control-line points were written into the status bytes (scatter_points)
    // new sprites were written into running environments (ignite_rows), each into every derived structure that is valid: the fires
    // may be of any size, as after map_loaded, and status bytes changed
    void cells_ignited() { fire_rows_ = 0; row_fresh_ = false; }
    // another number of rows per band (sf_set_rows_per_band): tiles and histograms are laid out per wave tile
    void geometry_changed() { row_fresh_ = false; hist_all_stale_ = true; tiles_valid_ = false; }
    void family_switched() { hist_all_stale_ = true; }      // tiled <-> per-cell kernels (sf_set_generic): only the tiled ones keep the histograms
    void sink_replaced() { row_fresh_ = false; }            // sf_set_result_sink: the new sink is filled by the next refresh
    // the caller holds a writable alias of the row-major status plane (sf_fire_map_device while it is current): recount everything
    void alias_handed_out() { hist_all_stale_ = true; row_fresh_ = false; }

    // ---- conversions and rebuilds
    void converted_to_rm() { blocked_ = false; }                            // ensure_rm
    void converted_to_bl() { blocked_ = true; tiles_valid_ = false; }       // ensure_bl
    void tiles_rebuilt() { tiles_valid_ = !blocked_; }                      // ensure_tiles (from the row-major planes: it converts first)
    void bits_rebuilt() { bits_valid_ = bits_fl_valid_ = true; }            // ensure_vbits: all three planes
    // a team launch is coming (enqueue_steps): it reads all three planes, so a bitmap with only plane 0 is rebuilt
    void team_launch_next() { if (!bits_fl_valid_) bits_valid_ = false; }

    // ---- stepping
    // a stepping call begins (enqueue_steps, the first scatter + step pair): was the result block current?  It no longer is.
    bool call_begins() { const bool was = row_fresh_; row_fresh_ = false; return was; }
    void plain_run_wide() { bits_fl_valid_ = false; }      // the plain k_run ran on rows of several words (run_resident)
    // the resident rollout is enqueued (run_resident): result = its last launch leaves the result block, win_first = k_win went in front
    void resident_done(bool result, bool win_first) { row_fresh_ = result; tiles_valid_ = false; last_kind_ = win_first ? 4 : 2; }
    // n per-step launches are enqueued (enqueue_steps): they keep neither the bitmap nor - the per-cell kernel - the tiles
    void per_step_enqueued(bool generic, bool fused, int n)
    {
        if (n <= 0) return;
        bits_valid_ = false;
        if (generic) tiles_valid_ = false;
        last_kind_ = generic ? 3 : (fused ? 1 : 0);
        committed_ = false;
    }
    // n updates were made on a grid of H rows (enqueue_steps, sf_loop_step)
    void updates_made(int n, int H) { if (fire_rows_ > 0) fire_rows_ = (int)std::min<long long>(H, fire_rows_ + 2LL * n); }
    void rings_folded() { committed_ = true; }      // ensure_commit

    // ---- result block and the closed loop
    void hist_marked() { hist_all_stale_ = false; }      // every histogram was marked dirty on the device (mark_hist_dirty)
    // the result block was counted (refresh_status): from the tile histograms - the rows are current -, or by k_counts - the histograms
    // are not looked after any more; that this branch leaves the row as it is is kept as found
    void counted(bool by_tiles) { if (by_tiles) row_fresh_ = true; else hist_all_stale_ = true; }
    void loop_started() { row_fresh_ = false; tiles_valid_ = false; last_kind_ = 2; }      // sf_loop_start: the resident launch is running
    void loop_stopped() { row_fresh_ = true; }      // loop_stop: the workgroups left the result block behind

private:
    bool blocked_ = false, bits_valid_ = false, bits_fl_valid_ = true, tiles_valid_ = false;
    bool hist_all_stale_ = true, row_fresh_ = false, committed_ = true, was_reset_ = false;
    int fire_rows_ = 0, last_kind_ = -1;
};

}  // namespace
