// What a handle knows about its terrain tables (one per environment with per_env_terrain, otherwise one), and the only code that
// changes it.  Plain C++17, no HIP: tests/tables_check.cpp drives it on its own.
//
// Per table: has an R table been supplied (rt), are its layers on the device (layers), is its fuel FBFM-coded (fbfm), and which of the
// four buffers derived from the table are behind it - sf_render's background words (bg_stale), the cell-major copy of the R table
// (rtc_stale, ensure_rtc), the table's part of the cache of wind-independent terms (wt_stale, ensure_wterms) and its part of
// sf_behavior's cache of the heat per unit area (hpa_stale, ensure_hpa: behind whatever puts wt_stale behind and behind a terrain
// copy; a wind change leaves it alone).  The stale flags start at 1: everything is stale until its buffer exists and has been built.
// Over the tables, two caches of the handle: rtc_valid (no table's cell-major copy is stale: ensure_rtc has nothing to do) and
// wind_sched_ready (the wind cache has been made current for the scheduled tables since the last change of either).
// A writer is one of the named transitions below; a list may be empty or name a table twice.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace {      // (internal linkage: the library exports its C ABI and nothing else)

// the tables lo .. hi - 1 as a list
inline std::vector<int32_t> iota_tabs(int lo, int hi)
{
    std::vector<int32_t> tabs;
    for (int i = lo; i < hi; ++i) tabs.push_back(i);
    return tabs;
}

class TableBook {
public:
    struct Table { char rt = 0, layers = 0, fbfm = 0, bg_stale = 1, rtc_stale = 1, wt_stale = 1, hpa_stale = 1; };

    void init(size_t n_tables) { t_.assign(n_tables, Table()); rtc_valid_ = wind_sched_ready_ = false; }      // sf_create
    int size() const { return (int)t_.size(); }
    const Table &operator[](size_t t) const { return t_[t]; }
    bool have_rt() const { for (const Table &t : t_) if (!t.rt) return false; return true; }      // every table has an R table
    bool any_wt_stale() const { for (const Table &t : t_) if (t.wt_stale) return true; return false; }
    bool rtc_valid() const { return rtc_valid_; }
    bool wind_sched_ready() const { return wind_sched_ready_; }

    // the listed tables were built from layers now on the device (sf_set_layers*, sf_generate_layers)
    void layers_set(const int32_t *tabs, int n, bool fbfm)
    {
        for (int k = 0; k < n; ++k) { Table &t = t_[tabs[k]]; t.layers = 1; t.fbfm = fbfm; t.bg_stale = 1; }
        rtable_set(tabs, n);
    }
    // the listed R tables were replaced (sf_set_rtable*): what is derived from the table is behind it, the layers are as they were
    void rtable_set(const int32_t *tabs, int n)
    {
        for (int k = 0; k < n; ++k) { Table &t = t_[tabs[k]]; t.rt = t.rtc_stale = t.wt_stale = t.hpa_stale = 1; }
        rtc_valid_ = wind_sched_ready_ = false;
    }
    // a wind change rebuilt the listed R tables (sf_set_wind); the cell-major copy, where the buffer exists, was written in the same pass
    void wind_rebuilt(const int32_t *tabs, int n, bool rtc_exists)
    {
        for (int k = 0; k < n; ++k) { Table &t = t_[tabs[k]]; t.rt = 1; t.rtc_stale = !rtc_exists; }
    }
    // table dst is now a copy of table src, its slices of the derived buffers included (sf_copy_envs with the terrain); the background
    // words are not copied
    void copied(int dst, int src, bool rtc_exists)
    {
        Table &d = t_[dst];
        d = t_[src];
        d.bg_stale = d.hpa_stale = 1;      // (the heat cache is not a slice of the copy: rebuilt at the next sf_behavior)
        if (!rtc_exists || d.rtc_stale) rtc_valid_ = false;
    }
    void rtc_built() { for (Table &t : t_) t.rtc_stale = 0; rtc_valid_ = true; }      // ensure_rtc: every stale copy rebuilt
    void wterms_allocated() { for (Table &t : t_) t.wt_stale = 1; }                   // ensure_wterms: a new, empty cache
    void wterms_built(int t) { t_[t].wt_stale = 0; }
    void hpa_allocated() { for (Table &t : t_) t.hpa_stale = 1; }                      // ensure_hpa: a new, empty cache
    void hpa_built(int t) { t_[t].hpa_stale = 0; }
    void background_built(int t) { t_[t].bg_stale = 0; }                              // sf_render
    void rgb_changed() { for (Table &t : t_) if (!t.fbfm) t.bg_stale = 1; }           // sf_render: other fuel colours (FBFM colours are fixed)
    // the set of scheduled tables changed, or whether there is a cache (wind_sched_count, sf_set_wind_lab); wind_sched_pass made it current
    void schedule_changed() { wind_sched_ready_ = false; }
    void schedule_ready() { wind_sched_ready_ = true; }

private:
    std::vector<Table> t_;
    bool rtc_valid_ = false, wind_sched_ready_ = false;
};

}  // namespace
