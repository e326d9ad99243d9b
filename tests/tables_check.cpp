// Stand-alone check of TableBook (simfire_amd/csrc/sf_tables.h): a 3-table and a 1-table book driven through scripted sequences, every
// flag compared after every operation with literals written down from the rules the host code followed while the flags were six
// parallel vectors (tests/test_tables_cpu.py builds this with the address and undefined-behaviour sanitizers and runs it).
//
// A table is written as six digits: rt layers fbfm bg_stale rtc_stale wt_stale.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../simfire_amd/csrc/sf_tables.h"

static int g_failed = 0;

static std::string row(const TableBook &b, int t)
{
    const TableBook::Table &r = b[t];
    std::string s;
    for (char c : {r.rt, r.layers, r.fbfm, r.bg_stale, r.rtc_stale, r.wt_stale}) s += c ? '1' : '0';
    return s;
}

// the whole book: its tables, then have_rt / rtc_valid / wind_sched_ready
static void expect(int line, const TableBook &b, const std::vector<std::string> &tables, bool have_rt, bool rtc_valid, bool ready)
{
    bool ok = b.size() == (int)tables.size() && b.have_rt() == have_rt && b.rtc_valid() == rtc_valid && b.wind_sched_ready() == ready;
    bool any_wt = false;
    for (int t = 0; ok && t < b.size(); ++t) { ok = row(b, t) == tables[t]; any_wt = any_wt || tables[t][5] == '1'; }
    if (ok && b.any_wt_stale() != any_wt) ok = false;
    if (ok) return;
    ++g_failed;
    std::printf("line %d: got", line);
    for (int t = 0; t < b.size(); ++t) std::printf(" %s", row(b, t).c_str());
    std::printf(" have_rt=%d rtc_valid=%d ready=%d any_wt_stale=%d, expected", b.have_rt(), b.rtc_valid(), b.wind_sched_ready(), b.any_wt_stale());
    for (const std::string &s : tables) std::printf(" %s", s.c_str());
    std::printf(" have_rt=%d rtc_valid=%d ready=%d\n", have_rt, rtc_valid, ready);
}
#define EXPECT(...) expect(__LINE__, __VA_ARGS__)

static void three_tables()
{
    TableBook b;
    b.init(3);
    EXPECT(b, {"000111", "000111", "000111"}, false, false, false);      // fresh: everything stale, nothing supplied
    const int32_t one[] = {1}, outer[] = {0, 2}, zero[] = {0}, two[] = {2};
    b.layers_set(one, 1, false);
    EXPECT(b, {"000111", "110111", "000111"}, false, false, false);      // one table of three: not ready to step
    b.layers_set(outer, 2, true);
    EXPECT(b, {"111111", "110111", "111111"}, true, false, false);
    b.rtc_built();
    EXPECT(b, {"111101", "110101", "111101"}, true, true, false);
    b.schedule_ready();
    EXPECT(b, {"111101", "110101", "111101"}, true, true, true);
    b.wterms_built(0);
    b.wterms_built(2);
    EXPECT(b, {"111100", "110101", "111100"}, true, true, true);
    b.wterms_allocated();                                                 // a new cache holds nothing, whatever was marked before
    EXPECT(b, {"111101", "110101", "111101"}, true, true, true);
    b.wterms_built(0);
    EXPECT(b, {"111100", "110101", "111101"}, true, true, true);
    b.background_built(0);
    b.background_built(1);
    EXPECT(b, {"111000", "110001", "111101"}, true, true, true);
    b.rgb_changed();                                                      // FBFM colours are fixed: table 0 keeps its background
    EXPECT(b, {"111000", "110101", "111101"}, true, true, true);
    b.rtable_set(zero, 1);                                                // layers, fbfm and the background are as they were
    EXPECT(b, {"111011", "110101", "111101"}, true, false, false);
    b.wind_rebuilt(zero, 1, true);                                        // the cell-major copy was written in the same pass
    EXPECT(b, {"111001", "110101", "111101"}, true, false, false);
    b.rtc_built();
    EXPECT(b, {"111001", "110101", "111101"}, true, true, false);
    b.wind_rebuilt(two, 1, false);                                        // no cell-major buffer: stale; rtc_valid is not this operation's
    EXPECT(b, {"111001", "110101", "111111"}, true, true, false);
    b.copied(1, 0, true);                                                 // a clean source: nothing to rebuild but the background
    EXPECT(b, {"111001", "111101", "111111"}, true, true, false);
    b.copied(0, 2, true);                                                 // a stale source onto a clean destination
    EXPECT(b, {"111111", "111101", "111111"}, true, false, false);
    b.copied(2, 1, true);                                                 // a clean source onto a stale destination: rtc_valid stays down
    EXPECT(b, {"111111", "111101", "111101"}, true, false, false);
    b.rtc_built();
    EXPECT(b, {"111101", "111101", "111101"}, true, true, false);
    b.copied(2, 1, false);                                                // without a cell-major buffer nothing is valid
    EXPECT(b, {"111101", "111101", "111101"}, true, false, false);
    // an empty list changes no table; layers_set / rtable_set still drop the two caches, wind_rebuilt does not
    b.rtc_built();
    b.schedule_ready();
    b.wind_rebuilt(nullptr, 0, true);
    EXPECT(b, {"111101", "111101", "111101"}, true, true, true);
    b.schedule_changed();
    EXPECT(b, {"111101", "111101", "111101"}, true, true, false);
    b.schedule_ready();
    b.layers_set(nullptr, 0, false);
    EXPECT(b, {"111101", "111101", "111101"}, true, false, false);
    b.rtc_built();
    b.schedule_ready();
    b.rtable_set(nullptr, 0);
    EXPECT(b, {"111101", "111101", "111101"}, true, false, false);
    // a table named twice is a table named once
    const int32_t ones[] = {1, 1}, twos[] = {2, 2};
    b.rtable_set(ones, 2);
    EXPECT(b, {"111101", "111111", "111101"}, true, false, false);
    b.layers_set(twos, 2, false);
    EXPECT(b, {"111101", "111111", "110111"}, true, false, false);
    b.wind_rebuilt(ones, 2, true);
    EXPECT(b, {"111101", "111101", "110111"}, true, false, false);
}

static void one_table()
{
    TableBook b;
    b.init(1);
    EXPECT(b, {"000111"}, false, false, false);
    const int32_t zero[] = {0};
    b.rtable_set(zero, 1);                                                // an R table without layers
    EXPECT(b, {"100111"}, true, false, false);
    b.wind_rebuilt(zero, 1, false);
    EXPECT(b, {"100111"}, true, false, false);
    b.wind_rebuilt(zero, 1, true);
    EXPECT(b, {"100101"}, true, false, false);
    b.background_built(0);
    EXPECT(b, {"100001"}, true, false, false);
    b.rgb_changed();
    EXPECT(b, {"100101"}, true, false, false);
    b.layers_set(zero, 1, true);
    EXPECT(b, {"111111"}, true, false, false);
    b.background_built(0);
    b.rgb_changed();
    EXPECT(b, {"111011"}, true, false, false);
    b.wterms_allocated();
    b.wterms_built(0);
    b.rtc_built();
    EXPECT(b, {"111000"}, true, true, false);
    b.init(1);                                                            // (a new handle)
    EXPECT(b, {"000111"}, false, false, false);
}

int main()
{
    three_tables();
    one_table();
    const std::vector<int32_t> tabs = iota_tabs(2, 5), none = iota_tabs(3, 3);
    if (tabs != std::vector<int32_t>{2, 3, 4} || !none.empty()) { ++g_failed; std::printf("iota_tabs\n"); }
    if (g_failed) std::printf("FAILED: %d\n", g_failed);
    else std::printf("ok\n");
    return g_failed ? 1 : 0;
}
