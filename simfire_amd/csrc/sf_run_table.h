// The k_run instantiations of one translation unit of libsimfire_hip.so, as the host launches them (simfire_hip.hip: run_fn).  An entry is
// keyed by the template arguments k_run<MAXD, ATT, DIAG, MIT, TEAM> and holds the kernel's host handle.  The units share StepArgs by
// layout only (each has its own copy in an anonymous namespace): every table records its unit's sizeof(StepArgs), which the launcher checks.
// (a unit hands its table out of a host function, sf_runN_table(): a table at namespace scope would be compiled into the device code too)
#pragma once
#include <cstddef>

struct RunKey {
    int maxd, att, diag, mit, team;
    bool operator==(const RunKey &o) const { return maxd == o.maxd && att == o.att && diag == o.diag && mit == o.mit && team == o.team; }
};
struct RunEntry { RunKey key; const void *fn; };
struct RunTable { const RunEntry *entries; int n; size_t args_bytes; };

#define SF_RUN_ENTRY(D, A, G, M, T) {{D, A, G, M, T}, reinterpret_cast<const void *>(k_run<D, A, G, M, T>)}
