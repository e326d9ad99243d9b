// Second translation unit of libsimfire_hip.so: instantiations of k_run that only some handles ever launch - the team launch on one-word
// rows (k_run<1, ..., TEAM = 1>), teams that grow inside the launch (TEAM = 2) and the closed loop (k_run<MIT = -2>) - compiled beside
// simfire_hip.hip so that the library builds in the time of the largest unit (python -m simfire_amd.build runs the compiles side by side;
// simfire_hip_run3.hip: the plain kernels for several bitmap words per thread, simfire_hip_run4.hip: the team kernels for two).  Everything
// it shares with the first unit comes from the same headers (all in anonymous namespaces: each unit has its own copy of the device helpers);
// the first unit launches these kernels by their handles in the table below (sf_run_table.h).
// Replaces (like sf_run_kernels.h): n calls of RothermelFireManager.update per environment, simfire/game/managers/fire.py:616-719.
// (only the k_run instantiations below are compiled here: the kernels every handle launches live in simfire_hip.hip alone)
#define SF_RUN_UNIT 1
#include <hip/hip_runtime.h>

#include "../../include/simfire_hip.h"
#include "sf_common.h"
#include "sf_step_kernels.h"
#include "sf_aux_kernels.h"
#include "sf_run_kernels.h"
#include "sf_run_table.h"

RunTable sf_run2_table()
{
    static const RunEntry runs[] = {
        // teams on one-word rows: [attenuation][diagonal spread read at run time / known to be on]
        SF_RUN_ENTRY(1, 0, -1, -1, 1), SF_RUN_ENTRY(1, 0, 1, -1, 1), SF_RUN_ENTRY(1, 1, -1, -1, 1), SF_RUN_ENTRY(1, 1, 1, -1, 1),
        // teams that grow inside the launch: one-word rows, diagonal spread, no control lines inside the launch
        // (the first without the statistics of sf_get_counters - bench.py's kernel - and once more with them, TEAM = 3, for handles with the counters on)
        SF_RUN_ENTRY(1, 0, 1, 0, 2), SF_RUN_ENTRY(1, 0, 1, 0, 3), SF_RUN_ENTRY(1, 1, 1, 0, 2),
        // the closed loop of sf_loop_start: one workgroup per environment, steps until the host's stop
        // (diagonal spread is looked up at run time: the two instantiations that knew it at compile time were retired in round 6 for k_win's two -
        // a select or two per batch in a call whose time is the signalling between host and device)
        SF_RUN_ENTRY(1, 0, -1, -2, 0), SF_RUN_ENTRY(1, 1, -1, -2, 0)};
    return {runs, (int)(sizeof runs / sizeof runs[0]), sizeof(StepArgs)};
}
