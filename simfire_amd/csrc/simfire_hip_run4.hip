// Fourth translation unit of libsimfire_hip.so (see simfire_hip_run2.hip): the team kernels for two bitmap words per thread - grids of
// 1025 .. 2048 columns, BASELINE config C4.  Everything it shares with the first unit comes from the same headers (all in anonymous
// namespaces: each unit has its own copy of the device helpers); the first unit launches these kernels by their handles in the table
// below (sf_run_table.h).
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

RunTable sf_run4_table()
{
    static const RunEntry runs[] = {
        // [attenuation][diagonal spread read at run time / known to be on]
        SF_RUN_ENTRY(2, 0, -1, -1, 1), SF_RUN_ENTRY(2, 0, 1, -1, 1), SF_RUN_ENTRY(2, 1, -1, -1, 1), SF_RUN_ENTRY(2, 1, 1, -1, 1),
        // (diagonal spread on, no control lines inside the launch = BASELINE config C4: its own instantiations, without the control-line
        // code and its registers)
        SF_RUN_ENTRY(2, 0, 1, 0, 1), SF_RUN_ENTRY(2, 1, 1, 0, 1)};
    return {runs, (int)(sizeof runs / sizeof runs[0]), sizeof(StepArgs)};
}

#ifdef SF_WIN_PROF
// (profiles/win_prof.sh: this unit's own copy of the window loop's phase clocks - C4's team kernels live here)
extern "C" int sf_debug_win_prof4(unsigned long long *out /* [1024][16][8] */)
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_win_prof), sizeof(unsigned long long) * 1024 * 16 * 8) == hipSuccess ? 0 : -1;
}
#endif
