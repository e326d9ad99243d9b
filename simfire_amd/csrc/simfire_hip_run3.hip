// Third translation unit of libsimfire_hip.so (see simfire_hip_run2.hip): k_run for two and four bitmap words per thread - more than 1024
// rows per workgroup, or 8-wave workgroups on 1024 rows (the many-environments regime).  Everything it shares with the first unit
// comes from the same headers (all in anonymous namespaces: each unit has its own copy of the device helpers); the first unit launches
// these kernels by their handles in the table below (sf_run_table.h).
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

RunTable sf_run3_table()
{
    static const RunEntry runs[] = {
        // the closed loop of sf_loop_start with two bitmap rows per thread: 8-wave workgroups on 1024 rows, two to a CU - the light loop, which leaves
        // half of every CU to the harness's own kernels (SF_TUNE_LOOP_LIGHT).  Diagonal spread is looked up at run time.
        SF_RUN_ENTRY(2, 0, -1, -2, 0), SF_RUN_ENTRY(2, 1, -1, -2, 0),
        // two words per thread: [attenuation off / on][diagonal spread read at run time / known to be on]
        SF_RUN_ENTRY(2, 0, -1, -1, 0), SF_RUN_ENTRY(2, 0, 1, -1, 0), SF_RUN_ENTRY(2, 1, -1, -1, 0), SF_RUN_ENTRY(2, 1, 1, -1, 0),
        // four words per thread: diagonal spread read at run time only
        SF_RUN_ENTRY(kRunMaxD, 0, -1, -1, 0), SF_RUN_ENTRY(kRunMaxD, 1, -1, -1, 0),
        // two words per thread, diagonal spread known to be on, no control lines inside the launch: the instantiations with the window phase
        SF_RUN_ENTRY(2, 0, 1, 0, 0), SF_RUN_ENTRY(2, 1, 1, 0, 0)};
    return {runs, (int)(sizeof runs / sizeof runs[0]), sizeof(StepArgs)};
}
