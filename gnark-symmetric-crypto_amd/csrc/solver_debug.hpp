// TEST HOOK gsc_debug_solve (include/libprove.h, solver_debug.hip): the witness solver kernels on a caller's constraint system.
#pragma once
#include "../../include/libprove.h"

namespace gsc {
// 0, -2 (mode 1: the circuit does not qualify) or -3 (a device error, one line on stdout); throws std::runtime_error for what the hook or the builders refuse
int debug_solve(int device, const gsc_debug_solve_args& args);
}  // namespace gsc
