// TEST HOOK gsc_debug_assemble (include/libprove.h, assemble_debug.hip): the proof assembly kernels on a caller's sums and scalars.
#pragma once
#include "../../include/libprove.h"

namespace gsc {
// throws std::runtime_error with the refusal's reason; everything the host can decide is refused before a device is asked for
void debug_assemble(int device, const gsc_debug_assemble_args& args);
}  // namespace gsc
