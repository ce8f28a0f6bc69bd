// TEST HOOK gsc_debug_msm (include/libprove.h, msm_debug.hip): the MSM kernels on a caller's bases and scalars.
#pragma once
#include "../../include/libprove.h"

namespace gsc {
// throws std::runtime_error with the refusal's reason; everything the host can decide is refused before a device is asked for
void debug_msm(int device, const gsc_debug_msm_args& args);
}  // namespace gsc
