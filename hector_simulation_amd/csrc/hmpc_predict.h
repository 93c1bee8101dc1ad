// hmpc_predict.h -- host-visible side of the prediction kernel (hmpc_predict.hip): the model's own state trajectory and tracking
// cost of every instance of a batch, from its record and whatever its slot of the force buffer holds (hmpc_predict_states).
#pragma once
#include <hip/hip_runtime.h>

#include "hmpc_derived_shape.h"  // DERIVED_NT
#include "hmpc_kernel_args.h"

namespace hmpc {
constexpr int PREDICT_NT = DERIVED_NT;  // threads per workgroup (one workgroup per instance)

// One launch over the batch on `stream`.  Of `args` the kernel reads what stage A reads (records, stride, batch, horizon, dt, f_max, the
// robot constants) and `forces`; it writes states[batch][horizon][13] (binary32) and cost[batch][2] (binary64) and nothing else.
// Shapes: derived_shape (hmpc_derived_shape.h); anything else: hipErrorInvalidValue, nothing launched.
hipError_t launch_predict(int nc, const KernelArgs &args, float *states, double *cost, hipStream_t stream);

}  // namespace hmpc
