// hmpc_builder_launch.h -- host-visible side of the kernels of hmpc_builder.h (compiled in hmpc_builder.hip, the one unit that may
// include them: they are no templates): one launch function per kernel, on `stream`, returning hipGetLastError().  Counts of 0 launch nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hector_mpc.h"

#pragma GCC visibility push(hidden)
namespace hmpc {

// rows f1 + f2: records[batch] (and cls[batch], wpd_out[batch][2] where not nullptr) from ticks[batch]
hipError_t launch_build_records(const hmpc_tick_inputs *ticks, int batch, int h, double dtMPC, unsigned char *records, int stride,
                                double *wpd_out, float f_max, unsigned char *cls, hipStream_t stream);
// cls[batch]: the size classes of two-contact records that are already in HBM
hipError_t launch_classify_records(const unsigned char *records, int stride, int batch, int h, float f_max, unsigned char *cls,
                                   hipStream_t stream);
// longest-first dispatch: keys[batch] = predicted cost buckets of the records; order[batch] = the instances sorted by keys, or
// (keys == nullptr) by the iteration counts of status[batch]
hipError_t launch_predicted_cost(const unsigned char *records, int stride, int batch, int h, int nc, unsigned char *keys, hipStream_t stream);
hipError_t launch_dispatch_order(const uint32_t *status, int batch, int *order, const unsigned char *keys, hipStream_t stream);
// row f3: f_ff[batch][12] from forces[batch][12 h] and rBody[batch][9]
hipError_t launch_body_wrench(const float *forces, int batch, int h, const double *rBody, double *f_ff, hipStream_t stream);
// ... and tau[n][10] (f_ff optional) of the first n rows of `forces`; rBody and the joint angles from rBody[n][9], leg_q[n][10], or
// (ticks != nullptr) from the tick structs
hipError_t launch_leg_torques(const float *forces, int n, int h, const double *rBody, const double *leg_q, double *f_ff, double *tau,
                              const hmpc_tick_inputs *ticks, hipStream_t stream);

}  // namespace hmpc
#pragma GCC visibility pop
