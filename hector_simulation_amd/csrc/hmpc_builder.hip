// hmpc_builder.hip -- the unit that compiles the kernels of hmpc_builder.h (record builder, size classes, dispatch order, body wrenches,
// joint torques) and launches them (hmpc_builder_launch.h).
#include "hmpc_builder.h"
#include "hmpc_builder_launch.h"

namespace hmpc {

static constexpr int NT = 256;  // one thread per item
static dim3 grid_for(int items) { return dim3((items + NT - 1) / NT); }

hipError_t launch_build_records(const hmpc_tick_inputs *ticks, int batch, int h, double dtMPC, unsigned char *records, int stride,
                                double *wpd_out, float f_max, unsigned char *cls, hipStream_t stream) {
  if (batch < 1) return hipSuccess;
  const int nwords = stride / 4;  // one workgroup per instance, a thread per 32-bit word of the record
  const int bs = ((nwords + 63) / 64) * 64 > 256 ? 256 : ((nwords + 63) / 64) * 64;
  hipLaunchKernelGGL(build_records_kernel, dim3(batch), dim3(bs), 0, stream, ticks, batch, h, dtMPC, records, stride, wpd_out, f_max, cls);
  return hipGetLastError();
}

hipError_t launch_classify_records(const unsigned char *records, int stride, int batch, int h, float f_max, unsigned char *cls,
                                   hipStream_t stream) {
  if (batch < 1) return hipSuccess;
  hipLaunchKernelGGL(classify_records_kernel, grid_for(batch), dim3(NT), 0, stream, records, stride, batch, h, f_max, cls);
  return hipGetLastError();
}

hipError_t launch_predicted_cost(const unsigned char *records, int stride, int batch, int h, int nc, unsigned char *keys, hipStream_t stream) {
  if (batch < 1) return hipSuccess;
  hipLaunchKernelGGL(predicted_cost_kernel, grid_for(batch), dim3(NT), 0, stream, records, stride, batch, h, nc, keys);
  return hipGetLastError();
}

hipError_t launch_dispatch_order(const uint32_t *status, int batch, int *order, const unsigned char *keys, hipStream_t stream) {
  if (batch < 1) return hipSuccess;
  hipLaunchKernelGGL(dispatch_order_kernel, dim3(1), dim3(1024), 0, stream, status, batch, order, keys);
  return hipGetLastError();
}

hipError_t launch_body_wrench(const float *forces, int batch, int h, const double *rBody, double *f_ff, hipStream_t stream) {
  if (batch < 1) return hipSuccess;
  hipLaunchKernelGGL(body_wrench_kernel, grid_for(12 * batch), dim3(NT), 0, stream, forces, batch, h, rBody, f_ff);
  return hipGetLastError();
}

hipError_t launch_leg_torques(const float *forces, int n, int h, const double *rBody, const double *leg_q, double *f_ff, double *tau,
                              const hmpc_tick_inputs *ticks, hipStream_t stream) {
  if (n < 1) return hipSuccess;
  hipLaunchKernelGGL(leg_torque_kernel, grid_for(2 * n), dim3(NT), 0, stream, forces, n, h, rBody, leg_q, f_ff, tau, ticks);
  return hipGetLastError();
}

}  // namespace hmpc
