// hmpc_front.hip -- front_scalars_kernel: stages A1 and A2 of the assembly (hmpc_front.h) for a whole two-contact batch in one launch
// ahead of the fast solve kernels, which read the result (struct FrontScalars, one block per instance) instead of running the serial
// binary64 chains on a lane or two of their own 256.
//
// Mapping: FRONT_LANES = 16 lanes per instance, the roles of stage A1 -- 0..9 a joint angle each, 10 / 11 q2+q3+q4 of a leg, 12 / 13 / 14
// roll / pitch / yaw, 15 the gait bytes -- and FRONT_IPW = 16 instances per workgroup of 256 threads.  The roles of one wave share their
// code where the functions allow it: ONE det_atan2 serves the three Euler lanes (the others ride along on atan2(0, 1)), then ONE
// det_sincos serves the twelve joint roles and pitch and yaw.  A1 hands sines and cosines to A2 through LDS; in A2 role 0 is the body,
// roles 1 and 2 a foot each.  The blocks are staged in LDS and leave as one coalesced burst per workgroup.
// Instances are indexed 0 .. batch-1 directly (the dispatch order only permutes which workgroup of the solve reads which block).  A
// group beyond the batch computes the batch's last instance again into its own LDS slot and stores nothing: no early return before a
// barrier, no read or write out of bounds.
#include "hmpc_front.h"

namespace hmpc {

__global__ __launch_bounds__(FRONT_NT) void front_scalars_kernel(const FrontArgs a, FrontScalars *out) {
  using RL = RecLayout<2>;
  struct Trig {
    float sc[10][2], sc234[2][2], ypsc[4];
  };
  __shared__ Trig trig[FRONT_IPW];
  __shared__ FrontScalars blk[FRONT_IPW];
  const int tid = threadIdx.x, slot = tid / FRONT_LANES, role = tid % FRONT_LANES;
  const int first = (int)blockIdx.x * FRONT_IPW;
  const int inst = (first + slot < a.batch) ? first + slot : a.batch - 1;
  const int h = a.horizon;
  const float *rf = reinterpret_cast<const float *>(a.records + (size_t)inst * a.stride);
  const unsigned char *gait = reinterpret_cast<const unsigned char *>(rf + RL::NF + 12 * h);
  const float *in_q = rf + RL::Q, *in_r = rf + RL::R, *in_ja = rf + RL::JA;
  Trig &T = trig[slot];
  FrontScalars &B = blk[slot];
  // ---------------- A1
  {
    double y = 0.0, x = 1.0;
    if (role == 12) front_euler_args<0>(in_q, y, x);
    else if (role == 13) front_euler_args<1>(in_q, y, x);
    else if (role == 14) front_euler_args<2>(in_q, y, x);
    float ang = (float)det_atan2(y, x);
    if (role < 12) ang = front_trig_angle(in_ja, role);
    double s, c;
    det_sincos((double)ang, s, c);
    if (role < 10) {
      T.sc[role][0] = (float)s, T.sc[role][1] = (float)c;
    } else if (role < 12) {
      T.sc234[role - 10][0] = (float)s, T.sc234[role - 10][1] = (float)c;
    } else if (role == 12) {
      B.rpy[0] = ang;
    } else if (role == 13) {
      B.rpy[1] = ang, T.ypsc[2] = (float)c, T.ypsc[3] = (float)s;
    } else if (role == 14) {
      B.rpy[2] = ang, T.ypsc[0] = (float)c, T.ypsc[1] = (float)s;
    } else {
      const float f_max = a.f_max;
      int nv, nl;
      front_prefix<2>(gait, h, [f_max](int) { return f_max; }, B.pre_nl, B.pre_nv, B.pre_st, nv, nl);
      for (int i = h; i < FRONT_STEPS; ++i) B.pre_nl[i] = 0, B.pre_nv[i] = 0, B.pre_st[i] = 0;
      B.n = (unsigned short)nv, B.nls = (unsigned short)nl;
      B.pad0 = 0.0f;
    }
  }
  __syncthreads();
  // ---------------- A2
  if (role == 0) {
    front_body<2>(in_q, T.ypsc, in_r, a.Ib, a.dt, B.Rbi_dt, B.Iinv_dt, B.blk_dt);
  } else if (role == 1 || role == 2) {
    float *f = B.foot[role - 1];
    front_foot<2>(in_q, T.sc, T.sc234, role - 1, a.lt, a.lh, nullptr, f, f + 3, f + 6, f + 9);
  }
  __syncthreads();
  // the workgroup's live blocks, one coalesced burst
  {
    const int live = (a.batch - first < FRONT_IPW) ? a.batch - first : FRONT_IPW;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(blk);
    uint32_t *dst = reinterpret_cast<uint32_t *>(out + first);
    for (int t = tid; t < live * FRONT_WORDS; t += FRONT_NT) dst[t] = src[t];
  }
}

hipError_t launch_front_scalars(const FrontArgs &a, FrontScalars *out, hipStream_t stream) {
  if (a.batch < 1) return hipSuccess;
  hipLaunchKernelGGL(front_scalars_kernel, dim3((a.batch + FRONT_IPW - 1) / FRONT_IPW), dim3(FRONT_NT), 0, stream, a, out);
  return hipGetLastError();
}

}  // namespace hmpc
