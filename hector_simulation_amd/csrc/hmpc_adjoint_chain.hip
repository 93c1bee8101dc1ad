// hmpc_adjoint_chain.hip -- the model, limit and record gradients of the solve under several seeds (hmpc_adjoint_chain_multi, DESIGN.md
// section 4.21): for every seed of the multi-seed adjoint that stands, slice s of every output bit for bit what hmpc_model_adjoint.hip,
// hmpc_limit_adjoint.hip and hmpc_pose_adjoint.hip leave behind hmpc_select_adjoint_seed(s) -- with the record load, the assembly, the
// forward chain, the tracking costate, the active set, the admitted normals and lambda formed once per tile of seeds.
//
// A launch of its own behind hmpc_solve_adjoint_multi (never part of hmpc_kernel, not a row of hmpc_variants.h).  Like its neighbours
// it assembles by CALLING the solve kernel's own stage function -- stage_a_scalars of hmpc_kernel.h, behind the record load of A0, over
// the smallest Smem that serves (NC, HMAX).  Everything behind the assembly is adjoint_chain_of_instance of hmpc_adjoint_chain.h.
// Mapping: one workgroup of 128 threads per instance and tile; a tile is 6 NC seeds (the multi-seed adjoint's), worked off in sub-tiles
// of as many seeds as static LDS below 64 KB holds beside the shared part (chain_sub_tile).  The passes' arrays and the seeds' overlay
// the assembly's Smem, which is dead once the first phase has widened what the passes read.
// Traffic per instance and tile of ns seeds: the record and 6 NC h floats in, once; per seed 2 x 6 NC h + 13 + 12 h + 12 + 6 NC doubles in
// and NF + 12 h + 9 (1 + NC) + 3 + 4 + 3 + NC + 3 doubles out, plus the detail arrays asked for.  No atomics, no inline assembly, no
// matrix cores, nothing kept between launches.
#include <hip/hip_runtime.h>

#include "hmpc_kernel.h"
#include "hmpc_adjoint_chain.h"

namespace hmpc {
namespace {

// the smallest Smem stage_a_scalars can be instantiated over (as hmpc_adjoint.hip)
template <int HMAX, int NC>
using CadjSmem = Smem<12, HMAX, CADJ_NT, 1, NC, 1>;

template <int HMAX, int NC, int SUB>
struct CadjLds {
  union {
    CadjSmem<HMAX, NC> S;           // the assembly, and the first phase of adjoint_chain_of_instance
    ChainWork<NC, HMAX, SUB> Wk;    // the passes and the sub-tile's seeds
  } o;
  ChainKeep<NC, HMAX> Kp;
  float u[6 * NC * HMAX];  // the instance's slot of the force buffer
  float cap[4];            // Fz cap of each contact
  float R[12];             // quat_to_R of the record's quaternion
};

// seeds per sub-tile: as many as fit below 64 KB of static LDS, a whole tile at the most
template <int HMAX, int NC, int SUB = 6 * NC>
constexpr int chain_sub_tile() {
  if constexpr (SUB > 1 && sizeof(CadjLds<HMAX, NC, SUB>) > 64 * 1024) return chain_sub_tile<HMAX, NC, SUB - 1>();
  else return SUB;
}

// seeds s0 .. s0 + ns - 1 of the launch's n_seeds; in and out point at slice 0
template <int HMAX, int NC>
__global__ __launch_bounds__(CADJ_NT) void hmpc_adjoint_chain_kernel(KernelArgs args, double act_tol, double mass, AdjointChainIn in, int s0, int ns,
                                                                     AdjointChainOut out) {
  using RL = RecLayout<NC>;
  constexpr int U = 6 * NC, NT = CADJ_NT, SUB = chain_sub_tile<HMAX, NC>();
  __shared__ CadjLds<HMAX, NC, SUB> L;
  static_assert(sizeof(CadjLds<HMAX, NC, SUB>) <= 64 * 1024, "static LDS of one workgroup");
  auto &S = L.o.S;
  const int tid = threadIdx.x, inst = blockIdx.x, h = args.horizon;
  if (inst >= args.batch || h > HMAX || args.stride > (int)sizeof(S.u.a.rec) || ns < 1 || ns > U) return;  // uniform
  {
    // stage A0 as hmpc_kernel has it: the record, one coalesced burst into LDS (restated as in hmpc_predict.hip, for the reason given there)
    const uint32_t *src = reinterpret_cast<const uint32_t *>(args.records + (size_t)inst * (size_t)args.stride);
    const int nwords = args.stride >> 2;
    for (int t = tid; t < nwords; t += NT) S.u.a.rec[t] = src[t];
  }
  for (int t = tid; t < U * h; t += NT) L.u[t] = args.forces[(size_t)inst * U * h + t];
  __syncthreads();
  Prof prof;
  stage_a_scalars<12, HMAX, NT, 1, NC, 1>(S, args, inst, h, prof);  // (ends with a barrier)
  const auto &A = S.u.a;
  const float *rf = reinterpret_cast<const float *>(A.rec);
  const unsigned char *gait = reinterpret_cast<const unsigned char *>(A.rec + RL::NF + 12 * h);
  if (tid < NC) L.cap[tid] = (NC == 3 && tid == 2) ? rf[RL::FMH] : args.f_max;
  if (tid == NT - 1) {  // the body rotation, as stage A2 forms it
    float R[9], Rt[9];
    quat_to_R(rf + RL::Q, R, Rt);
#pragma unroll
    for (int k = 0; k < 9; ++k) L.R[k] = R[k];
  }
  __syncthreads();
  const size_t i = (size_t)inst, nb = (size_t)args.batch, hz = (size_t)h, s = (size_t)s0 * nb;
  const size_t nrec = (size_t)RL::NF + 12 * hz, nls = (size_t)10 * NC * hz;
  auto at = [&](double *p, const size_t row) -> double * { return p ? p + (s + i) * row : nullptr; };
  const ChainIo io = {in.seeds + (s + i) * hz * U,     in.dir + (s + i) * hz * U,      in.grad_x0 + (s + i) * 13,
                      in.grad_traj + (s + i) * hz * 12, in.grad_weights + (s + i) * 12, in.grad_alpha + (s + i) * U,
                      at(out.grad_record, nrec),       at(out.grad_frames, 9 * (1 + NC)), at(out.grad_rpy, 3),
                      at(out.grad_params, MADJ_PARAMS), at(out.grad_limits, 3 + NC),   at(out.limit_summary, LADJ_SUMMARY),
                      at(out.grad_A, 169),             at(out.grad_B, 13 * U),         at(out.grad_r, 3 * NC),
                      at(out.costate, MADJ_COSTATE),   at(out.grad_Fc, 8 * NC * U),    at(out.grad_bound, nls),
                      at(out.lambda, nls),             at(out.nu, nls),                nb};
  adjoint_chain_of_instance<NC, HMAX, NT, SUB>(A.x0, A.Acd, A.Bcd, A.W, rf + RL::NF, rf + RL::AL, A.Fc, L.u, gait, L.cap, rf, &A.sc[0][0],
                                               &A.sc234[0][0], A.ypsc, L.R, io, ns, h, act_tol, (double)args.dt, mass, (double)args.lt,
                                               (double)args.lh, (double)args.Ib[0], (double)args.Ib[1], (double)args.Ib[2], L.Kp, L.o.Wk);
}

}  // namespace

hipError_t launch_adjoint_chain(int nc, const KernelArgs &args, double act_tol, double mass, const AdjointChainIn &in, int n_seeds,
                                const AdjointChainOut &out, hipStream_t stream) {
  if (args.batch < 1 || args.horizon < 1 || n_seeds < 1 || !in.seeds || !in.dir || !in.grad_x0 || !in.grad_traj || !in.grad_weights ||
      !in.grad_alpha || !out.grad_record || !out.grad_frames || !out.grad_rpy || !out.grad_params || !out.grad_limits || !out.limit_summary ||
      !args.forces || !args.records)
    return hipErrorInvalidValue;
  const int shape = (nc == 2 && args.horizon <= 10) ? 0 : (nc == 2 && args.horizon <= 20) ? 1 : (nc == 3 && args.horizon <= 10) ? 2 : -1;
  if (shape < 0) return hipErrorInvalidValue;
  const dim3 grid(args.batch), block(CADJ_NT);
  const int tile = 6 * nc;
  for (int s0 = 0; s0 < n_seeds; s0 += tile) {
    const int ns = (n_seeds - s0 < tile) ? n_seeds - s0 : tile;
    if (shape == 0) hipLaunchKernelGGL((hmpc_adjoint_chain_kernel<10, 2>), grid, block, 0, stream, args, act_tol, mass, in, s0, ns, out);
    else if (shape == 1) hipLaunchKernelGGL((hmpc_adjoint_chain_kernel<20, 2>), grid, block, 0, stream, args, act_tol, mass, in, s0, ns, out);
    else hipLaunchKernelGGL((hmpc_adjoint_chain_kernel<10, 3>), grid, block, 0, stream, args, act_tol, mass, in, s0, ns, out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace hmpc
