// hmpc_adjoint_chain.hip -- the model, limit and record gradients of the solve under several seeds (hmpc_adjoint_chain_multi, DESIGN.md
// section 4.21): for every seed of the multi-seed adjoint that stands, slice s of every output bit for bit what hmpc_model_adjoint.hip,
// hmpc_limit_adjoint.hip and hmpc_pose_adjoint.hip leave behind hmpc_select_adjoint_seed(s) -- with the record load, the assembly, the
// forward chain, the tracking costate, the active set, the admitted normals and lambda formed once per tile of seeds.
//
// A launch of its own behind hmpc_solve_adjoint_multi (never part of hmpc_kernel, not a row of hmpc_variants.h).  Like its neighbours it
// assembles by CALLING the solve kernel's own stage function -- the common front of hmpc_derived.h.  Everything behind the assembly is
// adjoint_chain_of_instance of hmpc_adjoint_chain.h.
// Mapping: one workgroup of 128 threads per instance and tile; a tile is 6 NC seeds (the multi-seed adjoint's), worked off in sub-tiles
// of as many seeds as static LDS below 64 KB holds beside the shared part (chain_sub_tile).  The passes' arrays and the seeds' overlay
// the assembly's Smem, which is dead once the first phase has widened what the passes read.
// Traffic per instance and tile of ns seeds: the record and 6 NC h floats in, once; per seed 2 x 6 NC h + 13 + 12 h + 12 + 6 NC doubles in
// and NF + 12 h + 9 (1 + NC) + 3 + 4 + 3 + NC + 3 doubles out, plus the detail arrays asked for.  No atomics, no inline assembly, no
// matrix cores, nothing kept between launches.
#include <hip/hip_runtime.h>

#include "hmpc_derived.h"
#include "hmpc_adjoint_chain.h"

namespace hmpc {
namespace {

template <int HMAX, int NC, int SUB>
struct CadjLds {
  union {
    DerivedSmem<HMAX, NC> S;        // the assembly, and the first phase of adjoint_chain_of_instance
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
__global__ __launch_bounds__(DERIVED_NT) void hmpc_adjoint_chain_kernel(KernelArgs args, double act_tol, double mass, AdjointChainIn in, int s0, int ns,
                                                                          AdjointChainOut out) {
  using RL = RecLayout<NC>;
  constexpr int U = 6 * NC, NT = DERIVED_NT, SUB = chain_sub_tile<HMAX, NC>();
  __shared__ CadjLds<HMAX, NC, SUB> L;
  static_assert(sizeof(CadjLds<HMAX, NC, SUB>) <= 64 * 1024, "static LDS of one workgroup");
  auto &S = L.o.S;
  const int inst = blockIdx.x, h = args.horizon;
  if (ns < 1 || ns > U) return;  // uniform
  if (!derived_front(S, L.u, args)) return;  // uniform
  const auto &A = S.u.a;
  const float *rf = derived_record_floats(S);
  const unsigned char *gait = derived_gait(S, h);
  derived_fill_caps(S, args, L.cap);
  derived_fill_rotation(S, L.R);
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
  const dim3 grid(args.batch), block(DERIVED_NT);
  return for_derived_seed_tiles(nc, args.horizon, n_seeds, [&](auto H, auto C, int s0, int ns) {
    hipLaunchKernelGGL((hmpc_adjoint_chain_kernel<H(), C()>), grid, block, 0, stream, args, act_tol, mass, in, s0, ns, out);
  });
}

}  // namespace hmpc
