// aslr_sweep_team.hpp -- what the sweeps with one team of lanes per trajectory share: adjoint_kernel, covariance_kernel,
// lqg_kernel, plant_sens_kernel and identify_normal_kernel.  Only what leaves their instruction text as it was; a team's index
// set-up, the loaders and the sums stay written out in each kernel, because shared they changed the schedule of the nx = 28
// instantiations and lqg_kernel ran up to 3.5 % longer (profiles/sweep_team/README.md).
//
// The team: nx = 8: 8 lanes, 8 trajectories per wave; nx = 28: 32 lanes (28 at work), 2 per wave; one wave per block
// (SizeTraits::sweep_blocks).  Every lane of the wave stays alive on clamped indices -- a trajectory past B reads the last
// one's data, an idle lane of a 32-lane team the last row's -- and only the stores, to memory and to LDS, are guarded.  So a
// trajectory's arithmetic is the same instruction stream whatever its position in the batch: its bits do not depend on B.
#pragma once
#include "aslr_common.hpp"

namespace aslr {

// the long sums of these kernels stay loops, two steps per trip (aslr_covariance.inc.hpp says why)
#define ASLR_SWEEP_LOOP _Pragma("unroll 2")

template <int NX> // joints, lanes of a team, teams of a wave
struct SweepTeam { static constexpr int NJ = NX / 4, TEAM = NX == 8 ? 8 : 32, TPW = 64 / TEAM; };

// the action model of knot t, a wave-uniform word read through the constant address space (adjoint_kernel keeps the
// expression: through this function all four of its instantiations came out with other text)
__device__ __forceinline__ int knot_model(const int32_t *node_model, int t) {
  return ((const int32_t __attribute__((address_space(4))) *)(node_model))[t];
}

// one launcher: one wave per block, SizeTraits::sweep_blocks of them
template <int NJ, int DAM, class Args>
int launch_sweep(void (*kernel)(Args), const Args &a, hipStream_t st) {
  hipLaunchKernelGGL(kernel, dim3(SizeTraits<NJ, DAM>::sweep_blocks(a.B)), dim3(64), 0, st, a);
  HIP_TRY(hipGetLastError());
  return ASLR_OK;
}
// ... of the kernel pick(STIFF) gives.  a.stiff: the stiffness columns are wanted.  The STIFF kernels are built for the SEA sizes
// alone: a VSA model takes its stiffness from u and the calls refuse every stiffness argument on one, so a.stiff is 0 there
template <int NJ, int DAM, class Args, class F>
int launch_sweep_stiff(F pick, const Args &a, hipStream_t st) {
  void (*kernel)(Args) = pick(std::false_type{});
  if constexpr (DAM == ASLR_DAM_SEA)
    if (a.stiff) kernel = pick(std::true_type{});
  return launch_sweep<NJ, DAM>(kernel, a, st);
}

} // namespace aslr
