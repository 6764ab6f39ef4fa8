// forward pass (rollout + trial costs + line search) for nj = 7 with VSA actuation (nx = 28, nu = 14), in a translation
// unit of its own so that it compiles next to aslr_forward_nj7.hip instead of after it.  SolverBoxDDP is the one solver
// built for this size (aslr_abi.hip, solver_unsupported): the rollout carries no FDDP gap terms.
#include "aslr_forward.inc.hpp"
#include "aslr_forward_team.inc.hpp"

namespace aslr {
int launch_forward_nj7_vsa(const KArgs &k, const SolverDev &sd, const ModelLimits &lim, hipStream_t st) {
  const int nb = k.b1 - k.b0; // trajectories of this launch
  dim3 block(64), cgrid((nb + 63) / 64, k.T + 1, ASLR_NALPHA), sgrid((nb + 63) / 64), ugrid((nb + 63) / 64, ASLR_NALPHA);
  // one block of 16 eight-lane teams per trajectory (aslr_forward_team.inc.hpp)
  hipLaunchKernelGGL((rollout_team_kernel<7, false, ASLR_DAM_VSA>), dim3(nb), dim3(128), 0, st, k, sd, lim);
  hipLaunchKernelGGL((trial_cost_kernel<7, ASLR_DAM_VSA, false>), cgrid, block, 0, st, k, sd);
  hipLaunchKernelGGL((sum_cost_kernel<14>), ugrid, block, 0, st, k, sd);
  hipLaunchKernelGGL((select_kernel<14>), sgrid, block, 0, st, k, sd);
  HIP_TRY(hipGetLastError());
  return ASLR_OK;
}
} // namespace aslr
