// closed-loop policy roll-outs that draw their perturbations (aslr_policy_rollout_noise): policy_rollout_team_kernel with
// PolicyNoiseArgs for nj = 7 (nx = 28; SEA and VSA) -- a unit of its own so that the build stays parallel
#include "aslr_policy_team.inc.hpp"

namespace aslr {
int launch_policy_rollout_noise_team(int nj, int dam, const KArgs &k, const ModelLimits &lim, const PolicyNoiseArgs &pa, hipStream_t st) {
  return launch_policy_rollout_team_as("aslr_policy_rollout_noise", nj, dam, k, lim, pa, st);
}
} // namespace aslr
