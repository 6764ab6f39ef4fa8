// closed-loop policy roll-outs that draw their perturbations (aslr_policy_rollout_noise): policy_rollout_kernel with
// PolicyNoiseArgs for nj = 2 (nx = 8; SEA and VSA, planar and 3-D chains) -- a unit of its own so that the build stays parallel
#include "aslr_policy.inc.hpp"

namespace aslr {
int launch_policy_rollout_noise(int nj, int dam, const KArgs &k, const ModelLimits &lim, const PolicyNoiseArgs &pa, hipStream_t st) {
  return launch_policy_rollout_as("aslr_policy_rollout_noise", nj, dam, k, lim, pa, st);
}
} // namespace aslr
