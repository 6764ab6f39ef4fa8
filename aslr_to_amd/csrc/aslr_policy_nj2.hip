// closed-loop policy roll-outs (aslr_policy_rollout): policy_rollout_kernel for nj = 2 (nx = 8; SEA and VSA, planar and 3-D chains)
#include "aslr_policy.inc.hpp"

namespace aslr {
int launch_policy_rollout(int nj, int dam, const KArgs &k, const ModelLimits &lim, const PolicyArgs &pa, hipStream_t st) {
  return launch_policy_rollout_as("aslr_policy_rollout", nj, dam, k, lim, pa, st);
}
} // namespace aslr
