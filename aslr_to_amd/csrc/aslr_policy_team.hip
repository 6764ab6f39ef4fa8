// closed-loop policy roll-outs (aslr_policy_rollout_all): policy_rollout_team_kernel for nj = 7 (nx = 28; SEA and VSA)
#include "aslr_policy_team.inc.hpp"

namespace aslr {
int launch_policy_rollout_team(int nj, int dam, const KArgs &k, const ModelLimits &lim, const PolicyArgs &pa, hipStream_t st) {
  return launch_policy_rollout_team_as("aslr_policy_rollout_all", nj, dam, k, lim, pa, st);
}
} // namespace aslr
