// closed-loop policy roll-outs that draw their perturbations (aslr_policy_rollout_noise): policy_rollout_team_kernel with
// PolicyNoiseArgs for nj = 7 (nx = 28; SEA and VSA) -- a unit of its own so that the build stays parallel
#include "aslr_policy_team.inc.hpp"

namespace aslr {
template decltype(launch_policy_rollout_team<7, ASLR_DAM_SEA, PolicyNoiseArgs>) launch_policy_rollout_team<7, ASLR_DAM_SEA, PolicyNoiseArgs>;
template decltype(launch_policy_rollout_team<7, ASLR_DAM_VSA, PolicyNoiseArgs>) launch_policy_rollout_team<7, ASLR_DAM_VSA, PolicyNoiseArgs>;
} // namespace aslr
