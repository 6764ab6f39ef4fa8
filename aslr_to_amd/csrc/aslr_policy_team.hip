// closed-loop policy roll-outs (aslr_policy_rollout_all): policy_rollout_team_kernel for nj = 7 (nx = 28; SEA and VSA)
#include "aslr_policy_team.inc.hpp"

namespace aslr {
template decltype(launch_policy_rollout_team<7, ASLR_DAM_SEA, PolicyArgs>) launch_policy_rollout_team<7, ASLR_DAM_SEA, PolicyArgs>;
template decltype(launch_policy_rollout_team<7, ASLR_DAM_VSA, PolicyArgs>) launch_policy_rollout_team<7, ASLR_DAM_VSA, PolicyArgs>;
} // namespace aslr
