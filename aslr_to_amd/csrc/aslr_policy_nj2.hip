// closed-loop policy roll-outs (aslr_policy_rollout): policy_rollout_kernel for nj = 2 (nx = 8; SEA and VSA, planar and 3-D chains)
#include "aslr_policy.inc.hpp"

namespace aslr {
template decltype(launch_policy_rollout<2, ASLR_DAM_SEA, PolicyArgs>) launch_policy_rollout<2, ASLR_DAM_SEA, PolicyArgs>;
template decltype(launch_policy_rollout<2, ASLR_DAM_VSA, PolicyArgs>) launch_policy_rollout<2, ASLR_DAM_VSA, PolicyArgs>;
} // namespace aslr
