// closed-loop policy roll-outs that draw their perturbations (aslr_policy_rollout_noise): policy_rollout_kernel with
// PolicyNoiseArgs for nj = 2 (nx = 8; SEA and VSA, planar and 3-D chains) -- a unit of its own so that the build stays parallel
#include "aslr_policy.inc.hpp"

namespace aslr {
template decltype(launch_policy_rollout<2, ASLR_DAM_SEA, PolicyNoiseArgs>) launch_policy_rollout<2, ASLR_DAM_SEA, PolicyNoiseArgs>;
template decltype(launch_policy_rollout<2, ASLR_DAM_VSA, PolicyNoiseArgs>) launch_policy_rollout<2, ASLR_DAM_VSA, PolicyNoiseArgs>;
} // namespace aslr
