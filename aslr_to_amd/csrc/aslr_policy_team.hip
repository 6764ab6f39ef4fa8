// closed-loop policy roll-outs (aslr_policy_rollout_all): policy_rollout_team_kernel for nj = 7 (nx = 28; SEA and VSA)
#include "aslr_policy_team.inc.hpp"
