// forward pass for nj = 7, SEA, with a per-trajectory parameter table: TP = true team rollout
#include "aslr_forward.inc.hpp"
#include "aslr_forward_team.inc.hpp"

namespace aslr {
template decltype(launch_forward<7, ASLR_DAM_SEA, true>) launch_forward<7, ASLR_DAM_SEA, true>;
} // namespace aslr
