// forward pass for nj = 7, VSA (SolverBoxDDP), with a per-trajectory parameter table: TP = true team rollout
#include "aslr_forward.inc.hpp"
#include "aslr_forward_team.inc.hpp"

namespace aslr {
template decltype(launch_forward<7, ASLR_DAM_VSA, true>) launch_forward<7, ASLR_DAM_VSA, true>;
} // namespace aslr
