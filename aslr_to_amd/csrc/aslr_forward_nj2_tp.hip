// forward pass for nj = 2 with a per-trajectory parameter table: TP = true rollouts (the trial costs, their sums and the
// line search do not read the table: the same kernels as in aslr_forward_nj2.hip)
#include "aslr_forward.inc.hpp"

namespace aslr {
template decltype(launch_forward<2, ASLR_DAM_SEA, true>) launch_forward<2, ASLR_DAM_SEA, true>;
template decltype(launch_forward<2, ASLR_DAM_VSA, true>) launch_forward<2, ASLR_DAM_VSA, true>;
} // namespace aslr
