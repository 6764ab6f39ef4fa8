// backward pass for nx = 8 with a per-trajectory parameter table (TP = true: the control box of a boxed node is the
// trajectory's own row, aslr_set_trajectory_params)
#include "aslr_backward.inc.hpp"

namespace aslr {
template decltype(launch_backward<2, ASLR_DAM_SEA, true>) launch_backward<2, ASLR_DAM_SEA, true>;
template decltype(launch_backward<2, ASLR_DAM_VSA, true>) launch_backward<2, ASLR_DAM_VSA, true>;
} // namespace aslr
