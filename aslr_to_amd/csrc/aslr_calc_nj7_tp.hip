// nj = 7, SEA, with a per-trajectory parameter table: the TP = true calc / calcDiff sweeps (team kernels included) and
// quasi-static controls
#include "aslr_calc.inc.hpp"
#include "aslr_calc_team.inc.hpp"

namespace aslr {
template decltype(launch_calc<7, ASLR_DAM_SEA, true>) launch_calc<7, ASLR_DAM_SEA, true>;
template decltype(launch_quasi_static<7, ASLR_DAM_SEA, true>) launch_quasi_static<7, ASLR_DAM_SEA, true>;
} // namespace aslr
