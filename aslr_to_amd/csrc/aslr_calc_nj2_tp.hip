// nj = 2 with a per-trajectory parameter table (aslr_set_trajectory_params): the TP = true calc / calcDiff sweeps and
// quasi-static controls, in a translation unit of their own -- aslr_calc_nj2.hip compiles to what it did without them
#include "aslr_calc.inc.hpp"

namespace aslr {
template decltype(launch_calc<2, ASLR_DAM_SEA, true>) launch_calc<2, ASLR_DAM_SEA, true>;
template decltype(launch_calc<2, ASLR_DAM_VSA, true>) launch_calc<2, ASLR_DAM_VSA, true>;
template decltype(launch_quasi_static<2, ASLR_DAM_SEA, true>) launch_quasi_static<2, ASLR_DAM_SEA, true>;
template decltype(launch_quasi_static<2, ASLR_DAM_VSA, true>) launch_quasi_static<2, ASLR_DAM_VSA, true>;
} // namespace aslr
