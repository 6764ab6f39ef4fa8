// nj = 7, VSA, with a per-trajectory parameter table: the TP = true calc / calcDiff sweeps and quasi-static controls
#include "aslr_calc.inc.hpp"

namespace aslr {
template decltype(launch_calc<7, ASLR_DAM_VSA, true>) launch_calc<7, ASLR_DAM_VSA, true>;
template decltype(launch_quasi_static<7, ASLR_DAM_VSA, true>) launch_quasi_static<7, ASLR_DAM_VSA, true>;
} // namespace aslr
