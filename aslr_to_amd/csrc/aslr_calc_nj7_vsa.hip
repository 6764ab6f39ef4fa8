// nj = 7 with VSA actuation (nx = 28, nu = 14): calc / calcDiff sweeps, dam_eval, dam_residuals, quasi-static controls
// in a translation unit of their own, so that they compile next to aslr_calc_nj7.hip instead of after it
#include "aslr_calc.inc.hpp"

namespace aslr {
template decltype(launch_calc<7, ASLR_DAM_VSA>) launch_calc<7, ASLR_DAM_VSA>;
template decltype(launch_dam_eval<7, ASLR_DAM_VSA>) launch_dam_eval<7, ASLR_DAM_VSA>;
template decltype(launch_dam_residuals<7, ASLR_DAM_VSA>) launch_dam_residuals<7, ASLR_DAM_VSA>;
template decltype(launch_quasi_static<7, ASLR_DAM_VSA>) launch_quasi_static<7, ASLR_DAM_VSA>;
} // namespace aslr
