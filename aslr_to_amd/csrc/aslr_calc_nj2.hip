// calc / calcDiff kernels instantiated for nj = 2 (3-D and planar chain paths)
#include "aslr_calc.inc.hpp"

namespace aslr {
template decltype(launch_calc<2, ASLR_DAM_SEA>) launch_calc<2, ASLR_DAM_SEA>;
template decltype(launch_calc<2, ASLR_DAM_VSA>) launch_calc<2, ASLR_DAM_VSA>;
template decltype(launch_dam_eval<2, ASLR_DAM_SEA>) launch_dam_eval<2, ASLR_DAM_SEA>;
template decltype(launch_dam_eval<2, ASLR_DAM_VSA>) launch_dam_eval<2, ASLR_DAM_VSA>;
template decltype(launch_dam_residuals<2, ASLR_DAM_SEA>) launch_dam_residuals<2, ASLR_DAM_SEA>;
template decltype(launch_dam_residuals<2, ASLR_DAM_VSA>) launch_dam_residuals<2, ASLR_DAM_VSA>;
template decltype(launch_frame_placement<2>) launch_frame_placement<2>;
template decltype(launch_quasi_static<2, ASLR_DAM_SEA>) launch_quasi_static<2, ASLR_DAM_SEA>;
template decltype(launch_quasi_static<2, ASLR_DAM_VSA>) launch_quasi_static<2, ASLR_DAM_VSA>;
} // namespace aslr

#ifdef ASLR_BWD_PROFILE
extern "C" int aslr_debug_calc_prof(unsigned long long *out32, int reset) { return aslr::prof_table(out32, reset); } // tools/calc_regions.py
#endif
