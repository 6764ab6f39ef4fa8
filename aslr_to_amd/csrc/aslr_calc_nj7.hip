// calc / calcDiff kernels instantiated for nj = 7 (SEA; the frame placements serve both actuations)
#include "aslr_calc.inc.hpp"
#include "aslr_calc_team.inc.hpp"

namespace aslr {
template decltype(launch_calc<7, ASLR_DAM_SEA>) launch_calc<7, ASLR_DAM_SEA>;
template decltype(launch_dam_eval<7, ASLR_DAM_SEA>) launch_dam_eval<7, ASLR_DAM_SEA>;
template decltype(launch_dam_residuals<7, ASLR_DAM_SEA>) launch_dam_residuals<7, ASLR_DAM_SEA>;
template decltype(launch_frame_placement<7>) launch_frame_placement<7>;
template decltype(launch_quasi_static<7, ASLR_DAM_SEA>) launch_quasi_static<7, ASLR_DAM_SEA>;
} // namespace aslr
