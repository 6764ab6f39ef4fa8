// the two sweeps of aslr_state_smooth: smooth_filter_kernel and smooth_adjoint_kernel for the four sizes
#include "aslr_smooth.inc.hpp"

namespace aslr {
template decltype(launch_smooth_filter<2, ASLR_DAM_SEA>) launch_smooth_filter<2, ASLR_DAM_SEA>;
template decltype(launch_smooth_filter<2, ASLR_DAM_VSA>) launch_smooth_filter<2, ASLR_DAM_VSA>;
template decltype(launch_smooth_filter<7, ASLR_DAM_SEA>) launch_smooth_filter<7, ASLR_DAM_SEA>;
template decltype(launch_smooth_filter<7, ASLR_DAM_VSA>) launch_smooth_filter<7, ASLR_DAM_VSA>;
template decltype(launch_smooth_adjoint<2, ASLR_DAM_SEA>) launch_smooth_adjoint<2, ASLR_DAM_SEA>;
template decltype(launch_smooth_adjoint<2, ASLR_DAM_VSA>) launch_smooth_adjoint<2, ASLR_DAM_VSA>;
template decltype(launch_smooth_adjoint<7, ASLR_DAM_SEA>) launch_smooth_adjoint<7, ASLR_DAM_SEA>;
template decltype(launch_smooth_adjoint<7, ASLR_DAM_VSA>) launch_smooth_adjoint<7, ASLR_DAM_VSA>;
} // namespace aslr
