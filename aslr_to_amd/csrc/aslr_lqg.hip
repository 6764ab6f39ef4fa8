// output-feedback covariance sweep (aslr_policy_lqg): lqg_kernel for the four sizes
#include "aslr_lqg.inc.hpp"

namespace aslr {
template decltype(launch_lqg<2, ASLR_DAM_SEA>) launch_lqg<2, ASLR_DAM_SEA>;
template decltype(launch_lqg<2, ASLR_DAM_VSA>) launch_lqg<2, ASLR_DAM_VSA>;
template decltype(launch_lqg<7, ASLR_DAM_SEA>) launch_lqg<7, ASLR_DAM_SEA>;
template decltype(launch_lqg<7, ASLR_DAM_VSA>) launch_lqg<7, ASLR_DAM_VSA>;
} // namespace aslr
