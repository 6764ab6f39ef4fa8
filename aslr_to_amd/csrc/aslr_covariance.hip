// closed-loop covariance sweep (aslr_policy_covariance): covariance_kernel for the four sizes
#include "aslr_covariance.inc.hpp"

namespace aslr {
template decltype(launch_covariance<2, ASLR_DAM_SEA>) launch_covariance<2, ASLR_DAM_SEA>;
template decltype(launch_covariance<2, ASLR_DAM_VSA>) launch_covariance<2, ASLR_DAM_VSA>;
template decltype(launch_covariance<7, ASLR_DAM_SEA>) launch_covariance<7, ASLR_DAM_SEA>;
template decltype(launch_covariance<7, ASLR_DAM_VSA>) launch_covariance<7, ASLR_DAM_VSA>;
} // namespace aslr
