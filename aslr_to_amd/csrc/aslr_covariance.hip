// closed-loop covariance sweep (aslr_policy_covariance): covariance_kernel for the four record shapes in use
#include "aslr_covariance.inc.hpp"
