// adjoint sweep (aslr_cost_sensitivity): adjoint_kernel for the four sizes
#include "aslr_adjoint.inc.hpp"

namespace aslr {
template decltype(launch_adjoint<2, ASLR_DAM_SEA>) launch_adjoint<2, ASLR_DAM_SEA>;
template decltype(launch_adjoint<2, ASLR_DAM_VSA>) launch_adjoint<2, ASLR_DAM_VSA>;
template decltype(launch_adjoint<7, ASLR_DAM_SEA>) launch_adjoint<7, ASLR_DAM_SEA>;
template decltype(launch_adjoint<7, ASLR_DAM_VSA>) launch_adjoint<7, ASLR_DAM_VSA>;
} // namespace aslr
