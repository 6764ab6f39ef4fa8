// forward pass (rollout + trial costs + line search) instantiated for nj = 2
#include "aslr_forward.inc.hpp"

namespace aslr {
template decltype(launch_forward<2, ASLR_DAM_SEA>) launch_forward<2, ASLR_DAM_SEA>;
template decltype(launch_forward<2, ASLR_DAM_VSA>) launch_forward<2, ASLR_DAM_VSA>;
} // namespace aslr
