// forward pass (rollout + trial costs + line search) instantiated for nj = 7
#include "aslr_forward.inc.hpp"
#include "aslr_forward_team.inc.hpp"

namespace aslr {
template decltype(launch_forward<7, ASLR_DAM_SEA>) launch_forward<7, ASLR_DAM_SEA>;
} // namespace aslr

#ifdef ASLR_BWD_PROFILE
extern "C" int aslr_debug_fwd_prof7(unsigned long long *out32, int reset) { return aslr::prof_table(out32, reset); } // tools/fwd_regions_c5.py
#endif
