// backward pass instantiated for nx = 28 (7-DoF arm: SEA, nu = 7; VSA, nu = 14)
#include "aslr_backward_blk.inc.hpp"

namespace aslr {
template decltype(launch_backward<7, ASLR_DAM_SEA>) launch_backward<7, ASLR_DAM_SEA>;
template decltype(launch_backward<7, ASLR_DAM_VSA>) launch_backward<7, ASLR_DAM_VSA>;
} // namespace aslr

#ifdef ASLR_BWD_PROFILE
extern "C" int aslr_debug_bwd_prof28(unsigned long long *out32, int reset) { return aslr::prof_table(out32, reset); } // tools/bwd_regions_c5.py
#endif
