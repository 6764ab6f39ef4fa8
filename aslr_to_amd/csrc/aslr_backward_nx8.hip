// backward pass instantiated for nx = 8 (2-DoF SEA nu = 2, 2-DoF VSA nu = 4)
#include "aslr_backward.inc.hpp"

namespace aslr {
template decltype(launch_backward<2, ASLR_DAM_SEA>) launch_backward<2, ASLR_DAM_SEA>;
template decltype(launch_backward<2, ASLR_DAM_VSA>) launch_backward<2, ASLR_DAM_VSA>;
} // namespace aslr

#ifdef ASLR_BWD_PROFILE
extern "C" int aslr_debug_bwd_prof(unsigned long long *out32, int reset) { return aslr::prof_table(out32, reset); } // tools/bwd_regions.py
#endif
