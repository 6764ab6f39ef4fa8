// plant identification (aslr_plant_identify): identify_normal_kernel and identify_step_kernel for the four sizes
#include "aslr_identify.inc.hpp"

namespace aslr {
template decltype(launch_identify_normal<2, ASLR_DAM_SEA>) launch_identify_normal<2, ASLR_DAM_SEA>;
template decltype(launch_identify_normal<2, ASLR_DAM_VSA>) launch_identify_normal<2, ASLR_DAM_VSA>;
template decltype(launch_identify_normal<7, ASLR_DAM_SEA>) launch_identify_normal<7, ASLR_DAM_SEA>;
template decltype(launch_identify_normal<7, ASLR_DAM_VSA>) launch_identify_normal<7, ASLR_DAM_VSA>;
template decltype(launch_identify_step<2, ASLR_DAM_SEA>) launch_identify_step<2, ASLR_DAM_SEA>;
template decltype(launch_identify_step<2, ASLR_DAM_VSA>) launch_identify_step<2, ASLR_DAM_VSA>;
template decltype(launch_identify_step<7, ASLR_DAM_SEA>) launch_identify_step<7, ASLR_DAM_SEA>;
template decltype(launch_identify_step<7, ASLR_DAM_VSA>) launch_identify_step<7, ASLR_DAM_VSA>;
} // namespace aslr
