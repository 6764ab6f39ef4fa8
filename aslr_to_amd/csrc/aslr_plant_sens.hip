// tangent sweep (aslr_policy_plant_sensitivity): plant_sens_kernel for the four sizes
#include "aslr_plant_sens.inc.hpp"

namespace aslr {
template decltype(launch_plant_sens<2, ASLR_DAM_SEA>) launch_plant_sens<2, ASLR_DAM_SEA>;
template decltype(launch_plant_sens<2, ASLR_DAM_VSA>) launch_plant_sens<2, ASLR_DAM_VSA>;
template decltype(launch_plant_sens<7, ASLR_DAM_SEA>) launch_plant_sens<7, ASLR_DAM_SEA>;
template decltype(launch_plant_sens<7, ASLR_DAM_VSA>) launch_plant_sens<7, ASLR_DAM_VSA>;
} // namespace aslr
