// tangent sweep (aslr_policy_plant_sensitivity): plant_sens_kernel for the four record shapes in use
#include "aslr_plant_sens.inc.hpp"
