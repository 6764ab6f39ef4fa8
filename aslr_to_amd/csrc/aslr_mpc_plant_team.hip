// the plant phase of aslr_mpc_run_plant_all: mpc_plant_team_kernel for nj = 7 (nx = 28; SEA and VSA)
#include "aslr_mpc_plant_team.inc.hpp"

namespace aslr {
template decltype(launch_mpc_plant_team<7, ASLR_DAM_SEA>) launch_mpc_plant_team<7, ASLR_DAM_SEA>;
template decltype(launch_mpc_plant_team<7, ASLR_DAM_VSA>) launch_mpc_plant_team<7, ASLR_DAM_VSA>;
} // namespace aslr
