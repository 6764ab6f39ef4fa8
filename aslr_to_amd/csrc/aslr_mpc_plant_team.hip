// the plant phase of aslr_mpc_run_plant_all: mpc_plant_team_kernel for nj = 7 (nx = 28; SEA and VSA)
#include "aslr_mpc_plant_team.inc.hpp"
