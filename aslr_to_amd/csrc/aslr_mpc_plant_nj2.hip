// the plant phase of aslr_mpc_run_plant: mpc_plant_kernel for nj = 2 (nx = 8; SEA and VSA, planar and 3-D chains)
#include "aslr_mpc_plant.inc.hpp"

namespace aslr {
template decltype(launch_mpc_plant<2, ASLR_DAM_SEA>) launch_mpc_plant<2, ASLR_DAM_SEA>;
template decltype(launch_mpc_plant<2, ASLR_DAM_VSA>) launch_mpc_plant<2, ASLR_DAM_VSA>;
} // namespace aslr
