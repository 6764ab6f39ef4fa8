// forward pass (rollout + trial costs + line search) for nj = 7 with VSA actuation (nx = 28, nu = 14), in a translation
// unit of its own so that it compiles next to aslr_forward_nj7.hip instead of after it.  SolverBoxDDP is the one solver
// built for this size (aslr_abi.hip, solver_unsupported): the rollout carries no FDDP gap terms.
#include "aslr_forward.inc.hpp"
#include "aslr_forward_team.inc.hpp"

namespace aslr {
template decltype(launch_forward<7, ASLR_DAM_VSA>) launch_forward<7, ASLR_DAM_VSA>;
} // namespace aslr
