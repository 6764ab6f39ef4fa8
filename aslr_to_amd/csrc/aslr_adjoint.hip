// adjoint sweep (aslr_cost_sensitivity): adjoint_kernel for the four record shapes in use
#include "aslr_adjoint.inc.hpp"
