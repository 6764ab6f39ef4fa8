/*
 * aslr_to_amd_sens.h -- extension of the C ABI (aslr_to_amd.h): cost sensitivities of the batch by an adjoint sweep.
 *
 * A header of its own, exported from the same libaslr_to_hip.so: the set of functions aslr_to_amd.h declares, the structs
 * aslr_sizeof knows and ASLR_ABI_VERSION are what existing bindings check against, and this entry point changes none of
 * them (plain pointers, no new struct).  A binding that wants it declares it next to the base set;
 * one that does not is unaffected.  Conventions and the error contract are those of aslr_to_amd.h.
 *
 * The reference (spykspeigel/aslr_to) is built around choosing the stiffness of a soft actuator; its scripts compare
 * designs by solving one problem per value (examples/two_dof_sea.py:50-51).  With per-trajectory parameters
 * (aslr_set_trajectory_params) that comparison is one batched solve; this call adds the gradient of every trajectory's
 * cost in its own parameters, and in its initial state.
 */
#ifndef ASLR_TO_AMD_SENS_H
#define ASLR_TO_AMD_SENS_H

#include "aslr_to_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* For trajectory b with states xs, controls us (XS, US of the handle) and parameters theta = (diag K, diag B) -- its column
 * of the parameter table if one is set, the models' constants otherwise:
 *   J(theta, x0) = sum_t cost_t(x_t, u_t) + cost_T(x_T),   x_{t+1} = f_t(x_t, u_t; theta),   us held fixed.
 * Runs the calcDiff sweep on (XS, US) as aslr_calc_diff does (writes XNEXT, COST, DERIV), then one backward recursion per
 * trajectory:   lambda_T = Lx_T,   lambda_t = Lx_t + Fx_t^T lambda_{t+1};
 *   dJ/dx0 = lambda_0,   dJ/dtheta_j = sum_{t<T} lambda_{t+1}^T df_t/dtheta_j.
 * No cost term depends on theta (CostModelStiffness reads u).  With models that differ in K or B and no table, the
 * derivative is with respect to a common shift of that entry in every model.
 * Exact for any candidate whose gaps are zero (xs[t+1] = xnext[t]): every rolled-out candidate and every solved, feasible
 * trajectory.  At a converged solution, box-constrained ones included, it is also the derivative of the OPTIMAL cost
 * (envelope theorem; the box does not depend on theta), up to a term of first order in the stationarity residual
 * Lu + Fu^T lambda that the solve left: solve tightly first.  With non-zero gaps it is the gradient of the linearisation about
 * the stored (xs, us).
 * Outputs are DEVICE pointers, each optional (NULL: not computed, nothing written), rows [row][B] like TRAJ_PARAMS:
 *   dcost_dstiffness     [nj][B]  dJ/dK_j.  SEA only: a VSA model takes its stiffness from u (ASLR_E_INVALID);
 *   dcost_dmotor_inertia [nj][B]  dJ/dB_j (with respect to B_j itself, not its reciprocal);
 *   dcost_dx0            [nx][B]  lambda_0;
 *   costate              [T+1][B][nx]  lambda_t, time-major like the workspace.
 * Honours the parameter table, a reference path (through the calcDiff sweep) and padded controls.  Covers the whole shard
 * on the caller's stream (sub-shards do not apply); enqueues only, like aslr_calc_diff.  Side effects: those of
 * aslr_calc_diff.
 * ASLR_E_INVALID (aslr_last_error starts with "aslr_cost_sensitivity:"): a NULL handle; all four outputs NULL;
 * dcost_dstiffness on a VSA model; K or B of a model that is not diagonal; a stiffness entry equal to 0 in the models or
 * in the table (SEA: the stiffness term divides by it). */
int aslr_cost_sensitivity(aslr_problem_t *p,
                          double *dcost_dstiffness,
                          double *dcost_dmotor_inertia,
                          double *dcost_dx0,
                          double *costate,
                          void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ASLR_TO_AMD_SENS_H */
