/*
 * aslr_to_amd_cov.h -- extension of the C ABI (aslr_to_amd.h): first-order closed-loop covariance of the stored policy.
 *
 * A header of its own, exported from the same libaslr_to_hip.so: the set of functions aslr_to_amd.h declares, the structs
 * aslr_sizeof knows and ASLR_ABI_VERSION are what existing bindings check against, and this entry point changes none of
 * them (plain pointers, no new struct).  A binding that wants it declares it next to the base set;
 * one that does not is unaffected.  Conventions and the error contract are those of aslr_to_amd.h.
 *
 * aslr_policy_rollout (aslr_to_amd_policy.h) answers "what does the policy do away from its nominal trajectory" by
 * sampling, for the 2-joint models.  This call answers it to first order without samples and without a model evaluation,
 * from the records of one calcDiff sweep, for every model size: the spread of the state and of the control under the
 * Riccati feedback, and what that spread costs in the solver's own quadratic model.
 */
#ifndef ASLR_TO_AMD_COV_H
#define ASLR_TO_AMD_COV_H

#include "aslr_to_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* For trajectory b with states xs, controls us and gains K (XS, US and KGAIN of the handle), under the policy of
 * aslr_policy_rollout, u_t = us_t - K_t (x_t - xs_t):
 * runs the calcDiff sweep on (XS, US) as aslr_cost_sensitivity does (writes XNEXT, COST, DERIV), then one forward recursion
 * per trajectory on the records:
 *   A_t = Fx_t - Fu_t K_t,   Sigma_{t+1} = A_t Sigma_t A_t^T + diag(noise_var[t]),   U_t = K_t Sigma_t K_t^T      (t < T)
 *   cost_increase = 1/2 sum_{t<T} [tr(Lxx_t Sigma_t) - 2 tr(Lxu_t K_t Sigma_t) + tr(Luu_t U_t)] + 1/2 tr(Lxx_T Sigma_T),
 * the terms added in knot order.  Noise t enters x_{t+1}, the convention of the disturbance arguments of
 * aslr_policy_rollout.  KGAIN is used as the handle holds it: KFF is not read, and a handle without a backward sweep has
 * K = 0 (the open-loop covariance).  The control box is not applied: this is a linearisation, and a BoxDDP solve already
 * carries zero gain rows for its clamped controls.
 * Inputs are DEVICE pointers, each nullable (NULL: zero):
 *   sigma0     [B][nx][nx]   Sigma_0, symmetric: only the entries [i][j] with i >= j are read, and they are mirrored;
 *   noise_var  [T][B][nx]    variances of the process noise, time-major like the workspace.
 * Outputs are DEVICE pointers, each optional (NULL: not computed, nothing written), time-major like the workspace:
 *   x_var          [T+1][B][nx]      diagonal of Sigma_t;
 *   u_var          [T][B][nu]        diagonal of U_t (padded controls have zero gain rows and variance 0);
 *   cov_final      [B][nx][nx]       Sigma_T;
 *   cov            [T+1][B][nx][nx]  every Sigma_t (the layout of VXX);
 *   cost_increase  [B].
 * Row j of a stored Sigma_t is computed as row j of (A Sigma) A^T and taken as column j of the next knot; the two triangles
 * of an output agree to rounding, not bit for bit.  The results of a trajectory do not depend on B or on its place in the
 * batch, and an output has the same bits whichever others are asked for.
 * Honours the parameter table, a reference path and padded controls, all through the calcDiff sweep.  Covers the whole
 * shard on the caller's stream (sub-shards do not apply); enqueues only, like aslr_calc_diff.  Side effects: those of
 * aslr_calc_diff.
 * ASLR_E_INVALID (aslr_last_error starts with "aslr_policy_covariance:"; nothing is written and the handle stays live):
 * a NULL handle; all five outputs NULL; sigma0 and noise_var both NULL (nothing to propagate); a record shape (nx, nu)
 * for which no kernel is built (built: (8, 2), (8, 4), (28, 7), (28, 14): every size a handle can have today). */
int aslr_policy_covariance(aslr_problem_t *p,
                           const double *sigma0,
                           const double *noise_var,
                           double *x_var,
                           double *u_var,
                           double *cov_final,
                           double *cov,
                           double *cost_increase,
                           void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ASLR_TO_AMD_COV_H */
