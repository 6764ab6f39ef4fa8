/*
 * aslr_to_amd_plant_sens.h -- extension of the C ABI (aslr_to_amd.h): first-order closed-loop sensitivity of the stored
 * policy to the plant's spring stiffness and motor inertia.
 *
 * A header of its own, exported from the same libaslr_to_hip.so: the set of functions aslr_to_amd.h declares, the structs
 * aslr_sizeof knows and ASLR_ABI_VERSION are what existing bindings check against, and this entry point changes none of
 * them (plain pointers, no new struct).  A binding that wants it declares it next to the base set;
 * one that does not is unaffected.  Conventions and the error contract are those of aslr_to_amd.h.
 *
 * aslr_policy_rollout (aslr_to_amd_policy.h) samples perturbed plants, for the 2-joint models.  aslr_policy_covariance
 * (aslr_to_amd_cov.h) serves every size but knows state noise only.  aslr_cost_sensitivity (aslr_to_amd_sens.h)
 * differentiates in the plant's parameters with the controls held fixed.  This call is the forward (tangent) counterpart of
 * that adjoint sweep with the feedback gains acting: where the closed loop ends up on an arm whose springs or motors are
 * not the model's, how much control the feedback spends on it, and what it costs -- for every model size.
 */
#ifndef ASLR_TO_AMD_PLANT_SENS_H
#define ASLR_TO_AMD_PLANT_SENS_H

#include "aslr_to_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* For trajectory b with states xs, controls us and gains K (XS, US and KGAIN of the handle), the plant runs under the
 * policy of aslr_policy_rollout without the clamp, u_t = us_t - K_t (x_t - xs_t).  Its parameters theta = (diag K, diag B)
 * are the trajectory's own (its column of the parameter table, else the constants of the knot's action model, exactly as
 * aslr_cost_sensitivity takes them) plus a small error.  Runs the calcDiff sweep on (XS, US) as aslr_policy_covariance does
 * (writes XNEXT, COST, DERIV), then one forward recursion per trajectory on the records, to first order about (XS, US):
 *   S_0 = 0,   V_t = K_t S_t,   S_{t+1} = (Fx_t - Fu_t K_t) S_t + G_t      (t < T;   S_t = dx_t/dtheta,   du_t/dtheta = -V_t)
 *   G_K[:, j] = -(delta_j / K_j) (Fx_t[:, nj+j] - e_{nj+j}),   delta_j = xs_t[j] - xs_t[nj+j]
 *   G_B[:, j] = -(1 / B_j) D_j (dt e_{nj+j} + e_{3nj+j}),      D_j = xnext_t[3nj+j] - xs_t[3nj+j]
 *   dJ/dtheta_p = sum_{t<T} (Lx_t^T S_t[:, p] - Lu_t^T V_t[:, p]) + Lx_T^T S_T[:, p],   the terms added in knot order
 *   x_var_t[i] = sum_p S_t[i][p]^2 var_p,   u_var_t[k] = sum_p V_t[k][p]^2 var_p
 * (the state is (q_l, q_m, v_l, v_m); independent parameter errors of variance var_p).  KGAIN is used as the handle holds
 * it: a handle without a backward sweep has K = 0, which gives the open loop, where dJ/dtheta is what
 * aslr_cost_sensitivity returns.  The control box is not applied.
 * Inputs are DEVICE pointers, each nullable (NULL: zero variance):
 *   stiffness_var, motor_inertia_var   [nj][B]   variances of the errors of diag K and diag B.
 * Outputs are DEVICE pointers, each optional (NULL: not computed, nothing written), time-major like the workspace:
 *   dx_dstiffness, dx_dmotor_inertia        [T+1][B][nx][nj]   S_t, the columns of each kind;
 *   dxT_dstiffness, dxT_dmotor_inertia      [B][nx][nj]        S_T;
 *   dcost_dstiffness, dcost_dmotor_inertia  [nj][B]            (the layout of aslr_cost_sensitivity);
 *   x_var  [T+1][B][nx];   u_var  [T][B][nu]   (a padded control has a zero gain row and variance 0).
 * Columns of S never mix: the stiffness columns are computed only when a stiffness argument asks for them, and an output
 * has the same bits whichever others are asked for.  The results of a trajectory do not depend on B or on its place in the
 * batch.  Honours the parameter table, a reference path and padded controls.  Covers the whole shard on the caller's stream
 * (sub-shards do not apply); enqueues only, like aslr_calc_diff.  Side effects: those of aslr_calc_diff.
 * ASLR_E_INVALID (aslr_last_error starts with "aslr_policy_plant_sensitivity:"; nothing is written and the handle stays
 * live): a NULL handle; all eight outputs NULL; any stiffness argument, input or output, on a VSA model, whose stiffness is
 * a control; x_var or u_var with both variance inputs NULL; K or B of a model not diagonal; a motor inertia entry equal to
 * 0; a stiffness entry equal to 0 (in the models, or in the table while one is set) when a stiffness quantity is asked
 * for; a record shape (nx, nu) other than (8, 2), (8, 4), (28, 7), (28, 14): every size a handle can have today. */
int aslr_policy_plant_sensitivity(aslr_problem_t *p,
                                  const double *stiffness_var,
                                  const double *motor_inertia_var,
                                  double *dx_dstiffness,
                                  double *dx_dmotor_inertia,
                                  double *dxT_dstiffness,
                                  double *dxT_dmotor_inertia,
                                  double *dcost_dstiffness,
                                  double *dcost_dmotor_inertia,
                                  double *x_var,
                                  double *u_var,
                                  void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ASLR_TO_AMD_PLANT_SENS_H */
