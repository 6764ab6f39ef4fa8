/*
 * aslr_to_amd_policy_all.h -- extension of the C ABI (aslr_to_amd.h): closed-loop roll-outs of the stored policy on a
 * perturbed plant for every model size, the 7-joint arms included.
 *
 * A header of its own, exported from the same libaslr_to_hip.so, for the reason aslr_to_amd_sens.h gives: the set of
 * functions aslr_to_amd.h declares, the structs aslr_sizeof knows and ASLR_ABI_VERSION are what existing bindings check
 * against, and this entry point changes none of them (plain pointers, no new struct).  aslr_policy_rollout
 * (aslr_to_amd_policy.h) keeps its behaviour, its refusal of 7-joint handles included; a binding that wants one call for
 * all sizes declares this one next to the base set; one that does not is unaffected.  Conventions and
 * the error contract are those of aslr_to_amd.h.
 *
 * aslr_policy_covariance and aslr_policy_plant_sensitivity predict, to first order, how a policy's states, controls and
 * cost spread and move when the plant is not the model, for every model size.  This call is the nonlinear closed loop those
 * predictions are checked against, on talos_arm_sea and talos_arm_vsa as on the 2-joint models.
 */
#ifndef ASLR_TO_AMD_POLICY_ALL_H
#define ASLR_TO_AMD_POLICY_ALL_H

#include "aslr_to_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The definition is that of aslr_policy_rollout (aslr_to_amd_policy.h), word for word.  Sample s (0 <= s < n_samples = S)
 * of trajectory b rolls the handle's policy out on its own plant:
 *   x_0 = X0[b] + dx0[s][b];
 *   for t < T:  u_t = us_t - K_t (x_t - xs_t)   with XS, US and KGAIN of the handle (KFF is not used);
 *               if clamp != 0 and the knot's model has control limits, u_t is clamped to the box -- the trajectory's row of the
 *               parameter table when one is set (aslr_set_trajectory_params), else the model's;
 *               x_{t+1} = f_t(x_t, u_t; plant) + disturbance[s][t][b]   (added only when the pointer is given);
 *   cost = sum_{t<T} cost_t(x_t, u_t) + cost_T(x_T)   with the handle's cost stack, the applied (clamped) control and, while
 *               a reference path is set, its row min(row0 + t, last); node costs are added in knot order.
 * f_t is the knot's action model with the diagonals of K and B replaced by the plant's where given; a NULL plant argument
 * means the trajectory's own value: its row of the parameter table if one is set, else the model's constant (the full
 * matrix: a model whose K or B is not diagonal rolls out as long as no plant argument is given).
 * failed_knot is the first t whose xnext = f_t(x_t, u_t) fails the solver's test (NaN, Inf or an entry >= 1e30 in absolute
 * value), or -1; for a failed sample the cost is NaN and the trajectory past that knot is unspecified.
 *
 * All pointers are DEVICE pointers, 16-byte aligned.  Inputs, each optional:
 *   plant_stiffness      [nj][S][B]    diag K of the plant.  SEA only: a VSA model takes its stiffness from u;
 *   plant_motor_inertia  [nj][S][B]    diag B of the plant (B itself, not its reciprocal).  A device array, so a
 *                                      non-positive entry is NOT checked: it shows up in failed_knot;
 *   dx0                  [S][B][nx];
 *   disturbance          [S][T][B][nx].
 * Outputs, each optional (NULL: nothing written), at least one given:
 *   cost [S][B],  failed_knot [S][B] (int32),  x_final [S][B][nx],  xs_closed [S][T+1][B][nx],  us_closed [S][T][B][nu].
 *
 * Sizes: every handle the solver entry points accept.  nj = 7 (nx = 28; SEA with nu = 7, VSA with nu = 14) runs
 * policy_rollout_team_kernel, a team of 8 lanes per (trajectory, sample); its outputs are held to the definition within
 * rounding (1e-9 in max |a - b| / (1 + |b|) in the test suite), not to the bits of another kernel.  nj = 2 is forwarded to the
 * kernel of aslr_policy_rollout and returns that call's bits.
 *
 * Nothing in the workspace is written (XS_TRY, TRAJ_F, TRAJ_I and the DONE flags included): a solve continued after the
 * call gives the bits it gives without it.  Covers the whole shard on the caller's stream (sub-shards do not apply);
 * enqueues only.
 * ASLR_E_INVALID (aslr_last_error starts with "aslr_policy_rollout_all:"; nothing is written): a NULL handle; n_samples <= 0
 * (or above 16 * 65535); all outputs NULL; plant_stiffness on a VSA model; a plant argument while K or B of a model is not
 * diagonal. */
int aslr_policy_rollout_all(aslr_problem_t *p, int n_samples,
                            const double *plant_stiffness,
                            const double *plant_motor_inertia,
                            const double *dx0,
                            const double *disturbance,
                            int clamp,
                            double *cost,
                            int32_t *failed_knot,
                            double *x_final,
                            double *xs_closed,
                            double *us_closed,
                            void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ASLR_TO_AMD_POLICY_ALL_H */
