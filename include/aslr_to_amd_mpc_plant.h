/*
 * aslr_to_amd_mpc_plant.h -- extension of the C ABI (aslr_to_amd.h): receding-horizon runs on a plant whose parameters
 * differ from the model's, re-planning every `hold` knots and tracking with the Riccati gains in between.
 *
 * A header of its own, exported from the same libaslr_to_hip.so, for the reason aslr_to_amd_sens.h gives: the set of
 * functions aslr_to_amd.h declares, the structs aslr_sizeof knows and ASLR_ABI_VERSION are what existing bindings check
 * against, and this entry point changes none of them (aslr_mpc_t is reused as it is, no new struct, no new workspace
 * region).  A binding that wants it declares it next to the base set; one that does not is unaffected.
 * Conventions and the error contract are those of aslr_to_amd.h.
 *
 * aslr_policy_rollout says how ONE stored policy holds up on an arm whose spring stiffness and motor inertia differ from the
 * model; aslr_mpc_run re-plans every knot, but on the model itself.  This call answers what lies between: does re-planning
 * rescue a mismatched arm, and how often must it re-plan?  The batch axis is the sample axis: replicate a problem B times
 * and give each copy its own plant.
 */
#ifndef ASLR_TO_AMD_MPC_PLANT_H
#define ASLR_TO_AMD_MPC_PLANT_H

#include "aslr_to_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* aslr_mpc_run with a plant of its own and a hold.  `mpc` is read as aslr_mpc_run reads it, but with N = n_steps * hold the
 * rows of three of its arrays count APPLIED KNOTS:  disturbance [N][B][nx],  x_closed [N+1][B][nx],  u_closed [N][B][nu];
 * stat_f and stat_i stay per control step.  All pointers are DEVICE pointers; disturbance, x_closed and u_closed are read and
 * written as 16-byte pieces, so these three must be 16-byte aligned (any allocator's buffer is; an offset into one must keep it).
 *
 * Control step s (0 <= s < n_steps):
 *  1. the solve of aslr_mpc_run's step 1 (first_maxiter iterations at s = 0, iters_per_step after, then the finalize; sub-
 *     shards apply), its statistics into stat_*[s];
 *  2. the plant phase, from x = XS[0]: for j = 0 .. hold-1, with k = s hold + j,
 *       u = US[0] for j = 0 (x is XS[0] itself: no feedback term is formed),  u = US[j] - KGAIN[j] (x - XS[j]) for j >= 1;
 *       if clamp != 0 and the running model has control limits, u is clamped to the box -- the trajectory's row of the
 *       parameter table when one is set (aslr_set_trajectory_params), else the model's;
 *       x_closed[k] = x,  u_closed[k] = u,  c_k = cost(x, u) with the running model's cost stack (with a reference path:
 *       against row min(row0 + k, last));
 *       x <- f(x, u; plant) + disturbance[k]   (no addition when disturbance is NULL).
 *     f is node 0's action model with the diagonals of K and B replaced by the plant's where given; a NULL plant argument
 *     means the trajectory's own value: its row of the parameter table if one is set, else the model's constant;
 *  3. the shift by hold: xs[t] <- xs[min(t + hold, T)] (t < T), us[t] <- us[min(t + hold, T - 1)] (t < T - 1), xs[0] <- x and
 *     X0 <- x; GAPS, VXXF and KFF are zeroed.  With a reference path the window advances hold rows per control step; the
 *     handle's row (aslr_reference_row) has grown by N afterwards.
 * After the last step x_closed[N] = x.
 *
 *   plant_stiffness      [nj][B]  diag K of the plant, or NULL.  SEA only: a VSA model takes its stiffness from u;
 *   plant_motor_inertia  [nj][B]  diag B of the plant (B itself, not its reciprocal), or NULL.  A device array, so a
 *                                 non-positive entry is NOT checked: it shows up in failed_knot;
 *   closed_cost [B]      sum_k c_k, added in knot order across the control steps; no terminal term; NaN for a trajectory that
 *                        failed; or NULL;
 *   failed_knot [B]      (int32) the first k whose plant state f(x, u; plant) fails the solver's test (NaN, Inf or an entry >=
 *                        1e30 in absolute value), else -1; or NULL.  The run goes on after a failure, as aslr_mpc_run does; what
 *                        follows the failure is unspecified.
 *
 * With hold == 1, both plant arguments, closed_cost and failed_knot NULL and clamp == 0 the call IS aslr_mpc_run: the same
 * launches, the same bits.  Enqueues only; at most two launches between two solves and no host wait, as aslr_mpc_run.
 * ASLR_E_INVALID (aslr_last_error starts with "aslr_mpc_run_plant:"; nothing is enqueued, the handle stays usable): everything
 * aslr_mpc_run refuses; hold < 1 or hold > T; plant_stiffness on a VSA model; a plant argument while K or B of a model is not
 * diagonal; a 7-joint handle (the plant kernel is built for the nx = 8 sizes, as aslr_policy_rollout's: two_dof_sea,
 * two_dof_vsa*, double_pendulum, double_pendulum_nu1, planar and general 3-D chains; aslr_mpc_run serves the 7-joint arms). */
int aslr_mpc_run_plant(aslr_problem_t *p, const aslr_solver_params_t *sp, const aslr_mpc_t *mpc,
                       int hold,
                       const double *plant_stiffness,
                       const double *plant_motor_inertia,
                       int clamp,
                       double *closed_cost,
                       int32_t *failed_knot,
                       void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ASLR_TO_AMD_MPC_PLANT_H */
