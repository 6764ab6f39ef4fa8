/*
 * aslr_to_amd_policy.h -- extension of the C ABI (aslr_to_amd.h): closed-loop roll-outs of the stored policy on a
 * perturbed plant, many samples per trajectory.
 *
 * A header of its own, exported from the same libaslr_to_hip.so, for the reason aslr_to_amd_sens.h gives: the set of
 * functions aslr_to_amd.h declares, the structs aslr_sizeof knows and ASLR_ABI_VERSION are what existing bindings check
 * against, and this entry point changes none of them (plain pointers, no new struct).  A binding that wants it declares it
 * next to the base set; one that does not is unaffected.  Conventions and the error contract are those of
 * aslr_to_amd.h.
 *
 * A solve leaves a policy on the device: XS, US and KGAIN hold u_t = us_t - K_t (x_t - xs_t).  The reference
 * (spykspeigel/aslr_to) computes that policy for soft actuators; what its users ask next is how it holds up when the real
 * arm differs from the model -- a spring that is 20 % off, another motor inertia, a wrong initial state, a push during the
 * motion.  This call answers that for S samples of every trajectory of the batch at once.
 */
#ifndef ASLR_TO_AMD_POLICY_H
#define ASLR_TO_AMD_POLICY_H

#include "aslr_to_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Sample s (0 <= s < n_samples = S) of trajectory b rolls the handle's policy out on its own plant:
 *   x_0 = X0[b] + dx0[s][b];
 *   for t < T:  u_t = us_t - K_t (x_t - xs_t)   with XS, US and KGAIN of the handle (KFF is not used);
 *               if clamp != 0 and the knot's model has control limits, u_t is clamped to the box -- the trajectory's row of the
 *               parameter table when one is set (aslr_set_trajectory_params), else the model's;
 *               x_{t+1} = f_t(x_t, u_t; plant) + disturbance[s][t][b]   (the convention of aslr_mpc_run's disturbance);
 *   cost = sum_{t<T} cost_t(x_t, u_t) + cost_T(x_T)   with the handle's cost stack, the applied (clamped) control and, while
 *               a reference path is set, its row min(row0 + t, last); node costs are added in knot order.
 * f_t is the knot's action model with the diagonals of K and B replaced by the plant's where given; a NULL plant argument
 * means the trajectory's own value: its row of the parameter table if one is set, else the model's constant.
 * failed_knot is the first t whose xnext = f_t(x_t, u_t) fails the solver's test (NaN, Inf or an entry >= 1e30 in absolute
 * value), or -1; for a failed sample the cost is NaN and the trajectory past that knot is unspecified.
 *
 * All pointers are DEVICE pointers.  Inputs, each optional:
 *   plant_stiffness      [nj][S][B]    diag K of the plant.  SEA only: a VSA model takes its stiffness from u;
 *   plant_motor_inertia  [nj][S][B]    diag B of the plant (B itself, not its reciprocal).  A device array, so a
 *                                      non-positive entry is NOT checked: it shows up in failed_knot;
 *   dx0                  [S][B][nx];
 *   disturbance          [S][T][B][nx].
 * Outputs, each optional (NULL: nothing written), at least one given:
 *   cost [S][B],  failed_knot [S][B] (int32),  x_final [S][B][nx],  xs_closed [S][T+1][B][nx],  us_closed [S][T][B][nu].
 * With every input NULL the roll-out of a gap-free candidate and the gains of its own backward sweep returns that
 * candidate, bit for bit.  A handle that has never run a backward sweep has K = 0: the roll-out is then open loop.
 *
 * Nothing in the workspace is written (XS_TRY, TRAJ_F, TRAJ_I and the DONE flags included): a solve continued after the
 * call gives the bits it gives without it.  Covers the whole shard on the caller's stream (sub-shards do not apply);
 * enqueues only.
 * ASLR_E_INVALID (aslr_last_error starts with "aslr_policy_rollout:"; nothing is written): a NULL handle; n_samples <= 0 (or
 * above 16 * 65535); all outputs NULL; plant_stiffness on a VSA model; a plant argument while K or B of a model is not
 * diagonal; a 7-joint handle (the kernel is built for the nx = 8 sizes: two_dof_sea, two_dof_vsa*, double_pendulum,
 * double_pendulum_nu1, planar and general 3-D chains). */
int aslr_policy_rollout(aslr_problem_t *p, int n_samples,
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
#endif /* ASLR_TO_AMD_POLICY_H */
