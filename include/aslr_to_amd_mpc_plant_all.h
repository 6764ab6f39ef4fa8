/*
 * aslr_to_amd_mpc_plant_all.h -- extension of the C ABI (aslr_to_amd.h): receding-horizon runs on a mismatched plant
 * (aslr_to_amd_mpc_plant.h) for every model size, the 7-joint arms included.
 *
 * A header of its own, exported from the same libaslr_to_hip.so, for the reason aslr_to_amd_sens.h gives: the set of
 * functions the other headers declare, the structs aslr_sizeof knows and ASLR_ABI_VERSION are what existing bindings check
 * against, and this entry point changes none of them (aslr_mpc_t is reused as it is, no new struct, no new workspace
 * region).  A binding that wants it declares it next to the base set; one that does not is unaffected.
 * Conventions and the error contract are those of aslr_to_amd.h.
 *
 * aslr_mpc_run_plant is built for the nx = 8 sizes and refuses a 7-joint handle; that refusal is part of what its callers
 * check against and stays.  The arms are where the question it answers is asked in earnest -- does re-planning rescue a
 * 7-joint arm whose springs and motors are 20 % off, and how often must it re-plan? -- so this twin takes the same ten
 * arguments and serves every handle the solver entry points serve.
 */
#ifndef ASLR_TO_AMD_MPC_PLANT_ALL_H
#define ASLR_TO_AMD_MPC_PLANT_ALL_H

#include "aslr_to_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The arguments, layouts and definition are those of the function aslr_to_amd_mpc_plant.h declares, word for word: control
 * steps 1 - 3 there, plants [nj][B], N = n_steps * hold applied knots in disturbance [N][B][nx], x_closed [N+1][B][nx] and
 * u_closed [N][B][nu], stat_f and stat_i per control step, closed_cost [B] and failed_knot [B] as defined there; the same
 * alignment of disturbance and x_closed (16 bytes).  What differs:
 *
 *  - it serves every handle the solver entry points serve.  A 2-joint handle runs exactly the launches of that function:
 *    the same bits.  talos_arm_sea and talos_arm_vsa (nj = 7, nx = 28, nu = 7 / 14) run the plant phase as a team of 8
 *    lanes per trajectory, between the same solve and the same shift by hold;
 *  - on a 7-joint handle a model whose K or B is not diagonal still runs while no plant argument is given and no parameter
 *    table is set: the plant is then the model's full rows;
 *  - on a 7-joint handle with hold == 1, both plant arguments, closed_cost and failed_knot NULL and clamp == 0 the call IS
 *    aslr_mpc_run, as it is there on a 2-joint one: the same launches, the same bits.
 *
 * Enqueues only; at most two launches between two solves and no host wait.
 * ASLR_E_INVALID (aslr_last_error starts with "aslr_mpc_run_plant_all:"; nothing is enqueued, the handle stays usable):
 * everything aslr_mpc_run refuses (a 7-joint VSA handle with a solver other than SolverBoxDDP among it); hold < 1 or
 * hold > T; plant_stiffness on a VSA model; a plant argument while K or B of a model is not diagonal; n_steps * hold, or the
 * reference row after them, beyond INT32_MAX. */
int aslr_mpc_run_plant_all(aslr_problem_t *p, const aslr_solver_params_t *sp, const aslr_mpc_t *mpc,
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
#endif /* ASLR_TO_AMD_MPC_PLANT_ALL_H */
