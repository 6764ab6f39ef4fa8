/*
 * aslr_to_amd_design.h -- extension of the C ABI (aslr_to_amd.h): a descent in the spring stiffness and the motor inertia
 * of every trajectory of the batch that stays on the device.
 *
 * A header of its own, exported from the same libaslr_to_hip.so: the set of functions aslr_to_amd.h declares, the structs
 * aslr_sizeof knows (aslr_design_t is read by this call alone and has no index there, like aslr_pool_params_t) and
 * ASLR_ABI_VERSION are what existing bindings check against, and this entry point changes none of them.  A binding that
 * wants it declares it next to the base set; one that does not is unaffected.  Conventions and the error
 * contract are those of aslr_to_amd.h.
 *
 * The reference (spykspeigel/aslr_to) exists to choose the stiffness of a soft actuator; its scripts compare designs by
 * solving one problem per value (examples/two_dof_sea.py:50-51).  aslr_set_trajectory_params makes that one batched solve,
 * aslr_cost_sensitivity (aslr_to_amd_sens.h) adds dJ/dK_j, dJ/dB_j of every design from one more sweep.  This call takes
 * the step: solve, gradient, accept or reject, next design -- n_steps times, every trajectory on its own design, without
 * a host round trip per step (what aslr_mpc_run is to a receding-horizon loop, for a design loop).
 */
#ifndef ASLR_TO_AMD_DESIGN_H
#define ASLR_TO_AMD_DESIGN_H

#include "aslr_to_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* theta = (diag K, diag B) of a trajectory, 2 nj entries, K before B ("rows": [2 nj][B] like TRAJ_PARAMS, entry j of
 * trajectory b at j B + b).  An entry is ACTIVE when its field is optimised (opt_stiffness: the K rows; opt_motor_inertia:
 * the B rows); the others keep their initial value throughout.
 *
 * Initial design theta_0: the handle's parameter table if one is set (aslr_set_trajectory_params), else the models'
 * constants, put in place as aslr_set_trajectory_params does with no field given (the same refusals; the control-box rows
 * come from the models).  Either way the handle is on the kernels that read the table afterwards.
 *
 * Step s = 0 .. n_steps - 1, everything enqueued on `stream`, no host wait between steps:
 *   1. solve at the candidate design in the table: the iterations aslr_solve enqueues when the host never polls
 *      (first_maxiter of them at s = 0, iters_per_step later) from XS / US, then aslr_finalize.  Every step starts like a
 *      solve: regularisation at sp->reg_init, GAPS / VXXF / KFF zero as a fresh problem has them (the step kernel leaves
 *      them so), feasibility sp->is_feasible at s = 0 and 0 later (the plan was made under other parameters).  sp->maxiter
 *      is not read.  Sub-shards (aslr_set_subshards) apply.  The first calcDiff sweep of a step rewrites the model-only
 *      record chunks: they depend on the table.
 *   2. gradient g at the finalized candidate: the two sweeps of aslr_cost_sensitivity, for the active fields.
 *   3. the step, per trajectory.  J = TRAJ_F[ASLR_TF_COST].  Evaluable: J and every active g_j are finite.
 *      Accepted: evaluable and (s = 0, or J <= J_acc + c1 pred, pred = sum_j g_acc_j (theta_try_j - theta_acc_j) over the
 *      active entries in ascending j, K before B).
 *        accepted:  theta_acc <- theta_try, J_acc <- J, g_acc <- g, xs_best / us_best <- XS / US, eta <- eta grow
 *                   (s = 0 included: eta starts at eta0, so the first candidate is a step of eta0 grow);
 *        otherwise: eta <- eta shrink, XS / US <- xs_best / us_best.
 *      A trajectory that is not evaluable at s = 0 is FROZEN: its candidate stays theta_0 in every step, its hist_i -1.
 *      Next candidate, a step in log theta to first order:
 *        dz_j = clamp(-eta (theta_acc_j g_acc_j), -max_rel, max_rel),  theta_try_j = clamp(theta_acc_j (1 + dz_j), lo_j, hi_j),
 *      written into column b of TRAJ_PARAMS: K_j as it is, the motor row 1.0 / B_j by IEEE division (the bits of the host's
 *      row builder); the control-box rows are not touched.  Every product and sum of pred and of the update is rounded on
 *      its own (no fused multiply-add).
 * After the last step the table holds theta_acc (not a further candidate) and XS / US hold xs_best / us_best; the handle's
 * host copy of the table is refreshed by ONE blocking device-to-host copy at the very end, and the handle is then, for
 * every later call, what aslr_set_trajectory_params(theta_acc) followed by that solve would leave.  TRAJ_F / TRAJ_I are
 * those of the LAST step's solve (of a candidate that may have been rejected), not of the accepted design.
 * Host waits: one on entry, before anything else is enqueued -- the bounds live on the device and are read back to be
 * checked, so that a refusal writes nothing -- and one on exit, the copy above (the uploads of the initial table and of
 * theta_0 ride on the stream and are covered by it).  None in between.
 *
 * All pointers are DEVICE pointers owned by the caller, alive until the stream has run the call. */
typedef struct aslr_design {
  int32_t n_steps;            /* outer steps, >= 1                                                              */
  int32_t first_maxiter;      /* iterations of step 0's solve, >= 1                                             */
  int32_t iters_per_step;     /* iterations of the later solves, >= 1                                           */
  int32_t opt_stiffness;      /* != 0: the K rows are optimised (SEA only)                                      */
  int32_t opt_motor_inertia;  /* != 0: the B rows are optimised; at least one of the two                        */
  int32_t _pad0;
  double eta0;                /* initial step length in log theta, > 0                                          */
  double grow;                /* factor on eta after an accepted step, >= 1                                     */
  double shrink;              /* factor on eta after a rejected one, in (0, 1)                                  */
  double c1;                  /* Armijo constant, in (0, 1)                                                     */
  double max_rel;             /* largest relative change of an entry per step, in (0, 1)                        */
  const double *lo, *hi;      /* [2 nj][B] bounds, 0 < lo <= hi, no NaN; rows of a field that is not optimised
                                 are not read                                                                  */
  double *theta_best;         /* [2 nj][B] out: the accepted design, K and B themselves (a VSA model: K rows 0) */
  double *cost_best;          /* [B] out: its cost (a frozen trajectory: the cost of step 0's solve)            */
  double *xs_best;            /* [T+1][B][nx] out: its plan                                                     */
  double *us_best;            /* [T][B][nu]                                                                     */
  double *hist_f;             /* optional [n_steps][3][B]: the cost evaluated in step s, the eta that produced its
                                 candidate (0 at s = 0 and for a frozen trajectory), the predicted decrease     */
  int32_t *hist_i;            /* optional [n_steps][B]: 1 accepted, 0 rejected, -1 not evaluable                */
  double *theta_hist;         /* optional [n_steps][2 nj][B]: the candidate evaluated in step s                 */
  double *g_acc;              /* [2 nj][B] scratch: the gradient at the accepted design                         */
  double *eta;                /* [B] scratch: the step length (negative: the trajectory is frozen)              */
  double *grad;               /* [2 nj][B] scratch: the gradient outputs of the sensitivity sweep               */
} aslr_design_t;

/* ASLR_E_INVALID (aslr_last_error starts with "aslr_design_descent:"; nothing is enqueued and no output is written):
 * p, sp or d NULL; a required buffer NULL (lo / hi count when their field is optimised); n_steps, first_maxiter or
 * iters_per_step < 1; neither field optimised; opt_stiffness on a VSA model; K or B of a model not diagonal; eta0, grow,
 * shrink, c1 or max_rel outside the ranges above; bounds that are not 0 < lo <= hi; an initial design that is not positive
 * or, in an active entry, outside [lo, hi]; an iteration log that is set (every step would overwrite it); the solver /
 * size combinations the solver entry points decline; without a table, what aslr_set_trajectory_params refuses with no
 * field given (models that differ in K, B or the control box).  A reference path (aslr_set_reference_path) is honoured by
 * every sweep and does not slide. */
int aslr_design_descent(aslr_problem_t *p, const aslr_solver_params_t *sp, const aslr_design_t *d, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ASLR_TO_AMD_DESIGN_H */
