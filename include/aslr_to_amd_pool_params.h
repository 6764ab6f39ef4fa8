/*
 * aslr_to_amd_pool_params.h -- extension of the C ABI (aslr_to_amd.h): a pool solve whose problems each carry their own
 * spring stiffness, motor inertia and control box.
 *
 * A header of its own, exported from the same libaslr_to_hip.so, for the reason aslr_to_amd_sens.h gives: the set of
 * functions aslr_to_amd.h declares, the structs aslr_sizeof knows (aslr_pool_t among them) and ASLR_ABI_VERSION are what
 * existing bindings check against, and this entry point changes none of them.  The one struct it adds is read by this call
 * alone and is not an aslr_sizeof index.  A binding that wants it declares it next to the base set; one
 * that does not is unaffected.  Conventions and the error contract are those of aslr_to_amd.h.
 *
 * The library has two ways to solve many problems.  A lock-step batch gives every trajectory its own K, B and control box
 * (aslr_set_trajectory_params): the design sweep.  The pool (aslr_solve_pool) streams P >> B problems through the B slots,
 * each to its own stop, because a lock-step batch waits for its slowest member -- and a design sweep, where soft and stiff
 * designs of one task need very different iteration counts, is the workload that waits most.  aslr_solve_pool declines a
 * handle with a table (a pool problem would inherit its slot's row).  This call is the pool for design sweeps: the refill
 * hands a slot its problem's parameters together with its x0 and target.
 */
#ifndef ASLR_TO_AMD_POOL_PARAMS_H
#define ASLR_TO_AMD_POOL_PARAMS_H

#include "aslr_to_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Per-PROBLEM parameters of a pool: the fields of aslr_traj_params_t with one row per problem of the pool instead of one per
 * trajectory of the shard.  The four tables are HOST pointers, row-major, each optional (NULL: every problem keeps the
 * models' constant for that field, which the models of the problem must then agree on -- the rule of
 * aslr_set_trajectory_params); params_dev is a DEVICE buffer. */
typedef struct aslr_pool_params {
  const double *stiffness;     /* HOST [P][nj] diagonal of K.  SEA only: a VSA model takes its stiffness from u      */
  const double *motor_inertia; /* HOST [P][nj] diagonal of B, finite and > 0 (the kernels use the reciprocals)       */
  const double *u_lb, *u_ub;   /* HOST [P][nu] the control box of every model with has_u_limits set, lb <= ub, no NaN */
  double *params_dev;          /* DEVICE scratch [2 nj + 2 nu][P] doubles, owned by the caller: the call uploads the
                                  table here (rows: K, 1 / B, u_lb, u_ub, as region TRAJ_PARAMS) and the refill reads
                                  column j when it hands out problem j.  Needed as soon as a field is given            */
} aslr_pool_params_t;

/* aslr_solve_pool (see there for pool, refill_every, poll_every, iters_done and the outputs) with problem j of the pool
 * solved with row j of every given field.  Every problem goes through exactly the iterations aslr_solve gives it on a
 * handle whose parameter table holds the same values in its row: results do not depend on B, on the slot, on refill_every
 * or on the sub-shard count, bit for bit.
 * pp == NULL, or every table of pp NULL: the call IS aslr_solve_pool(p, sp, pool, ...), refusals and their wording included.
 *
 * The tables are validated and lowered on the host as aslr_set_trajectory_params does it (1 / B is formed there), uploaded
 * to params_dev on `stream`, and the call returns after the last flush, as aslr_solve_pool does; the host arrays may be
 * released on return.
 *
 * The handle on return: X0 / FRAME_REF restored as by aslr_solve_pool; back on the models' constants (the kernels of a handle
 * without a table); the content of region TRAJ_PARAMS unspecified.  A plain aslr_solve afterwards gives the bits it gives
 * on a fresh handle, and so does aslr_set_trajectory_params followed by a solve.
 *
 * ASLR_E_INVALID (aslr_last_error starts with "aslr_solve_pool_params:"; nothing is written to the outputs, to params_dev or
 * to the workspace, and the handle stays as it was):
 *   everything aslr_solve_pool refuses (NULL arguments, P < 1, a missing pool array, maxiter < 1 or fixed_iterations, per-
 *   problem frame references on a handle without a frame_ref table, a reference path set, a solver the size is not built for);
 *   a handle with a parameter table set (the refill overwrites region TRAJ_PARAMS: the table would be lost -- clear it
 *   first, or put its rows into pp);
 *   params_dev NULL while a field is given;
 *   what aslr_set_trajectory_params refuses in a table: stiffness on a VSA model; u_lb / u_ub when no model has control
 *   limits; K or B of a model not diagonal; a field left out on which the models differ; a stiffness entry that is not
 *   finite; a motor_inertia entry that is not finite and > 0; u_lb <= u_ub violated (NaN included).
 * Out of scope: reference paths in pools, sensitivities at flush, parameter tables that already lie on the device, MPC
 * through a pool. */
int aslr_solve_pool_params(aslr_problem_t *p, const aslr_solver_params_t *sp, const aslr_pool_t *pool,
                           const aslr_pool_params_t *pp, int32_t refill_every, int32_t poll_every, void *stream,
                           int32_t *iters_done);

#ifdef __cplusplus
}
#endif
#endif /* ASLR_TO_AMD_POOL_PARAMS_H */
