/*
 * aslr_to_amd_identify.h -- extension of the C ABI (aslr_to_amd.h): fit the spring stiffness and the motor inertia of every
 * trajectory of the batch to a recorded run, on the device.
 *
 * A header of its own, exported from the same libaslr_to_hip.so: the set of functions aslr_to_amd.h declares, the structs
 * aslr_sizeof knows (aslr_identify_t is read by this call alone and has no index there, like aslr_design_t) and
 * ASLR_ABI_VERSION are what existing bindings check against, and this entry point changes none of them.  A binding that
 * wants it declares it next to the base set; one that does not is unaffected.  Conventions and the error
 * contract are those of aslr_to_amd.h.
 *
 * aslr_policy_rollout, aslr_policy_plant_sensitivity, aslr_mpc_run_plant and aslr_design_descent take the plant's diag K
 * and diag B as given.  This call goes the other way: given what an arm did -- recorded states Y and applied controls U --
 * which K and B explain it, trajectory by trajectory.
 */
#ifndef ASLR_TO_AMD_IDENTIFY_H
#define ASLR_TO_AMD_IDENTIFY_H

#include "aslr_to_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The data of trajectory b are the handle's XS [T+1] (the recorded states) and US [T] (the applied controls); the caller puts
 * them there.  The fitted parameters theta of a trajectory: np entries -- 2 nj with both fields (SEA), nj with one, stiffness
 * before motor inertia -- in rows [np][B] like aslr_design_t (entry p of trajectory b at p B + b).  A field that is not
 * fitted keeps the value of the handle's table.  dt and every other constant are the models'.
 *
 * One-step prediction error under the candidate theta in the table, weights w [nx][B] (NULL: ones):
 *   r_t = XS[t+1] - XNEXT[t]                                   (t < T; XNEXT of the calcDiff sweep at (XS, US); GAPS is not used)
 *   Jz_t = d xnext_t / d log theta, from the Fx record and four words of XS / XNEXT, without a division:
 *     Jz_t[:, K_j] = -delta_j (Fx_t[:, nj+j] - e_{nj+j}),   delta_j = xs_t[j] - xs_t[nj+j]
 *     Jz_t[:, B_j] = -D_j (dt e_{nj+j} + e_{3nj+j}),        D_j = xnext_t[3nj+j] - xs_t[3nj+j]
 *   sse  = sum_t sum_i w_i r_i^2
 *   g_p  = -sum_t sum_i w_i Jz_t[i][p] r_i                     (d (sse / 2) / d log theta_p)
 *   H_pq =  sum_t sum_i w_i Jz_t[i][p] Jz_t[i][q]              (Gauss-Newton; packed lower: entry (p, q <= p) at p (p+1)/2 + q)
 * every sum ONE chain of fused multiply-adds in ascending t and, within a knot, ascending i, term (w_i a) b.
 *
 * Step s = 0 .. n_steps - 1, everything enqueued on `stream`, no host wait between steps:
 *   1. the calcDiff sweep at (XS, US) under the candidate in the table, the model-only record chunks rewritten;
 *   2. sse, g, H of the candidate (identify_normal_kernel);
 *   3. the decision.  Evaluable: sse is finite.  Accepted: evaluable and (s = 0, or sse < sse_acc).
 *        accepted:  (theta, sse, g, H)_acc <- the candidate's, n_accepted + 1, mu <- max(mu shrink, mu_min)   (mu starts at mu0)
 *        otherwise: mu <- min(mu grow, mu_max)
 *      A trajectory that is not evaluable at s = 0 is FROZEN: mu = -1, its candidate stays theta_0, its decisions are -1
 *      and its `identifiable` entries 0; its sse, grad and information hold what step 0 computed.
 *   4. the next candidate, from the accepted set (not in the last step, where the table takes theta_acc itself):
 *        m_p = H_pp > min_curv max_q H_qq;  a parameter with m_p = 0 is NOT IDENTIFIABLE: identity row, dz_p = 0
 *        A = H + mu diag(H) on the identifiable rows and columns, factored A = L D L^T (square-root-free Cholesky; every
 *        product and sum rounded on its own).  A pivot D_p that is not positive or not finite counts as a rejected step:
 *        mu <- min(mu grow, mu_max) and A is rebuilt; at mu_max (or after 64 factorisations) dz = 0.
 *        dz = clamp(-A^-1 g, -max_rel, max_rel),  theta_try_p = clamp(theta_acc_p (1 + dz_p), lo_p, hi_p),
 *      written into column b of TRAJ_PARAMS: K_j as it is, the motor row 1.0 / B_j by IEEE division.
 * Afterwards the table holds theta_acc, the handle's host copy of it has been refreshed by one blocking device-to-host copy,
 * and the handle is, for every later call, what aslr_set_trajectory_params(theta_acc) would leave.  XS / US are not written.
 * Host waits: one on entry (the bounds are read back to be checked, so that a refusal writes nothing), one on exit.
 * The whole shard runs on `stream` (sub-shards are not used).  A reference path and padded controls do not matter: the
 * cost part of the sweep is not read.
 *
 * All pointers are DEVICE pointers owned by the caller, alive until the stream has run the call. */
typedef struct aslr_identify {
  int32_t n_steps;            /* outer steps, >= 1                                                                */
  int32_t fit_stiffness;      /* != 0: the K entries are fitted (SEA only)                                        */
  int32_t fit_motor_inertia;  /* != 0: the B entries are fitted; at least one of the two                          */
  int32_t _pad0;
  double mu0;                 /* initial damping, mu_min <= mu0 <= mu_max                                         */
  double mu_min, mu_max;      /* 0 < mu_min <= mu_max, finite                                                     */
  double grow;                /* factor on mu after a rejected step, > 1                                          */
  double shrink;              /* factor on mu after an accepted one, in (0, 1)                                    */
  double max_rel;             /* largest relative change of an entry per step, in (0, 1)                          */
  double min_curv;            /* identifiability threshold on H_pp / max_q H_qq, in [0, 1)                        */
  const double *weights;      /* [nx][B] per-component weights (>= 0; not checked); NULL: ones                   */
  const double *lo, *hi;      /* [np][B] bounds, 0 < lo <= theta_0 <= hi, finite                                  */
  double *theta;              /* [np][B] out: the accepted parameters                                             */
  double *sse;                /* [B] out: their weighted squared one-step prediction error                        */
  double *grad;               /* [np][B] out: g at the accepted parameters                                        */
  double *information;        /* [np (np+1)/2][B] out: H at the accepted parameters, packed lower                 */
  double *mu;                 /* [B] out: the damping after the last step (negative: the trajectory is frozen)    */
  int32_t *identifiable;      /* [np][B] out: m_p of the accepted set                                             */
  int32_t *n_accepted;        /* [B] out: accepted steps, step 0 included                                         */
  double *hist_theta;         /* optional [n_steps][np][B]: the candidate evaluated in step s                     */
  double *hist_sse;           /* optional [n_steps][B]: its sse                                                   */
  int32_t *hist_decision;     /* optional [n_steps][B]: 1 accepted, 0 rejected, -1 not evaluable or frozen        */
  double *work;               /* [2 np + 1 + np (np+1)/2][B] scratch: the candidate, then its sse, g and H        */
} aslr_identify_t;

/* ASLR_E_INVALID (aslr_last_error starts with "aslr_plant_identify:"; nothing is enqueued and no output is written):
 * p or d NULL; n_steps < 1; neither field fitted; fit_stiffness on a VSA model; K or B of a model not diagonal; a scalar
 * outside the ranges above; a required buffer NULL (all but weights and the three histories); an initial entry of a fitted field
 * that is not positive; bounds that are not 0 < lo <= theta_0 <= hi, finite; without a table, what aslr_set_trajectory_params refuses
 * with no field given. */
int aslr_plant_identify(aslr_problem_t *p, const aslr_identify_t *d, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ASLR_TO_AMD_IDENTIFY_H */
