/*
 * aslr_to_amd_lqg.h -- extension of the C ABI (aslr_to_amd.h): first-order covariance of the stored policy under OUTPUT
 * feedback -- the time-varying Kalman filter for "these state entries are measured, with this noise", the Riccati gains fed
 * the filter's estimate (LQG), and the spread that results.
 *
 * A header of its own, exported from the same libaslr_to_hip.so: the set of functions aslr_to_amd.h declares, the structs
 * aslr_sizeof knows and ASLR_ABI_VERSION are what existing bindings check against, and this entry point changes none of
 * them (plain pointers, no new struct).  A binding that wants it declares it next to the base set;
 * one that does not is unaffected.  Conventions and the error contract are those of aslr_to_amd.h.
 *
 * aslr_policy_covariance (aslr_to_amd_cov.h) assumes the feedback law sees the whole state x = [q_l, q_m, v_l, v_m].  An
 * elastic arm has two encoders per joint and nothing else; this call answers the same question for a controller that sees
 * some entries of the state, noisily, and estimates the rest.
 */
#ifndef ASLR_TO_AMD_LQG_H
#define ASLR_TO_AMD_LQG_H

#include "aslr_to_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* For trajectory b with states xs, controls us and gains K (XS, US and KGAIN of the handle) and e_t = x_t - xs_t:
 *   plant        e_{t+1} = Fx_t e_t + Fu_t du_t + w_t,        w_t ~ N(0, diag(noise_var[t]))
 *   measurement  y_t = e_t[m] + v_t  at every knot t = 0 .. T, v_t ~ N(0, diag(meas_var)),  m = meas_idx
 *   controller   du_t = -K_t eh_t,  eh_t the filter's posterior estimate;  the estimator starts on the plan (eh_0^- = 0) and
 *                e_0 ~ N(0, sigma0).
 * Runs the calcDiff sweep on (XS, US) as aslr_policy_covariance does (writes XNEXT, COST, DERIV), then one forward recursion
 * per trajectory on the records, with Pm the prior error covariance, P the posterior and Xh the covariance of the estimate:
 *   Pm_0 = sigma0,  Xm_0 = 0
 *   update (t = 0 .. T)   G_t = Pm_t[:, m],   S_t = Pm_t[m, m] + diag(meas_var),   L_t = G_t S_t^-1 (Cholesky of S_t),
 *                         D_t = L_t G_t^T,   P_t = Pm_t - D_t,   Xh_t = Xm_t + D_t
 *   outputs at t          Sigma_t = Xh_t + P_t,   U_t = K_t Xh_t K_t^T   (t < T)
 *   predict (t < T)       Pm_{t+1} = Fx_t P_t Fx_t^T + diag(noise_var[t]),   Xm_{t+1} = A_t Xh_t A_t^T,   A_t = Fx_t - Fu_t K_t
 *   cost_increase = 1/2 sum_{t<T} [tr(Lxx_t Sigma_t) - 2 tr(Lxu_t K_t Xh_t) + tr(Luu_t U_t)] + 1/2 tr(Lxx_T Sigma_T),
 * the terms added in knot order.  The filter reads neither K nor Fu (the estimator knows the control): P_t and L_t are the
 * same whatever the gains are.  With every entry measured and meas_var -> 0 this is aslr_policy_covariance; with
 * meas_var -> infinity it is the open-loop covariance with u_var = 0.  KGAIN is used as the handle holds it, and the control
 * box is not applied, as in aslr_policy_covariance.
 *   ny         number of measured state entries, 1 <= ny <= nx;
 *   meas_idx   HOST pointer, ny distinct indices in [0, nx), in any order; NULL: 0 .. ny-1 (ny = nx / 2: the positions
 *              q_l, q_m).  Read before the call returns.
 * Inputs, DEVICE pointers:
 *   meas_var   [B][ny]       variances of the measurement noise, > 0 (not checked: they live on the device), in the order
 *                            of meas_idx; required;
 *   sigma0     [B][nx][nx]   Sigma_0, symmetric: only the entries [i][j] with i >= j are read, and they are mirrored; nullable (zero);
 *   noise_var  [T][B][nx]    variances of the process noise, time-major like the workspace; nullable (zero).
 * Outputs are DEVICE pointers, each optional (NULL: not computed, nothing written), time-major like the workspace:
 *   x_var          [T+1][B][nx]      diagonal of Sigma_t;
 *   u_var          [T][B][nu]        diagonal of U_t (padded controls have zero gain rows and variance 0);
 *   est_var        [T+1][B][nx]      diagonal of P_t, the variance of the estimation error after the measurement of knot t;
 *   cov_final      [B][nx][nx]       Sigma_T;
 *   est_cov_final  [B][nx][nx]       P_T;
 *   kalman_gain    [T+1][B][nx][ny]  L_t, its columns in the order of meas_idx;
 *   cost_increase  [B].
 * Limit of validity.  P_t = Pm_t - D_t is the plain form of the update, not the Joseph form: it is a
 * difference that cancels log10(lambda_max(Pm_t) / meas_var) digits.  While that ratio stays below about 1e8 the outputs carry
 * at least half of a double's digits; as it approaches 1e16 (a plan whose open loop spreads the prior by that much against
 * the measurement noise, typically an unconverged plan over a long horizon) P_t loses definiteness, a pivot of the Cholesky
 * factor of S_{t+1} comes out <= 0, and every output of THAT trajectory is NaN from that knot on (cost_increase and the two
 * final matrices with it).  The same holds from knot 0 when a meas_var is <= 0 or NaN, or sigma0 is not positive
 * semi-definite.  Other trajectories are not affected, the return code is ASLR_OK (the call only enqueues), and nothing is
 * written out of bounds: check the outputs with isfinite, and scale meas_var to the spread or shorten the horizon.
 * Stored matrices are computed a row per lane and taken as columns by symmetry.  After every update P_t and Xh_t are made
 * symmetric, (a + b) / 2 of the two triangles: in the recursion as written their difference, a rounding error at first, is
 * multiplied by |Fx|^2 per knot and never damped.  cov_final and est_cov_final are therefore symmetric bit for bit.  The results of a trajectory do not depend on B or on its place in the batch, and an output
 * has the same bits whichever others are asked for.
 * Honours the parameter table, a reference path and padded controls, all through the calcDiff sweep.  Covers the whole
 * shard on the caller's stream (sub-shards do not apply); enqueues only, like aslr_calc_diff.  Side effects: those of
 * aslr_calc_diff.
 * ASLR_E_INVALID (aslr_last_error starts with "aslr_policy_lqg:"; nothing is written and the handle stays live): a NULL
 * handle; ny < 1 or ny > nx; an index outside [0, nx) or a repeated index (the message names it); meas_var NULL; all seven
 * outputs NULL; sigma0 and noise_var both NULL (nothing to propagate). */
int aslr_policy_lqg(aslr_problem_t *p,
                    int32_t ny,
                    const int32_t *meas_idx,
                    const double *meas_var,
                    const double *sigma0,
                    const double *noise_var,
                    double *x_var,
                    double *u_var,
                    double *est_var,
                    double *cov_final,
                    double *est_cov_final,
                    double *kalman_gain,
                    double *cost_increase,
                    void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ASLR_TO_AMD_LQG_H */
