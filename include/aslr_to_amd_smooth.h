/*
 * aslr_to_amd_smooth.h -- extension of the C ABI (aslr_to_amd.h): estimate the states of a recorded run from its encoder
 * samples -- an iterated extended Kalman smoother (Gauss-Newton on the MAP estimate) on the handle's model, on the device.
 *
 * A header of its own, exported from the same libaslr_to_hip.so: the set of functions aslr_to_amd.h declares, the structs
 * aslr_sizeof knows and ASLR_ABI_VERSION are what existing bindings check against, and this entry point changes none of
 * them (plain pointers, no new struct).  A binding that wants it declares it next to the base set;
 * one that does not is unaffected.  Conventions and the error contract are those of aslr_to_amd.h.
 *
 * aslr_plant_identify (aslr_to_amd_identify.h) fits the plant to recorded states xs [T+1][B][nx], velocities included; an
 * elastic arm has two encoders per joint and nothing else.  This call makes those states from what the encoders give:
 * measurements in, estimates out, with the filter aslr_policy_lqg (aslr_to_amd_lqg.h) builds the gains of.
 */
#ifndef ASLR_TO_AMD_SMOOTH_H
#define ASLR_TO_AMD_SMOOTH_H

#include "aslr_to_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* For trajectory b, with the applied controls in US and a nominal trajectory xb in XS of the handle:
 *   plant        x_{t+1} = f(x_t, u_t) + w_t,   w_t ~ N(0, diag(noise_var[t])),   x_0 ~ N(x0_mean, sigma0)
 *   measurement  y_t = x_t[m] + v_t  at every knot t = 0 .. T,  v_t ~ N(0, diag(meas_var)),  m = meas_idx
 * n_iters iterations, all enqueued by this one call.  One iteration:
 *   1. the calcDiff sweep at (XS, US), as aslr_policy_lqg runs it: Fx_t and XNEXT_t = f(xb_t, u_t);
 *   2. the forward filter, t = 0 .. T, from m^-_0 = x0_mean, Pm_0 = sigma0:
 *        G = Pm_t[:, m],  S = Pm_t[m, m] + diag(meas_var) = C C^T (Cholesky),  L_t = G S^-1,
 *        nu_t = y_t - m^-_t[m],  w_t = S^-1 nu_t,  m_t = m^-_t + L_t nu_t,  P_t = Pm_t - L_t G^T (made symmetric, (a + b) / 2
 *        of the two triangles, as aslr_policy_lqg does),  nis_t = nu_t^T w_t,
 *        m^-_{t+1} = XNEXT_t + Fx_t (m_t - xb_t),  Pm_{t+1} = Fx_t P_t Fx_t^T + diag(noise_var[t])                    (t < T)
 *        nll = 1/2 sum_t (nis_t + 2 sum_a log C_t[a][a]), the terms added in knot order;
 *   3. the backward adjoint sweep, t = T .. 0, from q^+_T = 0:
 *        q_t = q^+_t except at the measured entries, where q_t[m_a] = q^+_t[m_a] + w_t[a] - L_t[:, a] . q^+_t,
 *        xs_t = m^-_t + Pm_t q_t,  q^+_{t-1} = Fx_{t-1}^T q_t,  step = max_{t,i} |xs_t[i] - xb_t[i]|,
 *        XS_t <- xb_t + relax (xs_t - xb_t).
 * This is the fixed-interval smoother in innovation form: xs is the weighted least-squares solution of the problem
 * linearised about xb, xs_T = m_T, and no Pm_t is inverted, so noise_var may be NULL (the fit is then of x_0 alone under
 * exact dynamics).
 *   ny         number of measured state entries, 1 <= ny <= nx;
 *   meas_idx   HOST pointer, ny distinct indices in [0, nx), in any order; NULL: 0 .. ny-1 (ny = nx / 2: the positions
 *              q_l, q_m).  Read before the call returns;
 *   n_iters    >= 1;   relax  in (0, 1]: the part of the Gauss-Newton step that is taken.
 * Inputs, DEVICE pointers, time-major like the workspace:
 *   ys         [T+1][B][ny]  the measurements, in the order of meas_idx; required;
 *   meas_var   [B][ny]       variances of the measurement noise, > 0 (not checked: they live on the device); required;
 *   x0_mean    [B][nx]       required;
 *   sigma0     [B][nx][nx]   symmetric: only the entries [i][j] with i >= j are read, and they are mirrored; nullable (zero);
 *   noise_var  [T][B][nx]    variances of the process noise; nullable (zero);
 *   work       caller-owned scratch of (T+1) B (nx nx + nx ny + nx + ny) doubles; required.  Between the two sweeps of an
 *              iteration it holds Pm_t, L_t, m^-_t and w_t of every knot; its contents after the call are not specified.
 * Outputs are DEVICE pointers, each optional (NULL: nothing written):
 *   xs_smooth    [T+1][B][nx]  xs_t of the last iteration, before relax;
 *   x_filt       [T+1][B][nx]  m_t of the last iteration;
 *   est_var      [T+1][B][nx]  diagonal of P_t of the last iteration;
 *   nis          [T+1][B]      nis_t of the last iteration;
 *   neg_log_lik  [n_iters][B]  nll of every iteration;
 *   step_norm    [n_iters][B]  step of every iteration.
 * Side effects: those of aslr_calc_diff (XNEXT, COST, DERIV), and XS holds the relaxed estimate of the last iteration.  The
 * records are those of the nominal BEFORE the last step, not of what XS holds on return.  US, KGAIN and the solver state
 * are untouched.  n_iters = k is, bit for bit, k calls with n_iters = 1.
 * Limit of validity: that of aslr_policy_lqg.  P_t = Pm_t - L_t G^T is the plain form of the update; a pivot of the factor of
 * S_t that comes out <= 0 (meas_var <= 0 or NaN, sigma0 not positive semi-definite, a prior spread to 1e16 times meas_var)
 * makes every output of THAT trajectory NaN from that knot on, XS with it, and so for the remaining iterations.  Other
 * trajectories are not affected, the return code is ASLR_OK (the call only enqueues), and nothing is written out of bounds.
 * The results of a trajectory do not depend on B or on its place in the batch, and an output has the same bits whichever
 * others are asked for.
 * Honours the parameter table, a reference path and padded controls, all through the calcDiff sweep.  Covers the whole
 * shard on the caller's stream; enqueues only: no host round trip between iterations.
 * ASLR_E_INVALID (aslr_last_error starts with "aslr_state_smooth:"; nothing is enqueued or written and the handle stays
 * live): a NULL handle; ny < 1 or ny > nx; an index outside [0, nx) or a repeated index (the message names it); ys, meas_var,
 * x0_mean or work NULL; all six outputs NULL; sigma0 and noise_var both NULL; n_iters < 1; relax outside (0, 1]. */
int aslr_state_smooth(aslr_problem_t *p,
                      int32_t ny,
                      const int32_t *meas_idx,
                      const double *ys,
                      const double *meas_var,
                      const double *x0_mean,
                      const double *sigma0,
                      const double *noise_var,
                      int32_t n_iters,
                      double relax,
                      double *work,
                      double *xs_smooth,
                      double *x_filt,
                      double *est_var,
                      double *nis,
                      double *neg_log_lik,
                      double *step_norm,
                      void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ASLR_TO_AMD_SMOOTH_H */
