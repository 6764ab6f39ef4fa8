// aslr_identify.inc.hpp -- the two kernels behind aslr_plant_identify (include/aslr_to_amd_identify.h; DESIGN.md section
// 4.20): identify_normal_kernel, the normal equations of a one-step prediction-error fit of a trajectory's spring stiffness
// and motor inertia to the recorded run in XS / US, and identify_step_kernel, the Levenberg-Marquardt step between two sweeps.
//
//   r_t = xs_{t+1} - xnext_t                                                       (t = 0 .. T-1; xnext of the calcDiff sweep at (XS, US))
//   Jz_t[:, K_c] = -delta_c (Fx_t[:, nj+c] - e_{nj+c}),   delta_c = xs_t[c] - xs_t[nj+c]     (the columns of the tangent sweep's G_t
//   Jz_t[:, B_c] = -D_c (dt e_{nj+c} + e_{3nj+c}),        D_c = xnext_t[3nj+c] - xs_t[3nj+c]   times the parameter: no division)
//   sse = sum_t sum_i w_i r_i^2,   g_p = -sum_t sum_i w_i Jz_t[i][p] r_i,   H_pq = sum_t sum_i w_i Jz_t[i][p] Jz_t[i][q]
//
// ---- identify_normal_kernel ----
// With E_t = [Jz_t | r_t] ([nx][np + 1]) all three are entries of ONE packed lower matrix M = sum_t E_t^T W E_t of order np + 1:
// H is its leading block (same packed index), -g its last row, sse its last entry.  NE = (np + 1)(np + 2) / 2 entries: 6 .. 120.
//
// Decomposition: one team of lanes per trajectory (aslr_sweep_team.hpp).  Per knot lane j stages row j of E_t and of
// W E_t in the team's LDS (two buffers used in turn: one barrier per knot), then every lane of the team continues the sums of
// the entries it owns -- entry e of M belongs to lane e % TEAM, at most 4 per lane:
//   M[c][d] = fma(w_i E[i][c], E[i][d], M[c][d])        i = 0 .. nx-1 within the knot, knots in ascending order
// Every entry is therefore ONE fma chain over (t, i) in the order of the definition, held by one lane from the first knot to
// the last: no partial sums are combined, so there is no combination order to fix, and the knots are not a dependency chain
// beyond that sum (nothing of knot t feeds knot t + 1; the loads of knot t + 1 are in flight while knot t is reduced).
// The kernel reads, per knot: columns nj .. 2nj-1 of the lane's row of Fx (STIFF only), xs_t[0 .. 2nj-1] (STIFF only),
// xs_t[3nj+c] and xnext_t[3nj+c] of the lane's joint, xs_{t+1}[j] and xnext_t[j].  It reads no K and no B.
// The rows of E are indexed at run time in LDS only; the accumulators are registers with compile-time indices: no scratch.
//
// ---- identify_step_kernel ----
// One block per trajectory, lane 0 at work (np <= 14: the accepted set, a packed LDL^T and its solve, in LDS).  The rule is
// stated operation by operation in the header and restated in numpy by tests/_identify.py, which must reproduce the bits:
// every product, sum and quotient is an explicitly rounded intrinsic and the unit is compiled with -ffp-contract=off (the
// fma calls of the kernel above are explicit and unaffected).
#pragma once
#include "aslr_sweep_team.hpp"

namespace aslr {

template <int NX, int NU, bool STIFF>
__global__ void __launch_bounds__(64) identify_normal_kernel(IdentifyNormalArgs a) {
  constexpr int NJ = SweepTeam<NX>::NJ, TEAM = SweepTeam<NX>::TEAM, TPW = SweepTeam<NX>::TPW;
  constexpr int NP = STIFF ? 2 * NJ : NJ, P0 = NP - NJ, NC = NP + 1; // columns of Jz; the first motor-inertia column; columns of E
  constexpr int NE = NC * (NC + 1) / 2, SL = (NE + TEAM - 1) / TEAM;  // entries of M, and how many of them one lane sums
  constexpr int NF = STIFF ? NJ : 1;
  using L = RecLayout<NJ, NU>;
  constexpr int oE = 0, oW = NX * NC, BUF = 2 * NX * NC; // one buffer of a team: E [nx][nc], W E [nx][nc]
  __shared__ __attribute__((aligned(16))) double lds[TPW * 2 * BUF];
  const int lane = threadIdx.x, jr = lane % TEAM;
  double *tm = lds + (lane / TEAM) * 2 * BUF;
  const int br = blockIdx.x * TPW + lane / TEAM;
  const int B = a.B, T = a.T;
  const int b = br < B ? br : B - 1, j = jr < NX ? jr : NX - 1; // clamped: every lane reads inside the arrays
  const bool work = jr < NX;                                    // the idle lanes of a 32-lane team stage no row
  const bool mot = j >= NJ && j < 2 * NJ, vel = j >= 3 * NJ;     // row nj + c takes -D_c dt, row 3nj + c takes -D_c
  const int jj = mot ? j - NJ : (vel ? j - 3 * NJ : 0);
  const double w = a.weights ? a.weights[(size_t)j * B + b] : 1.0;
  // the entries of M this lane sums: (row c, column d <= c) of packed index jr + m TEAM, clamped
  int sc[SL], sd[SL];
  ASLR_UNROLL for (int m = 0; m < SL; ++m) {
    const int idx = jr + m * TEAM, ic = idx < NE ? idx : NE - 1;
    int c = 0;
    while ((c + 1) * (c + 2) / 2 <= ic) ++c;
    sc[m] = c; sd[m] = ic - c * (c + 1) / 2;
  }

  struct Knot { double fx[NF], q[2 * NF], x1, xn, vm, vmn; };
  const auto load = [&](Knot &k, int t) {
    const size_t xo = ((size_t)t * B + b) * NX;
    if (STIFF) {
      const double *rec = a.deriv + ((size_t)t * B + b) * L::len + L::oFx + j * NX + NJ;
      ASLR_UNROLL for (int c = 0; c < NJ; ++c) k.fx[c] = rec[c];
      ASLR_UNROLL for (int c = 0; c < 2 * NJ; ++c) k.q[c] = a.xs[xo + c];
    }
    k.x1 = a.xs[xo + (size_t)B * NX + j]; k.xn = a.xnext[xo + j];
    k.vm = a.xs[xo + 3 * NJ + jj]; k.vmn = a.xnext[xo + 3 * NJ + jj];
  };

  double acc[SL];
  ASLR_UNROLL for (int m = 0; m < SL; ++m) acc[m] = 0.0;
  Knot cur;
  load(cur, 0);
  for (int t = 0; t < T; ++t) {
    Knot nxt;
    load(nxt, t + 1 < T ? t + 1 : T - 1); // in flight while knot t is reduced (t = T-1: a repeat, dropped)
    double *bf = tm + (t & 1) * BUF;
    const int mi = knot_model(a.node_model, t);
    double dt = a.dt[0];
    ASLR_UNROLL for (int m = 1; m < ASLR_MAX_MODELS; ++m)
      if (mi == m) dt = a.dt[m];
    if (work) { // row j of E_t and of W E_t
      double *e = bf + oE + j * NC, *we = bf + oW + j * NC;
      if (STIFF) {
        ASLR_UNROLL for (int c = 0; c < P0; ++c) {
          const double v = -(cur.q[c] - cur.q[NJ + c]) * (cur.fx[c] - (j == NJ + c ? 1.0 : 0.0));
          e[c] = v; we[c] = w * v;
        }
      }
      const double nd = -(cur.vmn - cur.vm);
      ASLR_UNROLL for (int c = 0; c < NJ; ++c) {
        const double v = j == NJ + c ? nd * dt : (j == 3 * NJ + c ? nd : 0.0);
        e[P0 + c] = v; we[P0 + c] = w * v;
      }
      const double r = cur.x1 - cur.xn;
      e[NP] = r; we[NP] = w * r;
    }
    __syncthreads(); // (the buffer of knot t - 1 is the other one; that of knot t - 2 was last read before the barrier of t - 1)
    ASLR_UNROLL for (int m = 0; m < SL; ++m) {
      const double *pw = bf + oW + sc[m], *pe = bf + oE + sd[m];
      double v = acc[m];
      _Pragma("unroll 4") for (int i = 0; i < NX; ++i) v = fma(pw[i * NC], pe[i * NC], v);
      acc[m] = v;
    }
    cur = nxt;
  }
  if (br < B) {
    ASLR_UNROLL for (int m = 0; m < SL; ++m) {
      const int idx = jr + m * TEAM, c = sc[m], d = sd[m];
      if (idx >= NE) continue;
      if (c < NP) { if (c < a.np_out) a.information[(size_t)idx * B + b] = acc[m]; }
      else if (d < NP) { if (d < a.np_out) a.grad[(size_t)d * B + b] = -acc[m]; }
      else a.sse[b] = acc[m];
    }
  }
}

template <int NJ, int DAM>
int launch_identify_normal(const IdentifyNormalArgs &a, hipStream_t st) {
  return launch_sweep_stiff<NJ, DAM>([](auto STIFF) { return identify_normal_kernel<4 * NJ, ModelDims<NJ, DAM>::nu, decltype(STIFF)::value>; }, a, st);
}

// NPMAX: the most parameters a trajectory of the size can have (2 nj on SEA, nj on VSA): the size of the LDS arrays
template <int NPMAX>
__global__ void __launch_bounds__(64) identify_step_kernel(IdentifyStepArgs a) {
  constexpr int NH = NPMAX * (NPMAX + 1) / 2;
  __shared__ double H[NH], A[NH], D[NPMAX], g[NPMAX], x[NPMAX], th[NPMAX];
  __shared__ int msk[NPMAX];
  if (threadIdx.x != 0) return;
  const int b = blockIdx.x, B = a.B, np = a.np, nh = np * (np + 1) / 2;
  const auto at = [](int p, int q) { return p * (p + 1) / 2 + q; }; // packed lower, q <= p
  // ---- the decision on the candidate ----
  const double sse_t = a.sse_try[b];
  const double mu_in = a.s == 0 ? a.mu0 : a.mu[b];
  const bool frozen = a.s > 0 && mu_in < 0.0;
  const bool evaluable = isfinite(sse_t);
  const bool accept = a.s == 0 ? evaluable : (!frozen && evaluable && sse_t < a.sse[b]);
  const bool freeze = frozen || (a.s == 0 && !evaluable);
  const bool take = accept || a.s == 0;
  if (a.hist_sse) a.hist_sse[b] = sse_t;
  if (a.hist_decision) a.hist_decision[b] = (freeze || !evaluable) ? -1 : (accept ? 1 : 0);
  // ---- the accepted set ----
  for (int p = 0; p < np; ++p) {
    const size_t i = (size_t)p * B + b;
    const double tt = a.theta_try[i];
    if (a.hist_theta) a.hist_theta[i] = tt;
    if (take) { a.theta[i] = tt; a.grad[i] = a.g_try[i]; }
    th[p] = a.theta[i]; g[p] = a.grad[i];
  }
  for (int k = 0; k < nh; ++k) {
    const size_t i = (size_t)k * B + b;
    if (take) a.information[i] = a.h_try[i];
    H[k] = a.information[i];
  }
  if (take) a.sse[b] = sse_t;
  a.n_accepted[b] = (a.s == 0 ? 0 : a.n_accepted[b]) + (accept ? 1 : 0);
  double mu;
  if (freeze) mu = -1.0;
  else if (accept) { mu = __dmul_rn(mu_in, a.shrink); if (mu < a.mu_min) mu = a.mu_min; }
  else { mu = __dmul_rn(mu_in, a.grow); if (mu > a.mu_max) mu = a.mu_max; }
  // ---- which parameters the accepted data identify ----
  double maxd = H[0];
  for (int q = 1; q < np; ++q)
    if (H[at(q, q)] > maxd) maxd = H[at(q, q)];
  const double thr = __dmul_rn(a.min_curv, maxd);
  for (int p = 0; p < np; ++p) {
    msk[p] = !freeze && H[at(p, p)] > thr;
    a.identifiable[(size_t)p * B + b] = msk[p];
  }
  // ---- the next candidate: A = H + mu diag(H) = L D L^T on the identifiable block (L in place of A), dz = -A^-1 g ----
  bool solved = false;
  if (!a.last && !freeze) {
    for (int tries = 0;; ++tries) {
      for (int p = 0; p < np; ++p)
        for (int q = 0; q <= p; ++q) {
          const double h = H[at(p, q)];
          A[at(p, q)] = p == q ? (msk[p] ? __dadd_rn(h, __dmul_rn(mu, h)) : 1.0) : ((msk[p] && msk[q]) ? h : 0.0);
        }
      bool ok = true;
      for (int p = 0; p < np && ok; ++p) {
        double d = A[at(p, p)];
        for (int k = 0; k < p; ++k) d = __dsub_rn(d, __dmul_rn(__dmul_rn(A[at(p, k)], A[at(p, k)]), D[k]));
        if (!(d > 0.0) || !isfinite(d)) { ok = false; break; }
        D[p] = d;
        for (int i = p + 1; i < np; ++i) {
          double v = A[at(i, p)];
          for (int k = 0; k < p; ++k) v = __dsub_rn(v, __dmul_rn(__dmul_rn(A[at(i, k)], A[at(p, k)]), D[k]));
          A[at(i, p)] = __ddiv_rn(v, d);
        }
      }
      if (ok) { solved = true; break; }
      if (!(mu < a.mu_max) || tries == 63) break; // a failed pivot: a rejected step
      mu = __dmul_rn(mu, a.grow);
      if (mu > a.mu_max) mu = a.mu_max;
    }
    if (solved) {
      for (int p = 0; p < np; ++p) { // L y = -g, then y / D
        double v = msk[p] ? -g[p] : 0.0;
        for (int k = 0; k < p; ++k) v = __dsub_rn(v, __dmul_rn(A[at(p, k)], x[k]));
        x[p] = v;
      }
      for (int p = 0; p < np; ++p) x[p] = __ddiv_rn(x[p], D[p]);
      for (int p = np - 1; p >= 0; --p) { // L^T dz = that
        double v = x[p];
        for (int k = p + 1; k < np; ++k) v = __dsub_rn(v, __dmul_rn(A[at(k, p)], x[k]));
        x[p] = v;
      }
    }
  }
  a.mu[b] = mu;
  for (int p = 0; p < np; ++p) {
    const size_t i = (size_t)p * B + b;
    double next = th[p];
    if (solved && msk[p]) {
      double dz = x[p];
      dz = dz < -a.max_rel ? -a.max_rel : (dz > a.max_rel ? a.max_rel : dz);
      next = __dmul_rn(th[p], __dadd_rn(1.0, dz));
      const double lo = a.lo[i], hi = a.hi[i];
      next = next < lo ? lo : (next > hi ? hi : next);
    }
    a.theta_try[i] = next;
    // K as it is; the motor row is the reciprocal, by IEEE division like the host's row builder
    const int row = a.row0 + p;
    a.traj_params[(size_t)row * B + b] = row < a.nj ? next : __ddiv_rn(1.0, next);
  }
}

template <int NJ, int DAM>
int launch_identify_step(const IdentifyStepArgs &a, hipStream_t st) {
  hipLaunchKernelGGL((identify_step_kernel<(DAM == ASLR_DAM_SEA ? 2 * NJ : NJ)>), dim3(a.B), dim3(64), 0, st, a);
  HIP_TRY(hipGetLastError());
  return ASLR_OK;
}

} // namespace aslr
