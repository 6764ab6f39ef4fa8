// aslr_lqg.inc.hpp -- the output-feedback (LQG) covariance sweep behind aslr_policy_lqg (include/aslr_to_amd_lqg.h).
//
//   Pm_0 = sigma0, Xm_0 = 0;   at every knot t = 0 .. T, for the measured state entries m (ny of them, variances r):
//   update    G = Pm[:, m],  S = Pm[m, m] + diag(r) = C C^T,  L = G S^-1,  D = L G^T,  P = Pm - D,  Xh = Xm + D
//   outputs   Sigma = Xh + P,  U = K Xh K^T                                                                     (U: t < T)
//   predict   Pm' = Fx P Fx^T + diag(w_t),   Xm' = A Xh A^T,  A = Fx - Fu K                                        (t < T)
//   cost_increase = 1/2 sum_t [tr(Lxx_t Sigma_t) - 2 tr(Lxu_t K_t Xh_t) + tr(Luu_t U_t)] + 1/2 tr(Lxx_T Sigma_T)
//
// Decomposition: that of covariance_kernel (aslr_covariance.inc.hpp; the team: aslr_sweep_team.hpp).  Lane j owns column j
// of Pm / P and column j of Xm / Xh (its registers), row j of L, row j of Fx, Fu and A.  What a team shares is staged per
// team in LDS and read back at team-uniform addresses (broadcast reads).  The team's LDS, in doubles:
//   SP [TEAM][nx]  a row per lane: its column of Pm (update), then of P, then its row of Fx P
//   SX [TEAM][nx]  a row per lane: its row of the gain -- g, then z, then L[j][:] (update) -- then its column of Xh, then
//                  its row of A Xh
//   At [nx][nx]    the Cholesky factor C of S, row a at At + a nx (update); then A^T; then Fx^T
//   K, G [nu][nx]  K_t;  G = K Xh
//   F [TEAM][nu]   a row per lane: its row of Fu, then its row of U
//   R, D [nx]      the measurement variances of the trajectory (staged once);  1 / C[a][a], which stands for the diagonal
//   T [2 nx + nu]  the trace parts
// The measured rows are a run-time list, so nothing indexed by it is a register array: g[a] = Pm[m_a][j] is word m_a of the
// lane's own row of SP, S[a][c] = Pm[m_c][m_a] is word m_c of row m_a of SP, and the rows of the gain live in SX.  The list
// itself travels by value in the kernel arguments and is staged once, for the wave, in LDS.  One knot:
//   stage    K_t, column j of Pm, row j of Fu -> LDS                                                             | barrier
//   factor   for c = 0 .. ny-1: lane a >= c takes C[a][c] = (S[a][c] - sum_{k<c} C[a][k] C[c][k]) / C[c][c]; every lane
//            forms C[c][c] itself, from the row c it reads anyway, so a column costs one barrier                | ny barriers
//   solve    lane j: C z = g, C^T l = z on its own row of SX (two triangular solves); L[j][:] -> kalman_gain
//   D        d[c] = sum_a L[j][a] Pm[m_a][c]: row j of D, taken as column j by symmetry;  p = pm - d,  xh = xm + d  | barrier
//   sym      p and xh -> LDS | barrier | p[c] = (p[c] + P[j][c]) / 2 from lane c's row, xh likewise                   | barrier
//   stage    columns of P and Xh, row j of A (transposed), column j of G -> LDS; est_var, x_var                   | barrier
//   Xm'      Y = A Xh (row j -> LDS | barrier), Xm' = Y A^T;  the control terms as in covariance_kernel           | barrier
//   Pm'      Fx^T -> LDS | barrier | Y = Fx P (row j -> LDS | barrier), Pm' = Y Fx^T, + w_t on the diagonal
// The records of knot t + 1 are asked for once Fx_t^T is staged and are in flight during the last product.
// Every sum is ONE fma chain in ascending index order; the long sums stay loops, two steps per trip, for the reason given
// in aslr_covariance.inc.hpp (unrolled in full they spill), and the sums over the measured set are loops because ny is a
// run-time number.  The filter -- P, L -- reads neither K nor Fu.  The Xh half is computed only when an output needs it
// (x_var, u_var, cov_final, cost_increase), the control terms only for u_var or cost_increase; neither enters P, and the
// control terms do not enter Xh, so every output has the same bits whichever others are asked for.
//
// Arithmetic per lane and knot: 4 nx^2 + nu nx fma for the two congruence products and A, ny nx for D, ny^2 for the two
// solves and ny^2 / 2 (twice: the lane's entry and the diagonal) for the factor -- the last two on one serial chain each.
#pragma once
#include "aslr_sweep_team.hpp"

namespace aslr {

template <int NX, int NU>
__global__ void __launch_bounds__(64) lqg_kernel(LqgArgs a) {
  constexpr int NJ = SweepTeam<NX>::NJ, TEAM = SweepTeam<NX>::TEAM, TPW = SweepTeam<NX>::TPW;
  constexpr int NK = NU * NX, KP = (NK + TEAM - 1) / TEAM; // words of K_t, and how many of them one lane of the team loads
  using L = RecLayout<NJ, NU>;
  constexpr int oSP = 0, oSX = oSP + TEAM * NX, oAt = oSX + TEAM * NX, oK = oAt + NX * NX, oG = oK + NK, oF = oG + NK,
                oR = oF + TEAM * NU, oD = oR + NX, oT = oD + NX, LEN = (oT + 2 * NX + NU + 1) / 2 * 2;
  static_assert(TPW * LEN * sizeof(double) + NX * sizeof(int) <= 65536, "the teams of a wave do not fit the LDS of a block");
  __shared__ __attribute__((aligned(16))) double lds[TPW * LEN];
  __shared__ int meas[NX]; // the measured entries, for every team of the wave
  const int lane = threadIdx.x, jr = lane % TEAM;
  double *tm = lds + (lane / TEAM) * LEN;
  const int br = blockIdx.x * TPW + lane / TEAM;
  const int B = a.B, T = a.T, ny = a.ny;
  const int b = br < B ? br : B - 1, j = jr < NX ? jr : NX - 1; // clamped: every lane reads inside the arrays
  const int ku = jr < NU ? jr : NU - 1;                         // the row of U this lane reduces
  const int ar = jr < ny ? jr : ny - 1;                         // the row of the factor this lane reduces
  const bool work = jr < NX;                                    // the idle lanes of a 32-lane team write no shared word
  const bool live = br < B && work, live_u = br < B && jr < NU; // trajectories past B store nothing to memory
  const bool ctrl = a.u_var || a.cost_increase;
  const bool est = ctrl || a.x_var || a.cov_final;              // the Xh half is asked for
  double *my_p = tm + oSP + jr * NX, *my_x = tm + oSX + jr * NX, *my_f = tm + oF + jr * NU; // the lane's own rows

  struct Knot { double fx[NX], fu[NU], kp[KP], w; };
  const auto load = [&](Knot &k, int t) {
    const double *rec = a.deriv + ((size_t)t * B + b) * L::len;
    ASLR_UNROLL for (int c = 0; c < NX; ++c) k.fx[c] = rec[L::oFx + j * NX + c];
    ASLR_UNROLL for (int c = 0; c < NU; ++c) k.fu[c] = rec[L::oFu + j * NU + c];
    const double *kg = a.kgain + ((size_t)t * B + b) * NK;
    ASLR_UNROLL for (int m = 0; m < KP; ++m) {
      const int idx = jr + m * TEAM;
      k.kp[m] = kg[idx < NK ? idx : NK - 1];
    }
    k.w = a.noise_var ? a.noise_var[((size_t)t * B + b) * NX + j] : 0.0;
  };
  // the team's parts of a trace, added in lane order by every lane
  const auto team_sum = [&](int off, int n) {
    double v = 0.0;
    for (int i = 0; i < n; ++i) v += tm[off + i];
    return v;
  };

  double pm[NX], xm[NX]; // columns j of Pm_t and Xm_t; past the update, of P_t and Xh_t.  Pm_0: the lower triangle of sigma0, mirrored
  ASLR_UNROLL for (int c = 0; c < NX; ++c) {
    const int hi = j > c ? j : c, lo = j > c ? c : j;
    pm[c] = a.sigma0 ? a.sigma0[((size_t)b * NX + hi) * NX + lo] : 0.0;
    xm[c] = 0.0;
  }
  if (jr < ny) tm[oR + jr] = a.meas_var[(size_t)b * ny + jr];
  if (lane < ny) meas[lane] = a.meas[lane];
  // the measurement update of knot t, on pm and xm, and the outputs that are diagonals; run at every knot and once more at T
  const auto update = [&](int t) {
    ASLR_UNROLL for (int c = 0; c < NX; ++c) my_p[c] = pm[c];
    __syncthreads();
    // the factor C of S, a column per trip
    const int ma = meas[ar];
    for (int c = 0; c < ny; ++c) {
      const int mc = meas[c];
      double v = tm[oSP + ma * NX + mc], dv = tm[oSP + mc * NX + mc] + tm[oR + c];
      if (ar == c) v += tm[oR + c];
      for (int k = 0; k < c; ++k) {
        const double ck = tm[oAt + c * NX + k];
        v = fma(-tm[oAt + ar * NX + k], ck, v);
        dv = fma(-ck, ck, dv);
      }
      const double rinv = 1.0 / sqrt(dv);
      if (jr == c) tm[oD + c] = rinv; // (C[c][c] itself is never read: the solves multiply by its inverse)
      if (jr > c && jr < ny) tm[oAt + jr * NX + c] = v * rinv;
      __syncthreads();
    }
    // row j of L = G S^-1: C z = g, then C^T l = z, on the lane's own row of SX
    for (int i = 0; i < ny; ++i) {
      double v = my_p[meas[i]];
      for (int k = 0; k < i; ++k) v = fma(-tm[oAt + i * NX + k], my_x[k], v);
      my_x[i] = v * tm[oD + i];
    }
    for (int i = ny - 1; i >= 0; --i) {
      double v = my_x[i];
      for (int k = i + 1; k < ny; ++k) v = fma(-tm[oAt + k * NX + i], my_x[k], v);
      my_x[i] = v * tm[oD + i];
    }
    if (live && a.kalman_gain) {
      double *o = a.kalman_gain + (((size_t)t * B + b) * NX + j) * ny;
      for (int i = 0; i < ny; ++i) o[i] = my_x[i];
    }
    { // row j of D = L G^T;  P = Pm - D,  Xh = Xm + D
      double d[NX];
      ASLR_UNROLL for (int c = 0; c < NX; ++c) d[c] = 0.0;
      ASLR_SWEEP_LOOP for (int i = 0; i < ny; ++i) {
        const double li = my_x[i];
        const double *g = tm + oSP + meas[i] * NX;
        ASLR_UNROLL for (int c = 0; c < NX; ++c) d[c] = fma(li, g[c], d[c]);
      }
      ASLR_UNROLL for (int c = 0; c < NX; ++c) { pm[c] -= d[c]; xm[c] += d[c]; }
    }
    __syncthreads(); // (every lane has read the columns of Pm and the factor)
    // P and Xh are made symmetric, bit for bit: the lane holds row j of each, taken as column j, and the two triangles agree
    // to rounding only.  The congruence products multiply that difference by |Fx|^2 per knot and the update does not damp
    // it, so left alone it grows without bound over a long horizon (all of a 150-knot arm plan went to NaN with every
    // entry measured).  0.5 (a + b) is the same number from both sides, and the diagonal stays what it is.
    ASLR_UNROLL for (int c = 0; c < NX; ++c) { my_p[c] = pm[c]; my_x[c] = xm[c]; }
    __syncthreads();
    ASLR_UNROLL for (int c = 0; c < NX; ++c) pm[c] = 0.5 * (pm[c] + tm[oSP + c * NX + j]);
    if (est) {
      ASLR_UNROLL for (int c = 0; c < NX; ++c) xm[c] = 0.5 * (xm[c] + tm[oSX + c * NX + j]);
    }
    __syncthreads(); // (every lane has read the other triangle)
    // the columns of P and Xh, which the predict step shares
    ASLR_UNROLL for (int c = 0; c < NX; ++c) { my_p[c] = pm[c]; my_x[c] = xm[c]; }
    {
      // P_t[j][j] and Xh_t[j][j]: the lane's own words (an entry of a register array cannot be picked by a run-time j)
      const double pd = my_p[j], xd = my_x[j];
      if (live && a.est_var) a.est_var[((size_t)t * B + b) * NX + j] = pd;
      if (live && a.x_var) a.x_var[((size_t)t * B + b) * NX + j] = xd + pd;
    }
  };

  double acc = 0.0;
  Knot cur;
  load(cur, 0);
  for (int t = 0; t < T; ++t) {
    ASLR_UNROLL for (int m = 0; m < KP; ++m) {
      const int idx = jr + m * TEAM;
      if (idx < NK) tm[oK + idx] = cur.kp[m];
    }
    ASLR_UNROLL for (int k = 0; k < NU; ++k) my_f[k] = cur.fu[k];
    update(t); // (its first barrier orders these writes too)
    if (est) {
      // rows j, j and ku of the cost blocks are asked for where registers are free to take them, each ahead of a stretch
      // of arithmetic that does not need it: with the next knot's records and two columns in flight there is no room to
      // hold them across the update
      const double *rec = a.deriv + ((size_t)t * B + b) * L::len;
      double lxx[NX], lxu[NU], luu[NU];
      if (ctrl) {
        ASLR_UNROLL for (int c = 0; c < NX; ++c) lxx[c] = rec[L::oLxx + j * NX + c];
      }
      { // row j of A_t
        double av[NX];
        ASLR_UNROLL for (int c = 0; c < NX; ++c) av[c] = cur.fx[c];
        ASLR_SWEEP_LOOP for (int k = 0; k < NU; ++k) {
          const double fk = -my_f[k];
          ASLR_UNROLL for (int c = 0; c < NX; ++c) av[c] = fma(fk, tm[oK + k * NX + c], av[c]);
        }
        if (work) {
          ASLR_UNROLL for (int c = 0; c < NX; ++c) tm[oAt + c * NX + j] = av[c];
        }
      }
      double pxx = 0.0, pxu = 0.0;
      if (ctrl) { // column j of G_t = K_t Xh_t;  the lane's part of tr(Lxx Sigma)
        ASLR_SWEEP_LOOP for (int k = 0; k < NU; ++k) {
          double g = 0.0;
          ASLR_UNROLL for (int i = 0; i < NX; ++i) g = fma(tm[oK + k * NX + i], xm[i], g);
          if (work) tm[oG + k * NX + j] = g;
        }
        ASLR_UNROLL for (int c = 0; c < NX; ++c) pxx = fma(lxx[c], xm[c] + pm[c], pxx);
      }
      __syncthreads();
      if (ctrl) {
        ASLR_UNROLL for (int k = 0; k < NU; ++k) lxu[k] = rec[L::oLxu + j * NU + k];
        ASLR_UNROLL for (int l = 0; l < NU; ++l) luu[l] = rec[L::oLuu + ku * NU + l];
      }

      double y[NX]; // row j of A_t Xh_t
      ASLR_UNROLL for (int c = 0; c < NX; ++c) y[c] = 0.0;
      ASLR_SWEEP_LOOP for (int i = 0; i < NX; ++i) {
        const double ai = tm[oAt + i * NX + j];
        ASLR_UNROLL for (int c = 0; c < NX; ++c) y[c] = fma(ai, tm[oSX + i * NX + c], y[c]);
      }
      if (ctrl) {
        ASLR_UNROLL for (int k = 0; k < NU; ++k) pxu = fma(lxu[k], tm[oG + k * NX + j], pxu);
      }
      __syncthreads(); // (every lane has read the columns of Xh)
      ASLR_UNROLL for (int c = 0; c < NX; ++c) my_x[c] = y[c];
      ASLR_UNROLL for (int c = 0; c < NX; ++c) xm[c] = 0.0; // row j of Xm_{t+1}, taken as the lane's column by symmetry
      ASLR_SWEEP_LOOP for (int i = 0; i < NX; ++i) {
        const double yi = my_x[i];
        ASLR_UNROLL for (int c = 0; c < NX; ++c) xm[c] = fma(yi, tm[oAt + i * NX + c], xm[c]);
      }
      if (ctrl) {
        double gr[NX]; // row ku of G_t
        ASLR_UNROLL for (int c = 0; c < NX; ++c) gr[c] = tm[oG + ku * NX + c];
        double uk = 0.0;
        ASLR_SWEEP_LOOP for (int l = 0; l < NU; ++l) {
          double v = 0.0; // U[ku][l]
          ASLR_UNROLL for (int c = 0; c < NX; ++c) v = fma(gr[c], tm[oK + l * NX + c], v);
          if (l == ku) uk = v;
          my_f[l] = v;
        }
        double puu = 0.0;
        ASLR_UNROLL for (int l = 0; l < NU; ++l) puu = fma(luu[l], my_f[l], puu);
        if (live_u && a.u_var) a.u_var[((size_t)t * B + b) * NU + ku] = uk;
        if (work) { tm[oT + j] = pxx; tm[oT + NX + j] = pxu; }
        if (jr < NU) tm[oT + 2 * NX + ku] = puu;
      }
      __syncthreads(); // (every lane has read A^T; the trace parts are in place)
      if (ctrl) {
        const double txx = team_sum(oT, NX), txu = team_sum(oT + NX, NX), tuu = team_sum(oT + 2 * NX, NU);
        acc = fma(0.5, fma(-2.0, txu, txx) + tuu, acc);
      }
    }

    // ---- Pm_{t+1} = Fx P Fx^T + diag(w_t)
    if (work) {
      ASLR_UNROLL for (int c = 0; c < NX; ++c) tm[oAt + c * NX + j] = cur.fx[c];
    }
    // this knot's records are used up: the next knot's take their registers, in flight while this product is reduced (with
    // two columns per lane there is no room to hold two knots side by side; t = T-1: a repeat, not read)
    const double w = cur.w;
    load(cur, t + 1 < T ? t + 1 : T - 1);
    __syncthreads();
    {
      double y[NX]; // row j of Fx_t P_t
      ASLR_UNROLL for (int c = 0; c < NX; ++c) y[c] = 0.0;
      ASLR_SWEEP_LOOP for (int i = 0; i < NX; ++i) {
        const double fi = tm[oAt + i * NX + j];
        ASLR_UNROLL for (int c = 0; c < NX; ++c) y[c] = fma(fi, tm[oSP + i * NX + c], y[c]);
      }
      __syncthreads(); // (every lane has read the columns of P)
      ASLR_UNROLL for (int c = 0; c < NX; ++c) my_p[c] = y[c];
    }
    ASLR_UNROLL for (int c = 0; c < NX; ++c) pm[c] = 0.0;
    ASLR_SWEEP_LOOP for (int i = 0; i < NX; ++i) {
      const double yi = my_p[i];
      ASLR_UNROLL for (int c = 0; c < NX; ++c) pm[c] = fma(yi, tm[oAt + i * NX + c], pm[c]);
    }
    ASLR_UNROLL for (int c = 0; c < NX; ++c) pm[c] += j == c ? w : 0.0; // (+ 0.0 off the diagonal: the value stays)
    __syncthreads(); // (every lane has read Fx^T: the next knot's factor takes its place)
  }
  update(T); // pm and xm hold P_T and Xh_T
  if (live && a.est_cov_final) {
    double *o = a.est_cov_final + ((size_t)b * NX + j) * NX;
    ASLR_UNROLL for (int c = 0; c < NX; ++c) o[c] = pm[c];
  }
  if (live && a.cov_final) {
    double *o = a.cov_final + ((size_t)b * NX + j) * NX;
    ASLR_UNROLL for (int c = 0; c < NX; ++c) o[c] = xm[c] + pm[c];
  }
  if (a.cost_increase) {
    const double *rec = a.deriv + ((size_t)T * B + b) * L::len;
    double pxx = 0.0;
    ASLR_UNROLL for (int c = 0; c < NX; ++c) pxx = fma(rec[L::oLxx + j * NX + c], xm[c] + pm[c], pxx);
    __syncthreads(); // (the last knot's parts have been read)
    if (work) tm[oT + j] = pxx;
    __syncthreads();
    acc = fma(0.5, team_sum(oT, NX), acc);
    if (br < B && jr == 0) a.cost_increase[b] = acc;
  }
}

template <int NJ, int DAM>
int launch_lqg(const LqgArgs &a, hipStream_t st) {
  return launch_sweep<NJ, DAM>(lqg_kernel<4 * NJ, ModelDims<NJ, DAM>::nu>, a, st);
}

} // namespace aslr
