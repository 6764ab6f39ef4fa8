// aslr_smooth.inc.hpp -- the two sweeps of one iteration of aslr_state_smooth (include/aslr_to_amd_smooth.h): the iterated
// extended Kalman smoother in innovation form, on the records of the calcDiff sweep at the nominal xb = XS.
//
//   filter, t = 0 .. T, from m^-_0 = x0_mean, Pm_0 = sigma0, for the measured entries m (ny of them, variances r):
//     G = Pm[:, m],  S = Pm[m, m] + diag(r) = C C^T,  L = G S^-1,  nu = y - m^-[m],  w = S^-1 nu,
//     mf = m^- + L nu,  P = Pm - L G^T (symmetrised),  nis = nu^T w,
//     m^-' = XNEXT + Fx (mf - xb),  Pm' = Fx P Fx^T + diag(noise_var_t)                                              (t < T)
//     nll = 1/2 sum_t (nis_t + 2 sum_a log C_t[a][a]), the terms added in knot order;   m^-, Pm, L, w -> work
//   adjoint, t = T .. 0, from q^+_T = 0:
//     q = q^+, and at a measured entry  q[m_a] = q^+[m_a] + w[a] - L[:, a] . q^+
//     xs = m^- + Pm q,   q^+_{t-1} = Fx_{t-1}^T q,   step = max |xs - xb|,   XS <- xb + relax (xs - xb)
//
// Two kernels.  The filter wants a column of Pm, a row of Fx and a row of a product in registers (3 nx doubles per lane) and
// a team's matrices in LDS; the adjoint wants three columns per knot (Pm, L, Fx^T) and no LDS at all, and it can only start
// when the filter has reached knot T.  In one kernel the backward half would run with the forward half's LDS allocation
// and the union of both register sets (the compiler's remarks at nx = 28: 272 and 402 registers), for no saved traffic: m^-, Pm, L
// and w of every knot have to go through memory either way.  The launch between them costs microseconds per iteration.
//
// smooth_filter_kernel is the P half of lqg_kernel (aslr_lqg.inc.hpp) -- the team of aslr_sweep_team.hpp, lane j owning
// column j of Pm / P, row j of L and row j of Fx -- with the mean riding along.  The team's LDS, in doubles:
//   SP [TEAM][nx]  a row per lane: its column of Pm (update), then of P, then its row of Fx P
//   SX [TEAM][nx]  a row per lane: its row of the gain -- g, then z, then L[j][:]
//   SV [TEAM][nx]  a row per lane: the innovation's two solves -- nu, then C^-1 nu, then w.  Every lane of the team solves the
//                  same system on its own copy, in the loop trips of its gain's solves: no lane waits for another
//   At [nx][nx]    the Cholesky factor C of S, row a at At + a nx (update); then Fx^T
//   R, D [nx]      the measurement variances of the trajectory (staged once);  1 / C[a][a]
//   M, E, V [nx]   m^-;  mf - xb;  nu
// One knot is lqg_kernel's without the Xh half, and:
//   stage    m^-[j] -> M beside the column of Pm; both -> work                                                    | barrier
//   nu       lane a < ny: nu[a] = y[a] - M[m_a] -> V   (read behind the ny barriers of the factor)
//   solve    C z = nu, C^T w = z in the trips of the lane's own solves;  nis = nu . w;  L^T, w -> work
//   mf       m^-[j] + sum_a L[j][a] nu[a];  mf - xb[j] -> E   (read behind the barrier that follows the staging of Fx^T)
//   m^-'     XNEXT[j] + sum_i Fx[j][i] E[i], in the trips of Y = Fx P, which read Fx^T anyway
// smooth_adjoint_kernel is adjoint_kernel's shape (aslr_adjoint.inc.hpp): lane j holds q[j], an entry of another lane comes by
// a cross-lane shuffle, and a knot is three dot products: over column j of Pm and of Fx, read coalesced (word [i][j]), and, for
// a measured j, over row slot[j] of L^T, nx contiguous words of the lane's own (not coalesced: the filter stores that layout a
// word per lane; an unmeasured lane reads row 0 and drops the result).  Knot t - 1 is loaded while knot t is reduced.  It ends
// in a team max of the lane maxima, NaN winning.
//
// Every sum is ONE fma chain in ascending index order, written with fma(): the unit is built without contraction, so that
// xb + relax (xs - xb) is two roundings like the definition's.  A pivot <= 0 makes 1 / C[c][c] NaN (or inf), and every output
// of that trajectory with it, from that knot on.
#pragma once
#include "aslr_sweep_team.hpp"

namespace aslr {

template <int NX, int NU>
__global__ void __launch_bounds__(64) smooth_filter_kernel(SmoothArgs a) {
  constexpr int NJ = SweepTeam<NX>::NJ, TEAM = SweepTeam<NX>::TEAM, TPW = SweepTeam<NX>::TPW;
  using L = RecLayout<NJ, NU>;
  constexpr int oSP = 0, oSX = oSP + TEAM * NX, oSV = oSX + TEAM * NX, oAt = oSV + TEAM * NX, oR = oAt + NX * NX, oD = oR + NX,
                oM = oD + NX, oE = oM + NX, oV = oE + NX, LEN = (oV + NX + 1) / 2 * 2;
  static_assert(TPW * LEN * sizeof(double) + NX * sizeof(int) <= 65536, "the teams of a wave do not fit the LDS of a block");
  __shared__ __attribute__((aligned(16))) double lds[TPW * LEN];
  __shared__ int meas[NX]; // the measured entries, for every team of the wave
  const int lane = threadIdx.x, jr = lane % TEAM;
  double *tm = lds + (lane / TEAM) * LEN;
  const int br = blockIdx.x * TPW + lane / TEAM;
  const int B = a.B, T = a.T, ny = a.ny;
  const int b = br < B ? br : B - 1, j = jr < NX ? jr : NX - 1; // clamped: every lane reads inside the arrays
  const int ar = jr < ny ? jr : ny - 1;                         // the row of the factor, and the measurement, of this lane
  const bool work = jr < NX;                                    // the idle lanes of a 32-lane team write no shared word
  const bool live = br < B && work, live_y = br < B && jr < ny; // trajectories past B store nothing to memory
  double *my_p = tm + oSP + jr * NX, *my_x = tm + oSX + jr * NX, *my_v = tm + oSV + jr * NX; // the lane's own rows
  const size_t N = (size_t)(T + 1) * B;
  double *w_pm = a.work, *w_lt = w_pm + N * NX * NX, *w_mm = w_lt + N * NX * ny, *w_w = w_mm + N * NX;

  struct Knot { double fx[NX], w, xb, xn; };
  const auto load = [&](Knot &k, int t) {
    const double *rec = a.deriv + ((size_t)t * B + b) * L::len;
    ASLR_UNROLL for (int c = 0; c < NX; ++c) k.fx[c] = rec[L::oFx + j * NX + c];
    k.w = a.noise_var ? a.noise_var[((size_t)t * B + b) * NX + j] : 0.0;
    k.xb = a.xs[((size_t)t * B + b) * NX + j];
    k.xn = a.xnext[((size_t)t * B + b) * NX + j];
  };

  double pm[NX]; // column j of Pm_t; past the update, of P_t.  Pm_0: the lower triangle of sigma0, mirrored
  ASLR_UNROLL for (int c = 0; c < NX; ++c) {
    const int hi = j > c ? j : c, lo = j > c ? c : j;
    pm[c] = a.sigma0 ? a.sigma0[((size_t)b * NX + hi) * NX + lo] : 0.0;
  }
  double mm = a.x0_mean[(size_t)b * NX + j]; // m^-_t[j]
  double mf = 0.0;                           // m_t[j]
  double acc = 0.0;                          // the negative log-likelihood so far
  if (jr < ny) tm[oR + jr] = a.meas_var[(size_t)b * ny + jr];
  if (lane < ny) meas[lane] = a.meas[lane];
  // the measurement update of knot t with the lane's measurement y, on pm and mm -> mf; what the adjoint sweep reads and the
  // per-knot outputs
  const auto update = [&](int t, double y) {
    const size_t kn = (size_t)t * B + b;
    ASLR_UNROLL for (int c = 0; c < NX; ++c) my_p[c] = pm[c];
    if (work) tm[oM + j] = mm;
    if (live) {
      ASLR_UNROLL for (int c = 0; c < NX; ++c) w_pm[kn * NX * NX + c * NX + j] = pm[c];
      w_mm[kn * NX + j] = mm;
    }
    __syncthreads();
    const int ma = meas[ar];
    if (jr < ny) tm[oV + jr] = y - tm[oM + ma];
    // the factor C of S, a column per trip, and the sum of log C[c][c]
    double ld = 0.0;
    for (int c = 0; c < ny; ++c) {
      const int mc = meas[c];
      double v = tm[oSP + ma * NX + mc], dv = tm[oSP + mc * NX + mc] + tm[oR + c];
      if (ar == c) v += tm[oR + c];
      for (int k = 0; k < c; ++k) {
        const double ck = tm[oAt + c * NX + k];
        v = fma(-tm[oAt + ar * NX + k], ck, v);
        dv = fma(-ck, ck, dv);
      }
      const double cd = sqrt(dv), rinv = 1.0 / cd;
      ld += log(cd);
      if (jr == c) tm[oD + c] = rinv; // (C[c][c] itself is never read again: the solves multiply by its inverse)
      if (jr > c && jr < ny) tm[oAt + jr * NX + c] = v * rinv;
      __syncthreads();
    }
    // row j of L = G S^-1 and w = S^-1 nu: C z = g, then C^T l = z, on the lane's own rows of SX and SV
    for (int i = 0; i < ny; ++i) {
      double v = my_p[meas[i]], u = tm[oV + i];
      for (int k = 0; k < i; ++k) {
        const double ck = tm[oAt + i * NX + k];
        v = fma(-ck, my_x[k], v);
        u = fma(-ck, my_v[k], u);
      }
      my_x[i] = v * tm[oD + i];
      my_v[i] = u * tm[oD + i];
    }
    for (int i = ny - 1; i >= 0; --i) {
      double v = my_x[i], u = my_v[i];
      for (int k = i + 1; k < ny; ++k) {
        const double ck = tm[oAt + k * NX + i];
        v = fma(-ck, my_x[k], v);
        u = fma(-ck, my_v[k], u);
      }
      my_x[i] = v * tm[oD + i];
      my_v[i] = u * tm[oD + i];
    }
    double nis = 0.0, lv = 0.0; // nu . w;  (L nu)[j]
    for (int i = 0; i < ny; ++i) {
      const double ni = tm[oV + i];
      nis = fma(ni, my_v[i], nis);
      lv = fma(my_x[i], ni, lv);
    }
    mf = mm + lv;
    acc = acc + 0.5 * (nis + 2.0 * ld);
    if (live) {
      for (int i = 0; i < ny; ++i) w_lt[(kn * ny + i) * NX + j] = my_x[i];
    }
    if (live_y) w_w[kn * ny + jr] = my_v[jr];
    { // row j of D = L G^T;  P = Pm - D
      double d[NX];
      ASLR_UNROLL for (int c = 0; c < NX; ++c) d[c] = 0.0;
      ASLR_SWEEP_LOOP for (int i = 0; i < ny; ++i) {
        const double li = my_x[i];
        const double *g = tm + oSP + meas[i] * NX;
        ASLR_UNROLL for (int c = 0; c < NX; ++c) d[c] = fma(li, g[c], d[c]);
      }
      ASLR_UNROLL for (int c = 0; c < NX; ++c) pm[c] -= d[c];
    }
    __syncthreads(); // (every lane has read the columns of Pm, the factor and nu)
    // P is made symmetric, bit for bit, as lqg_kernel does and for its reason: (a + b) / 2 of the two triangles
    ASLR_UNROLL for (int c = 0; c < NX; ++c) my_p[c] = pm[c];
    __syncthreads();
    ASLR_UNROLL for (int c = 0; c < NX; ++c) pm[c] = 0.5 * (pm[c] + tm[oSP + c * NX + j]);
    __syncthreads(); // (every lane has read the other triangle)
    ASLR_UNROLL for (int c = 0; c < NX; ++c) my_p[c] = pm[c]; // the columns of P, which the predict step shares
    if (live && a.est_var) a.est_var[kn * NX + j] = my_p[j]; // (an entry of a register array cannot be picked by a run-time j)
    if (live && a.x_filt) a.x_filt[kn * NX + j] = mf;
    if (br < B && jr == 0 && a.nis) a.nis[kn] = nis;
  };

  Knot cur;
  load(cur, 0);
  double y = a.ys[(size_t)b * ny + ar];
  for (int t = 0; t < T; ++t) {
    update(t, y);
    // ---- m^-_{t+1} = XNEXT_t + Fx (m_t - xb_t),  Pm_{t+1} = Fx P Fx^T + diag(w_t)
    if (work) {
      tm[oE + j] = mf - cur.xb;
      ASLR_UNROLL for (int c = 0; c < NX; ++c) tm[oAt + c * NX + j] = cur.fx[c];
    }
    // this knot's records are used up: the next knot's take their registers, in flight while the product is reduced
    // (t = T-1: a repeat of the records, not read; the measurement of knot T is)
    const double w = cur.w, xn = cur.xn;
    load(cur, t + 1 < T ? t + 1 : T - 1);
    y = a.ys[((size_t)(t + 1) * B + b) * ny + ar];
    __syncthreads();
    double mp = 0.0; // (Fx (m - xb))[j]
    {
      double yr[NX]; // row j of Fx_t P_t
      ASLR_UNROLL for (int c = 0; c < NX; ++c) yr[c] = 0.0;
      ASLR_SWEEP_LOOP for (int i = 0; i < NX; ++i) {
        const double fi = tm[oAt + i * NX + j];
        mp = fma(fi, tm[oE + i], mp);
        ASLR_UNROLL for (int c = 0; c < NX; ++c) yr[c] = fma(fi, tm[oSP + i * NX + c], yr[c]);
      }
      __syncthreads(); // (every lane has read the columns of P)
      ASLR_UNROLL for (int c = 0; c < NX; ++c) my_p[c] = yr[c];
    }
    ASLR_UNROLL for (int c = 0; c < NX; ++c) pm[c] = 0.0;
    ASLR_SWEEP_LOOP for (int i = 0; i < NX; ++i) {
      const double yi = my_p[i];
      ASLR_UNROLL for (int c = 0; c < NX; ++c) pm[c] = fma(yi, tm[oAt + i * NX + c], pm[c]);
    }
    ASLR_UNROLL for (int c = 0; c < NX; ++c) pm[c] += j == c ? w : 0.0; // (+ 0.0 off the diagonal: the value stays)
    mm = xn + mp;
    __syncthreads(); // (every lane has read Fx^T: the next knot's factor takes its place)
  }
  update(T, y);
  if (br < B && jr == 0 && a.neg_log_lik) a.neg_log_lik[b] = acc;
}

template <int NX, int NU>
__global__ void __launch_bounds__(64) smooth_adjoint_kernel(SmoothArgs a) {
  constexpr int NJ = SweepTeam<NX>::NJ, TEAM = SweepTeam<NX>::TEAM, TPW = SweepTeam<NX>::TPW;
  using L = RecLayout<NJ, NU>;
  const int lane = threadIdx.x, jr = lane % TEAM;
  const int br = blockIdx.x * TPW + lane / TEAM;
  const int B = a.B, T = a.T, ny = a.ny;
  const bool live = br < B && jr < NX; // trajectories past B and the idle lanes of a 32-lane team store nothing
  const int b = br < B ? br : B - 1, j = jr < NX ? jr : NX - 1; // clamped: every lane reads inside the arrays
  const int sj = a.slot[j];
  const bool measured = sj >= 0;
  const int aj = measured ? sj : 0; // the column of L this lane reduces (an unmeasured lane: column 0, dropped)
  const double relax = a.relax;
  const size_t N = (size_t)(T + 1) * B;
  const double *w_pm = a.work, *w_lt = w_pm + N * NX * NX, *w_mm = w_lt + N * NX * ny, *w_w = w_mm + N * NX;

  struct Knot { double pm[NX], lt[NX], fx[NX], mm, w, xb; };
  const auto load = [&](Knot &k, int t) {
    const size_t kn = (size_t)t * B + b;
    ASLR_UNROLL for (int c = 0; c < NX; ++c) k.pm[c] = w_pm[kn * NX * NX + c * NX + j];
    ASLR_UNROLL for (int i = 0; i < NX; ++i) k.lt[i] = w_lt[(kn * ny + aj) * NX + i];
    const double *rec = a.deriv + ((size_t)(t > 0 ? t - 1 : 0) * B + b) * L::len; // Fx_{t-1}: column j
    ASLR_UNROLL for (int i = 0; i < NX; ++i) k.fx[i] = rec[L::oFx + i * NX + j];
    k.mm = w_mm[kn * NX + j];
    k.w = w_w[kn * ny + aj];
    k.xb = a.xs[kn * NX + j];
  };

  double qp = 0.0, smax = 0.0; // q^+_t[j];  the lane's max |xs - xb| so far
  Knot cur;
  load(cur, T);
  for (int t = T; t >= 0; --t) {
    Knot nxt;
    load(nxt, t > 0 ? t - 1 : 0); // in flight while knot t is reduced (t = 0: a repeat, dropped)
    double dot = 0.0; // L[:, aj] . q^+
    ASLR_UNROLL for (int i = 0; i < NX; ++i) dot = fma(cur.lt[i], __shfl(qp, i, TEAM), dot);
    const double q = measured ? (qp + cur.w) - dot : qp;
    double pq = 0.0, g = 0.0; // (Pm q)[j];  (Fx_{t-1}^T q)[j]
    ASLR_UNROLL for (int c = 0; c < NX; ++c) {
      const double qc = __shfl(q, c, TEAM);
      pq = fma(cur.pm[c], qc, pq);
      g = fma(cur.fx[c], qc, g);
    }
    const double xs = cur.mm + pq, dx = xs - cur.xb, d = fabs(dx);
    smax = (d > smax || d != d) ? d : smax; // a NaN stays
    if (live) {
      const size_t o = ((size_t)t * B + b) * NX + j;
      if (a.xs_smooth) a.xs_smooth[o] = xs;
      a.xs[o] = cur.xb + relax * dx;
    }
    qp = g;
    cur = nxt;
  }
  if (a.step_norm) {
    double sn = __shfl(smax, 0, TEAM);
    ASLR_UNROLL for (int i = 1; i < NX; ++i) {
      const double v = __shfl(smax, i, TEAM);
      sn = (v > sn || v != v) ? v : sn;
    }
    if (br < B && jr == 0) a.step_norm[b] = sn;
  }
}

template <int NJ, int DAM>
int launch_smooth_filter(const SmoothArgs &a, hipStream_t st) {
  return launch_sweep<NJ, DAM>(smooth_filter_kernel<4 * NJ, ModelDims<NJ, DAM>::nu>, a, st);
}
template <int NJ, int DAM>
int launch_smooth_adjoint(const SmoothArgs &a, hipStream_t st) {
  return launch_sweep<NJ, DAM>(smooth_adjoint_kernel<4 * NJ, ModelDims<NJ, DAM>::nu>, a, st);
}

} // namespace aslr
