// aslr_covariance.inc.hpp -- the closed-loop covariance sweep behind aslr_policy_covariance (include/aslr_to_amd_cov.h).
//
//   A_t = Fx_t - Fu_t K_t,   Sigma_{t+1} = A_t Sigma_t A_t^T + diag(w_t),   G_t = K_t Sigma_t,   U_t = G_t K_t^T      (t = 0 .. T-1)
//   cost_increase = 1/2 sum_t [tr(Lxx_t Sigma_t) - 2 tr(Lxu_t G_t) + tr(Luu_t U_t)] + 1/2 tr(Lxx_T Sigma_T)
//
// No model evaluation: the sweep reads Fx, Fu (and Lxx, Lxu, Luu for the control terms) of every record and KGAIN.
//
// Decomposition: one team of lanes per trajectory (aslr_sweep_team.hpp).  Lane j owns row j of A_t and column j of
// Sigma_t (its registers); row j of Fx and of Fu are contiguous words of the record.  What a team shares -- K_t, the
// columns of Sigma_t, the rows of A_t, G_t -- is staged per team in LDS and read back at team-uniform addresses (broadcast
// reads, two operands per 16-byte read): a lane needs ALL of Sigma and ALL of A every knot, nx^2 operands each, which as
// cross-lane shuffles would be 2 nx^2 two-dword permutes per knot against nx^2 / 2 wide reads.  One knot:
//   stage   K_t (the team's lanes load nu nx / TEAM words each), column j of Sigma, row j of Fu -> LDS            | barrier
//   1       a_j[c]   = Fx[j][c] - sum_k Fu[j][k] K[k][c]            -> LDS, transposed (At[c][j])
//   (ctrl)  G[k][j]  = sum_i K[k][i] Sigma[i][j]                    -> LDS                                        | barrier
//   2       Y[j][c]  = sum_i a_j[i] Sigma[i][c]                                                                  | barrier
//           (row j of Y -> LDS, over the lane's own column of Sigma)
//   3       S'[j][c] = sum_i Y[j][i] A[c][i]      the new row j, taken as the lane's column of the next knot by symmetry
//   (ctrl)  the lane's parts of tr(Lxx Sigma) and tr(Lxu G);  lane k < nu: U[k][l] = sum_c G[k][c] K[l][c],
//           u_var[k] = U[k][k], its part of tr(Luu U);  the parts -> LDS | barrier | every lane adds them in lane order
//   4       S'[j][j] += w_t[j]
// Every sum is ONE fma chain in ascending index order.  The long sums are loops over the summation index (or over the row
// of K) that stay loops, two steps per trip: their per-step operand -- Fu[j][k], a_j[i], Y[j][i] -- is the lane's own
// word in LDS, because an entry of a register array cannot be picked by a loop counter.  Unrolled in full, the 2 nx^2
// independent chains of a knot let the scheduler hoist every LDS read, and the nx = 28 kernels spilled 11 KB per lane.
// The control terms (ctrl) are computed only when u_var or cost_increase is asked for; they do not enter Sigma, so every
// output has the same bits whichever others are asked for.
//
// Arithmetic: 2 nx^2 + nu nx fma per lane and knot (+ 2 nu nx with the control terms) on a serial chain of T knots; the records
// of knot t + 1 are loaded while knot t is reduced.  Measured (profiles/covariance/README.md), the sweep is bound by the
// LDS round trips of that chain -- write, barrier, broadcast reads that the fma of the same trip wait for -- at the one or
// two waves per CU these batch sizes give, not by the fma rate.
#pragma once
#include "aslr_sweep_team.hpp"

namespace aslr {

template <int NX, int NU>
__global__ void __launch_bounds__(64) covariance_kernel(CovarianceArgs a) {
  constexpr int NJ = SweepTeam<NX>::NJ, TEAM = SweepTeam<NX>::TEAM, TPW = SweepTeam<NX>::TPW;
  constexpr int NK = NU * NX, KP = (NK + TEAM - 1) / TEAM; // words of K_t, and how many of them one lane of the team loads
  using L = RecLayout<NJ, NU>;
  // a team's LDS: S [TEAM][nx] a row per lane: its column of Sigma, then its row of Y;  At [nx][nx] A transposed;  K, G [nu][nx];
  // F [TEAM][nu] a row per lane: its row of Fu, then its row of U;  P [nx + nx + nu] the trace parts
  constexpr int oS = 0, oAt = oS + TEAM * NX, oK = oAt + NX * NX, oG = oK + NK, oF = oG + NK, oP = oF + TEAM * NU,
                LEN = (oP + 2 * NX + NU + 1) / 2 * 2;
  __shared__ __attribute__((aligned(16))) double lds[TPW * LEN];
  const int lane = threadIdx.x, jr = lane % TEAM;
  double *tm = lds + (lane / TEAM) * LEN;
  const int br = blockIdx.x * TPW + lane / TEAM;
  const int B = a.B, T = a.T;
  const int b = br < B ? br : B - 1, j = jr < NX ? jr : NX - 1; // clamped: every lane reads inside the arrays
  const int ku = jr < NU ? jr : NU - 1;                         // the row of U this lane reduces
  const bool work = jr < NX;                                    // the idle lanes of a 32-lane team write no shared word
  const bool live = br < B && work, live_u = br < B && jr < NU; // trajectories past B store nothing to memory
  const bool ctrl = a.u_var || a.cost_increase;
  double *my_s = tm + oS + jr * NX, *my_f = tm + oF + jr * NU;  // the lane's own rows (idle lanes included: nobody reads theirs)

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
  const auto store = [&](const double (&s)[NX], double d, int t) {
    if (!live) return;
    if (a.x_var) a.x_var[((size_t)t * B + b) * NX + j] = d;
    if (a.cov) {
      double *o = a.cov + (((size_t)t * B + b) * NX + j) * NX;
      ASLR_UNROLL for (int c = 0; c < NX; ++c) o[c] = s[c];
    }
  };
  // the team's parts of a trace, added in lane order by every lane
  const auto team_sum = [&](int off, int n) {
    double v = 0.0;
    for (int i = 0; i < n; ++i) v += tm[off + i];
    return v;
  };

  double s[NX]; // column j of Sigma_t.  Sigma_0: the lower triangle of sigma0, mirrored
  ASLR_UNROLL for (int c = 0; c < NX; ++c) {
    const int hi = j > c ? j : c, lo = j > c ? c : j;
    s[c] = a.sigma0 ? a.sigma0[((size_t)b * NX + hi) * NX + lo] : 0.0;
  }
  // Sigma_t[j][j], carried beside the column (an entry of a register array cannot be picked by a run-time j): the same fma
  // chain on the same operands as s[j], so it has the bits of s[j]
  double d = a.sigma0 ? a.sigma0[((size_t)b * NX + j) * NX + j] : 0.0;
  double acc = 0.0;
  Knot cur;
  load(cur, 0);
  for (int t = 0; t < T; ++t) {
    Knot nxt;
    load(nxt, t + 1 < T ? t + 1 : T - 1); // in flight while knot t is reduced (t = T-1: a repeat, dropped)
    const double *rec = a.deriv + ((size_t)t * B + b) * L::len;
    double lxx[NX], lxu[NU], luu[NU]; // rows j, j and ku of the cost blocks: asked for here, used after step 2
    if (ctrl) {
      ASLR_UNROLL for (int c = 0; c < NX; ++c) lxx[c] = rec[L::oLxx + j * NX + c];
      ASLR_UNROLL for (int k = 0; k < NU; ++k) lxu[k] = rec[L::oLxu + j * NU + k];
      ASLR_UNROLL for (int l = 0; l < NU; ++l) luu[l] = rec[L::oLuu + ku * NU + l];
    }
    store(s, d, t);
    ASLR_UNROLL for (int m = 0; m < KP; ++m) {
      const int idx = jr + m * TEAM;
      if (idx < NK) tm[oK + idx] = cur.kp[m];
    }
    ASLR_UNROLL for (int c = 0; c < NX; ++c) my_s[c] = s[c];
    ASLR_UNROLL for (int k = 0; k < NU; ++k) my_f[k] = cur.fu[k];
    __syncthreads();

    { // 1: row j of A_t
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
    if (ctrl) { // column j of G_t
      ASLR_SWEEP_LOOP for (int k = 0; k < NU; ++k) {
        double g = 0.0;
        ASLR_UNROLL for (int i = 0; i < NX; ++i) g = fma(tm[oK + k * NX + i], s[i], g);
        if (work) tm[oG + k * NX + j] = g;
      }
    }
    __syncthreads();

    double y[NX]; // 2: row j of A_t Sigma_t
    ASLR_UNROLL for (int c = 0; c < NX; ++c) y[c] = 0.0;
    ASLR_SWEEP_LOOP for (int i = 0; i < NX; ++i) {
      const double ai = tm[oAt + i * NX + j];
      ASLR_UNROLL for (int c = 0; c < NX; ++c) y[c] = fma(ai, tm[oS + i * NX + c], y[c]);
    }
    double pxx = 0.0, pxu = 0.0;
    if (ctrl) {
      ASLR_UNROLL for (int c = 0; c < NX; ++c) pxx = fma(lxx[c], s[c], pxx);
      ASLR_UNROLL for (int k = 0; k < NU; ++k) pxu = fma(lxu[k], tm[oG + k * NX + j], pxu);
    }
    __syncthreads(); // (every lane has read the columns of Sigma)
    ASLR_UNROLL for (int c = 0; c < NX; ++c) my_s[c] = y[c];

    // 3: row j of Sigma_{t+1} before the noise, and its entry j
    ASLR_UNROLL for (int c = 0; c < NX; ++c) s[c] = 0.0;
    d = 0.0;
    ASLR_SWEEP_LOOP for (int i = 0; i < NX; ++i) {
      const double yi = my_s[i];
      ASLR_UNROLL for (int c = 0; c < NX; ++c) s[c] = fma(yi, tm[oAt + i * NX + c], s[c]);
      d = fma(yi, tm[oAt + i * NX + j], d);
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
      if (work) { tm[oP + j] = pxx; tm[oP + NX + j] = pxu; }
      if (jr < NU) tm[oP + 2 * NX + ku] = puu;
      __syncthreads();
      const double txx = team_sum(oP, NX), txu = team_sum(oP + NX, NX), tuu = team_sum(oP + 2 * NX, NU);
      acc = fma(0.5, fma(-2.0, txu, txx) + tuu, acc);
    }
    ASLR_UNROLL for (int c = 0; c < NX; ++c) s[c] += j == c ? cur.w : 0.0; // (+ 0.0 off the diagonal: the value stays)
    d += cur.w;
    cur = nxt;
  }
  store(s, d, T);
  if (live && a.cov_final) {
    double *o = a.cov_final + ((size_t)b * NX + j) * NX;
    ASLR_UNROLL for (int c = 0; c < NX; ++c) o[c] = s[c];
  }
  if (a.cost_increase) {
    const double *rec = a.deriv + ((size_t)T * B + b) * L::len;
    double pxx = 0.0;
    ASLR_UNROLL for (int c = 0; c < NX; ++c) pxx = fma(rec[L::oLxx + j * NX + c], s[c], pxx);
    __syncthreads(); // (the last knot's parts have been read)
    if (work) tm[oP + j] = pxx;
    __syncthreads();
    acc = fma(0.5, team_sum(oP, NX), acc);
    if (br < B && jr == 0) a.cost_increase[b] = acc;
  }
}

template <int NJ, int DAM>
int launch_covariance(const CovarianceArgs &a, hipStream_t st) {
  return launch_sweep<NJ, DAM>(covariance_kernel<4 * NJ, ModelDims<NJ, DAM>::nu>, a, st);
}

} // namespace aslr
