// aslr_plant_sens.inc.hpp -- the tangent (forward sensitivity) sweep behind aslr_policy_plant_sensitivity
// (include/aslr_to_amd_plant_sens.h): the derivative of the closed-loop trajectory in the plant's spring stiffness and motor
// inertia, the forward counterpart of the adjoint sweep (aslr_adjoint.inc.hpp).
//
//   S_0 = 0,   V_t = K_t S_t,   S_{t+1} = Fx_t S_t - Fu_t V_t + G_t                        (t = 0 .. T-1;  S_t = dx_t/dtheta, [nx][np])
//   G_K[:, c] = -(delta_c / K_c) (Fx_t[:, nj+c] - e_{nj+c}),   delta = q_l - q_m of knot t          (the adjoint sweep's closed forms:
//   G_B[:, c] = -(1 / B_c) D_c (dt e_{nj+c} + e_{3nj+c}),      D = xnext_t[3nj+c] - x_t[3nj+c]       no second model evaluation)
//   dJ/dtheta_p = sum_{t<T} (Lx_t^T S_t[:, p] - Lu_t^T V_t[:, p]) + Lx_T^T S_T[:, p]
//   x_var_t[i] = sum_p S_t[i][p]^2 var_p,   u_var_t[k] = sum_p V_t[k][p]^2 var_p
//
// Columns of S never mix, so the stiffness columns exist only in the STIFF instantiations (picked when a stiffness quantity
// is asked for): np = 2 nj with them (stiffness first), nj without, and a motor-inertia column goes through the same
// operations on the same operands in both.
//
// Decomposition: one team of lanes per trajectory (aslr_sweep_team.hpp).  Lane j owns row j of S_t (np <= 14
// registers) and holds rows j of Fx_t and Fu_t.  What the team shares is staged in its LDS, two buffers used in turn so that
// a knot needs two barriers, not three.  One knot:
//   stage   K_t (nu nx / TEAM words per lane), row j of S, Lx[j], Lu[k]; lane nj + c: -(delta_c / K_c), -(D_c / B_c)   | barrier
//   1       V[k][p] = sum_i K[k][i] S[i][p], the nu np entries dealt round the team's lanes -> LDS
//           lane p < np: sum_i Lx[i] S[i][p]  (the team-wide sum over the rows, in lane order)                            | barrier
//   2       S'[j][p] = sum_i Fx[j][i] S[i][p], continued as sum_k (-Fu[j][k]) V[k][p], then + G[j][p]
//           lane k < nu: u_var[k];  lane p < np: sum_k Lu[k] V[k][p], and its cost term joins the lane's running sum
// Every sum is ONE fma chain in ascending index order; rows of S and of V are read back at team-uniform addresses
// (broadcast reads).  The two long sums of step 2 are loops over the summation index that stay loops, two steps per trip,
// with Fx[j][i] / Fu[j][k] read from the lane's own words in LDS, as in the covariance sweep and for its reason: unrolled
// in full over register operands, the scheduler hoisted the LDS reads of all (nx + nu) np chains and the nx = 28 kernels
// spilled 1 to 3 KB per lane.  As built no kernel uses scratch.  The outputs that do not feed S (x_var, u_var, dcost) are computed only when asked for, so every
// output has the same bits whichever others are asked for.
//
// Arithmetic: (nx + nu) np fma per lane and knot for S', nu np nx / TEAM for V: about a third of the covariance sweep's.  A
// serial chain of T knots; the records of knot t + 1 are loaded while knot t is reduced.
#pragma once
#include "aslr_sweep_team.hpp"

namespace aslr {

template <int NX, int NU, bool STIFF>
__global__ void __launch_bounds__(64) plant_sens_kernel(PlantSensArgs a) {
  constexpr int NJ = SweepTeam<NX>::NJ, TEAM = SweepTeam<NX>::TEAM, TPW = SweepTeam<NX>::TPW;
  constexpr int NP = STIFF ? 2 * NJ : NJ, P0 = NP - NJ;     // columns of S; the first motor-inertia column
  constexpr int NK = NU * NX, KP = (NK + TEAM - 1) / TEAM;  // words of K_t, and how many of them one lane of the team loads
  constexpr int NV = NU * NP, VP = (NV + TEAM - 1) / TEAM;  // entries of V_t, and how many of them one lane reduces
  using L = RecLayout<NJ, NU>;
  // one buffer of a team: S [nx][np], K [nu][nx], V [nu][np], Lx [nx], Lu [nu], Gp [2 nj] the scalar factors of G_K and G_B;
  // a team: two buffers, var [np] and F [TEAM][nx + nu] a row per lane: its rows of Fx_t and Fu_t, which nobody else reads
  constexpr int oS = 0, oK = oS + NX * NP, oV = oK + NK, oLx = oV + NV, oLu = oLx + NX, oGp = oLu + NU,
                BUF = (oGp + 2 * NJ + 1) / 2 * 2, oVar = 2 * BUF, oF = (oVar + NP + 1) / 2 * 2, LEN = oF + TEAM * (NX + NU);
  __shared__ __attribute__((aligned(16))) double lds[TPW * LEN];
  const int lane = threadIdx.x, jr = lane % TEAM;
  double *tm = lds + (lane / TEAM) * LEN;
  const int br = blockIdx.x * TPW + lane / TEAM;
  const int B = a.B, T = a.T;
  const int b = br < B ? br : B - 1, j = jr < NX ? jr : NX - 1; // clamped: every lane reads inside the arrays
  const int ku = jr < NU ? jr : NU - 1;                         // the control whose u_var this lane reduces
  const int pc = jr < NP ? jr : NP - 1;                         // the column whose cost derivative this lane sums
  const bool work = jr < NX;                                    // the idle lanes of a 32-lane team write no row of S
  const bool live = br < B && work, live_u = br < B && jr < NU, live_p = br < B && jr < NP;
  const bool motor = j >= NJ && j < 2 * NJ; // lane nj + jj: the parameter factors of joint jj
  const int jj = motor ? j - NJ : 0;
  const bool want_cost = a.dcost_k || a.dcost_b;
  double *my_f = tm + oF + jr * (NX + NU);

  // 1 / K_jj and 1 / B_jj of this lane's joint, per action model (one value for all of them with a table): as adjoint_kernel
  double rk[ASLR_MAX_MODELS], bi[ASLR_MAX_MODELS];
  double tk = 0.0, tv = 0.0;
  if (a.traj_params) { tk = a.traj_params[(size_t)jj * B + b]; tv = a.traj_params[(size_t)(NJ + jj) * B + b]; }
  ASLR_UNROLL for (int m = 0; m < ASLR_MAX_MODELS; ++m) {
    double k = a.plant.K[m][0], v = a.plant.Binv[m][0];
    ASLR_UNROLL for (int c = 1; c < NJ; ++c)
      if (jj == c) { k = a.plant.K[m][c]; v = a.plant.Binv[m][c]; }
    if (a.traj_params) { k = tk; v = tv; }
    rk[m] = k != 0.0 ? 1.0 / k : 0.0;
    bi[m] = v;
  }
  // the entries of V this lane reduces: (row of K, column of S), clamped
  int vk[VP], vp[VP];
  ASLR_UNROLL for (int m = 0; m < VP; ++m) {
    const int idx = jr + m * TEAM, ic = idx < NV ? idx : NV - 1;
    vk[m] = ic / NP; vp[m] = ic % NP;
  }
  { // variance of column pc (0 where its array is not given)
    const double *src = pc < P0 ? a.stiffness_var : a.motor_inertia_var;
    const int row = pc < P0 ? pc : pc - P0;
    const double v = src ? src[(size_t)row * B + b] : 0.0;
    if (jr < NP) tm[oVar + jr] = v;
  }
  __syncthreads();

  struct Knot { double fx[NX], fu[NU], kp[KP], lx, lu, ql, qm, vm, vmn; };
  const auto load = [&](Knot &k, int t) {
    const double *rec = a.deriv + ((size_t)t * B + b) * L::len;
    ASLR_UNROLL for (int c = 0; c < NX; ++c) k.fx[c] = rec[L::oFx + j * NX + c];
    ASLR_UNROLL for (int c = 0; c < NU; ++c) k.fu[c] = rec[L::oFu + j * NU + c];
    k.lx = rec[L::oLx + j]; k.lu = rec[L::oLu + ku];
    const double *kg = a.kgain + ((size_t)t * B + b) * NK;
    ASLR_UNROLL for (int m = 0; m < KP; ++m) {
      const int idx = jr + m * TEAM;
      k.kp[m] = kg[idx < NK ? idx : NK - 1];
    }
    const size_t xo = ((size_t)t * B + b) * NX;
    k.ql = a.xs[xo + jj]; k.qm = a.xs[xo + NJ + jj];
    k.vm = a.xs[xo + 3 * NJ + jj]; k.vmn = a.xnext[xo + 3 * NJ + jj];
  };
  const auto store = [&](const double (&s)[NP], int t) {
    if (!live) return;
    const size_t row = ((size_t)t * B + b) * NX + j;
    if (a.x_var) {
      double v = 0.0;
      ASLR_UNROLL for (int p = 0; p < NP; ++p) v = fma(s[p] * s[p], tm[oVar + p], v);
      a.x_var[row] = v;
    }
    if (STIFF && a.dx_k) {
      ASLR_UNROLL for (int c = 0; c < P0; ++c) a.dx_k[row * NJ + c] = s[c];
    }
    if (a.dx_b) {
      ASLR_UNROLL for (int c = 0; c < NJ; ++c) a.dx_b[row * NJ + c] = s[P0 + c];
    }
  };
  const auto stage_rows = [&](double *bf, const double (&s)[NP], double lx) {
    if (!work) return;
    ASLR_UNROLL for (int p = 0; p < NP; ++p) bf[oS + j * NP + p] = s[p];
    bf[oLx + j] = lx;
  };
  // sum_i Lx[i] S[i][pc]: the team's rows in lane order
  const auto cost_rows = [&](const double *bf) {
    double v = 0.0;
    for (int i = 0; i < NX; ++i) v = fma(bf[oLx + i], bf[oS + i * NP + pc], v);
    return v;
  };

  double s[NP]; // row j of S_t
  ASLR_UNROLL for (int p = 0; p < NP; ++p) s[p] = 0.0;
  double acc = 0.0; // dJ/dtheta of column pc
  Knot cur;
  load(cur, 0);
  for (int t = 0; t < T; ++t) {
    Knot nxt;
    load(nxt, t + 1 < T ? t + 1 : T - 1); // in flight while knot t is reduced (t = T-1: a repeat, dropped)
    double *bf = tm + (t & 1) * BUF;
    store(s, t);
    const int mi = knot_model(a.node_model, t);
    double dt = a.plant.dt[0], rkm = rk[0], bim = bi[0];
    ASLR_UNROLL for (int m = 1; m < ASLR_MAX_MODELS; ++m)
      if (mi == m) { dt = a.plant.dt[m]; rkm = rk[m]; bim = bi[m]; }
    ASLR_UNROLL for (int m = 0; m < KP; ++m) {
      const int idx = jr + m * TEAM;
      if (idx < NK) bf[oK + idx] = cur.kp[m];
    }
    stage_rows(bf, s, cur.lx);
    ASLR_UNROLL for (int c = 0; c < NX; ++c) my_f[c] = cur.fx[c];
    ASLR_UNROLL for (int k = 0; k < NU; ++k) my_f[NX + k] = cur.fu[k];
    if (jr < NU) bf[oLu + jr] = cur.lu;
    if (motor && work) {
      const double delta = cur.ql - cur.qm, D = cur.vmn - cur.vm;
      bf[oGp + jj] = -(delta * rkm);
      bf[oGp + NJ + jj] = -(bim * D);
    }
    __syncthreads();

    ASLR_UNROLL for (int m = 0; m < VP; ++m) { // 1: this lane's entries of V_t
      double v = 0.0;
      _Pragma("unroll 4") for (int i = 0; i < NX; ++i) v = fma(bf[oK + vk[m] * NX + i], bf[oS + i * NP + vp[m]], v);
      if (jr + m * TEAM < NV) bf[oV + jr + m * TEAM] = v;
    }
    double cx = 0.0;
    if (want_cost) cx = cost_rows(bf);
    __syncthreads();

    double sn[NP]; // 2: row j of S_{t+1}
    ASLR_UNROLL for (int p = 0; p < NP; ++p) sn[p] = 0.0;
    ASLR_SWEEP_LOOP for (int i = 0; i < NX; ++i) {
      const double f = my_f[i];
      ASLR_UNROLL for (int p = 0; p < NP; ++p) sn[p] = fma(f, bf[oS + i * NP + p], sn[p]);
    }
    ASLR_SWEEP_LOOP for (int k = 0; k < NU; ++k) {
      const double f = -my_f[NX + k];
      ASLR_UNROLL for (int p = 0; p < NP; ++p) sn[p] = fma(f, bf[oV + k * NP + p], sn[p]);
    }
    if (STIFF) {
      ASLR_UNROLL for (int c = 0; c < P0; ++c)
        sn[c] = fma(bf[oGp + c], my_f[NJ + c] - (j == NJ + c ? 1.0 : 0.0), sn[c]);
    }
    ASLR_UNROLL for (int c = 0; c < NJ; ++c)
      sn[P0 + c] = fma(bf[oGp + NJ + c], j == NJ + c ? dt : (j == 3 * NJ + c ? 1.0 : 0.0), sn[P0 + c]);
    if (a.u_var) {
      double v = 0.0;
      ASLR_UNROLL for (int p = 0; p < NP; ++p) {
        const double e = bf[oV + ku * NP + p];
        v = fma(e * e, tm[oVar + p], v);
      }
      if (live_u) a.u_var[((size_t)t * B + b) * NU + ku] = v;
    }
    if (want_cost) {
      double cu = 0.0;
      for (int k = 0; k < NU; ++k) cu = fma(bf[oLu + k], bf[oV + k * NP + pc], cu);
      acc += cx - cu;
    }
    ASLR_UNROLL for (int p = 0; p < NP; ++p) s[p] = sn[p];
    cur = nxt;
  }
  store(s, T);
  if (live) {
    const size_t row = (size_t)b * NX + j;
    if (STIFF && a.dxT_k) {
      ASLR_UNROLL for (int c = 0; c < P0; ++c) a.dxT_k[row * NJ + c] = s[c];
    }
    if (a.dxT_b) {
      ASLR_UNROLL for (int c = 0; c < NJ; ++c) a.dxT_b[row * NJ + c] = s[P0 + c];
    }
  }
  if (want_cost) {
    double *bf = tm + (T & 1) * BUF; // (last read in knot T-2: the barriers of knot T-1 lie in between)
    stage_rows(bf, s, a.deriv[((size_t)T * B + b) * L::len + L::oLx + j]);
    __syncthreads();
    acc += cost_rows(bf);
    if (live_p) {
      if (jr < P0) { if (a.dcost_k) a.dcost_k[(size_t)jr * B + b] = acc; }
      else if (a.dcost_b) a.dcost_b[(size_t)(jr - P0) * B + b] = acc;
    }
  }
}

template <int NJ, int DAM>
int launch_plant_sens(const PlantSensArgs &a, hipStream_t st) {
  return launch_sweep_stiff<NJ, DAM>([](auto STIFF) { return plant_sens_kernel<4 * NJ, ModelDims<NJ, DAM>::nu, decltype(STIFF)::value>; }, a, st);
}

} // namespace aslr
