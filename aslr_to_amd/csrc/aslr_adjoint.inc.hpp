// aslr_adjoint.inc.hpp -- the adjoint (costate) sweep behind aslr_cost_sensitivity (include/aslr_to_amd_sens.h).
//
//   lambda_T = Lx_T,   lambda_t = Lx_t + Fx_t^T lambda_{t+1}                      (t = T-1 .. 0)
//   dJ/dx0   = lambda_0
//   dJ/dK_j  = sum_t -(delta_j / K_j) ((Fx_t^T lambda_{t+1})[nj+j] - lambda_{t+1}[nj+j]),   delta = q_l - q_m of knot t
//   dJ/dB_j  = sum_t -(1 / B_j) (dt D lambda_{t+1}[nj+j] + D lambda_{t+1}[3nj+j]),          D = xnext_t[3nj+j] - x_t[3nj+j]
//
// xnext is linear in K_j and in 1 / B_j, and the q_m,j column of Fx already holds dxnext/dK_j up to the factor
// -delta_j / K_j, so no rigid-body term is evaluated again: the sweep reads Fx and Lx of every
// record and four words of XS / XNEXT per knot.
//
// Decomposition: one team of lanes per trajectory (aslr_sweep_team.hpp), lane j owns column j of Fx and entry j of
// lambda.  Column reads coalesce (row i of Fx is nx consecutive words, one per lane).  (Fx^T lambda)[j] is ONE fma chain
// over i = 0 .. nx-1, ascending; lambda[i] reaches the team through a cross-lane shuffle, never through memory.  The
// parameter terms are local to lane nj + j once that product exists and accumulate there in t order.  The clamped
// indices keep every shuffle source valid.
//
// Latency-bound like the other serial sweeps: knot t-1 is loaded while knot t is reduced.
#pragma once
#include "aslr_sweep_team.hpp"

namespace aslr {

template <int NX, int NU>
__global__ void __launch_bounds__(64) adjoint_kernel(AdjointArgs a) {
  constexpr int NJ = SweepTeam<NX>::NJ, TEAM = SweepTeam<NX>::TEAM, TPW = SweepTeam<NX>::TPW;
  using L = RecLayout<NJ, NU>;
  const int lane = threadIdx.x, jr = lane % TEAM;
  const int br = blockIdx.x * TPW + lane / TEAM;
  const bool live = br < a.B && jr < NX; // trajectories past B and the idle lanes of a 32-lane team store nothing
  const int B = a.B, T = a.T;
  const int b = br < B ? br : B - 1, j = jr < NX ? jr : NX - 1; // clamped: every lane reads inside the arrays
  const bool motor = j >= NJ && j < 2 * NJ; // lane nj + jj: the parameter terms of joint jj
  const int jj = motor ? j - NJ : 0;

  // 1 / K_jj and 1 / B_jj of this lane's joint, per action model (one value for all of them with a table).  As the model choice in
  // the loop, written out here and in plant_sens_kernel: through a helper both kernels came out changed (profiles/ext_rows/)
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

  struct Knot { double col[NX], lx, ql, qm, vm, vmn; };
  const auto load = [&](Knot &k, int t) {
    const double *rec = a.deriv + ((size_t)t * B + b) * L::len;
    ASLR_UNROLL for (int i = 0; i < NX; ++i) k.col[i] = rec[L::oFx + i * NX + j];
    k.lx = rec[L::oLx + j];
    const size_t xo = ((size_t)t * B + b) * NX;
    k.ql = a.xs[xo + jj]; k.qm = a.xs[xo + NJ + jj];
    k.vm = a.xs[xo + 3 * NJ + jj]; k.vmn = a.xnext[xo + 3 * NJ + jj];
  };

  double lam = a.deriv[((size_t)T * B + b) * L::len + L::oLx + j]; // lambda_T = Lx_T
  if (live && a.costate) a.costate[((size_t)T * B + b) * NX + j] = lam;
  double acc_k = 0.0, acc_b = 0.0;
  Knot cur;
  load(cur, T - 1);
  for (int t = T - 1; t >= 0; --t) {
    Knot nxt;
    load(nxt, t > 0 ? t - 1 : 0); // in flight while knot t is reduced (t = 0: a repeat, dropped)
    double g = 0.0; // (Fx_t^T lambda_{t+1})[j]
    ASLR_UNROLL for (int i = 0; i < NX; ++i) g = fma(cur.col[i], __shfl(lam, i, TEAM), g);
    const double lam_v = __shfl(lam, 3 * NJ + jj, TEAM); // lambda_{t+1}[3nj + jj]
    const int mi = ((const int32_t __attribute__((address_space(4))) *)(a.node_model))[t];
    double dt = a.plant.dt[0], rkm = rk[0], bim = bi[0];
    ASLR_UNROLL for (int m = 1; m < ASLR_MAX_MODELS; ++m)
      if (mi == m) { dt = a.plant.dt[m]; rkm = rk[m]; bim = bi[m]; }
    const double delta = cur.ql - cur.qm, D = cur.vmn - cur.vm;
    acc_k += -(delta * rkm) * (g - lam);
    acc_b += -bim * (dt * D * lam + D * lam_v);
    lam = cur.lx + g;
    if (live && a.costate) a.costate[((size_t)t * B + b) * NX + j] = lam;
    cur = nxt;
  }
  if (!live) return;
  if (a.d_x0) a.d_x0[(size_t)j * B + b] = lam;
  if (motor) {
    if (a.d_stiffness) a.d_stiffness[(size_t)jj * B + b] = acc_k;
    if (a.d_motor_inertia) a.d_motor_inertia[(size_t)jj * B + b] = acc_b;
  }
}

template <int NJ, int DAM>
int launch_adjoint(const AdjointArgs &a, hipStream_t st) {
  return launch_sweep<NJ, DAM>(adjoint_kernel<4 * NJ, ModelDims<NJ, DAM>::nu>, a, st);
}

} // namespace aslr
