// aslr_mpc_plant.inc.hpp -- the plant phase of a receding-horizon run on a plant that differs from the model
// (aslr_mpc_run_plant, include/aslr_to_amd_mpc_plant.h):
//
//   mpc_plant_kernel   one lane per trajectory.  Between two solves the lane applies `hold` knots of the plan the solve left
//                      in XS / US / KGAIN to its own plant (diagonals of K and B, additive disturbance): the first control as
//                      it is, the later ones with the Riccati feedback u = us_j - K_j (x - xs_j); it records the applied
//                      states and controls, sums the running costs of its closed loop in knot order and leaves the state the
//                      next solve starts from in the row behind its last record.
//
// There is one plant per trajectory, so the 16-lane sample teams of policy_rollout_kernel would idle 15 lanes: a wave takes
// 64 trajectories instead, and what a lane reads per knot -- [K | xs | us] of ITS trajectory -- is private to it (no LDS).
// With `hold` knots of a few hundred flops each the kernel is bound by the latency of those reads, not by bandwidth.
// The kernel writes nothing but the caller's buffers: no workspace region, no solver state.
#pragma once
#include "aslr_common.hpp"

namespace aslr {

template <int NJ, int DAM, bool PLANAR>
__global__ void __launch_bounds__(64) mpc_plant_kernel(KArgs a, ModelLimits lim, MpcPlantArgs pa) {
  constexpr int NX = 4 * NJ, NU = ModelDims<NJ, DAM>::nu;
  static_assert(NX % 2 == 0 && NU % 2 == 0, "16-byte pieces");
  using CH = std::conditional_t<PLANAR, ChainPlanar<NJ>, Chain3D<NJ>>;
  const int B = a.B, hold = pa.hold;
  // lanes past B run on a clamped index (the arithmetic of a trajectory is the same instruction stream wherever it sits);
  // only their stores are guarded
  const int bq = blockIdx.x * 64 + threadIdx.x;
  const int b = bq < B ? bq : B - 1;
  const bool on = bq < B;
  const DevDesc &D = *a.desc;

  // the plant of this lane: diag K and diag 1 / B -- the caller's arrays [nj][B] where given, else the trajectory's row of
  // the parameter table where one is set, else (use_k / use_b false) the constants of the model
  const bool table = pa.table != 0, use_k = pa.plant_stiffness || table, use_b = pa.plant_motor_inertia || table;
  double pk[NJ], pbinv[NJ], lim_lb[NU], lim_ub[NU];
  ASLR_UNROLL for (int i = 0; i < NJ; ++i) { pk[i] = 0.0; pbinv[i] = 0.0; }
  const int mi = node_model_at(a, 0); // every applied knot is node 0's action model (the running knots share one model)
  const DevModel &dm = D.models[mi];
  if (table) {
    const double *tp = traj_params_at(D, b);
    ASLR_UNROLL for (int i = 0; i < NJ; ++i) { pk[i] = tp[(size_t)i * B]; pbinv[i] = tp[(size_t)(NJ + i) * B]; }
    ASLR_UNROLL for (int i = 0; i < NU; ++i) { lim_lb[i] = tp[(size_t)(2 * NJ + i) * B]; lim_ub[i] = tp[(size_t)(2 * NJ + NU + i) * B]; }
  } else {
    ASLR_UNROLL for (int i = 0; i < NU; ++i) { lim_lb[i] = lim.lb[mi][i]; lim_ub[i] = lim.ub[mi][i]; }
  }
  if (pa.plant_stiffness) {
    ASLR_UNROLL for (int i = 0; i < NJ; ++i) pk[i] = pa.plant_stiffness[(size_t)i * B + b];
  }
  if (pa.plant_motor_inertia) {
    ASLR_UNROLL for (int i = 0; i < NJ; ++i) pbinv[i] = 1.0 / pa.plant_motor_inertia[(size_t)i * B + b];
  }
  const typename CH::Consts cc(D, true);
  ModelRegs<NJ, NU> mr;
  mr.load(dm);
  if (pa.diagonal) { // (the host's fact: a plant array or a table, both of which need diagonal models)
    TrajDiag<NJ> d;
    ASLR_UNROLL for (int i = 0; i < NJ; ++i) { d.k[i] = use_k ? pk[i] : mr.K[i][i]; d.binv[i] = use_b ? pbinv[i] : mr.Binv[i][i]; }
    mr.set_traj(d);
  }
  const bool clamp = pa.clamp && lim.has[mi];

  double x[NX];
  {
    const double *x0 = a.xs + (size_t)b * NX; // XS[0]: where the solve started, and the plant is now
    ASLR_UNROLL for (int p = 0; p < NX / 2; ++p) {
      const double2 v = *reinterpret_cast<const double2 *>(x0 + 2 * p);
      x[2 * p] = v.x; x[2 * p + 1] = v.y;
    }
  }
  const double *wsrc = pa.disturbance ? pa.disturbance + (size_t)b * NX : nullptr; // knot j at + j B NX
  double wn[NX]; // the disturbance of the knot ahead
  ASLR_UNROLL for (int i = 0; i < NX; ++i) wn[i] = 0.0;
  auto load_w = [&](int j) {
    ASLR_UNROLL for (int p = 0; p < NX / 2; ++p) {
      const double2 v = *reinterpret_cast<const double2 *>(wsrc + (size_t)j * B * NX + 2 * p);
      wn[2 * p] = v.x; wn[2 * p + 1] = v.y;
    }
  };
  if (wsrc) load_w(0);
  double *x_o = pa.x_rec + (size_t)b * NX, *u_o = pa.u_rec + (size_t)b * NU; // knot j at + j B NX / + j B NU

  // the sums of a run continue over its control steps: step 0 starts them, a later step picks up what the one before left
  double J = 0.0;
  int failed = -1;
  if (!pa.first) {
    if (pa.closed_cost) J = pa.closed_cost[b];
    if (pa.failed_knot) failed = pa.failed_knot[b];
  }
  bool failed_here = false;
  for (int j = 0; j < hold; ++j) {
    double w[NX];
    ASLR_UNROLL for (int i = 0; i < NX; ++i) w[i] = wn[i];
    if (wsrc && j + 1 < hold) load_w(j + 1); // in flight while knot j computes
    double u[NU];
    {
      const double *us = a.us + ((size_t)j * B + b) * NU;
      ASLR_UNROLL for (int p = 0; p < NU / 2; ++p) {
        const double2 v = *reinterpret_cast<const double2 *>(us + 2 * p);
        u[2 * p] = v.x; u[2 * p + 1] = v.y;
      }
    }
    if (j > 0) { // knot 0: x IS xs[0], no feedback term is formed (x - xs would be +0, but K may hold Inf or NaN)
      const double *xr = a.xs + ((size_t)j * B + b) * NX, *K = a.kgain + ((size_t)j * B + b) * NU * NX;
      double dx[NX];
      ASLR_UNROLL for (int p = 0; p < NX / 2; ++p) {
        const double2 v = *reinterpret_cast<const double2 *>(xr + 2 * p);
        dx[2 * p] = x[2 * p] - v.x; dx[2 * p + 1] = x[2 * p + 1] - v.y;
      }
      ASLR_UNROLL for (int i = 0; i < NU; ++i) {
        double sm = u[i];
        ASLR_UNROLL for (int p = 0; p < NX / 2; ++p) {
          const double2 v = *reinterpret_cast<const double2 *>(K + i * NX + 2 * p);
          sm -= v.x * dx[2 * p];
          sm -= v.y * dx[2 * p + 1];
        }
        u[i] = sm;
      }
    }
    if (clamp) {
      ASLR_UNROLL for (int i = 0; i < NU; ++i) u[i] = fmin(fmax(u[i], lim_lb[i]), lim_ub[i]);
    }
    if (on) {
      ASLR_UNROLL for (int p = 0; p < NX / 2; ++p)
        *reinterpret_cast<double2 *>(x_o + (size_t)j * B * NX + 2 * p) = make_double2(x[2 * p], x[2 * p + 1]);
      ASLR_UNROLL for (int p = 0; p < NU / 2; ++p)
        *reinterpret_cast<double2 *>(u_o + (size_t)j * B * NU + 2 * p) = make_double2(u[2 * p], u[2 * p + 1]);
    }
    const double *fref = a.frame_ref ? a.frame_ref + 12 * ((size_t)min(a.ref_row0 + j, a.ref_last) * B + b) : nullptr; // (the applied knot's row of the reference path)
    double xnext[NX], c = 0.0;
    knot_eval<NJ, DAM, kEvalDyn | kEvalCost, CH>(cc, mr, dm, fref, x, u, xnext, c, nullptr);
    J += c; // (applied control, knot order)
    double mx = 0.0;
    ASLR_UNROLL for (int i = 0; i < NX; ++i) mx += fabs(xnext[i]);
    if (inf_norm_bad<NX>(mx, xnext)) { // NaN / Inf / |xnext|_inf >= 1e30, as the solver's rollout
      failed_here = true;
      if (failed < 0) failed = pa.k0 + j;
    }
    if (wsrc) { ASLR_UNROLL for (int i = 0; i < NX; ++i) x[i] = xnext[i] + w[i]; }
    else { ASLR_UNROLL for (int i = 0; i < NX; ++i) x[i] = xnext[i]; }
  }
  if (!on) return;
  // x+: the row behind the last record (the next step's first record, or x_closed[N]); mpc_advance_kernel reads it there
  ASLR_UNROLL for (int p = 0; p < NX / 2; ++p)
    *reinterpret_cast<double2 *>(x_o + (size_t)hold * B * NX + 2 * p) = make_double2(x[2 * p], x[2 * p + 1]);
  if (pa.closed_cost) pa.closed_cost[b] = failed_here ? NAN : J; // (NaN stays NaN through the sums of the later steps)
  if (pa.failed_knot) pa.failed_knot[b] = failed;
}

// the nx = 8 sizes, as policy_rollout_kernel
template <int NJ, int DAM>
int launch_mpc_plant(const KArgs &k, const ModelLimits &lim, const MpcPlantArgs &pa, hipStream_t st) {
  const dim3 grid((k.B + 63) / 64), block(64);
  with_planar<NJ>(k, [&](auto P) {
    hipLaunchKernelGGL((mpc_plant_kernel<NJ, DAM, decltype(P)::value>), grid, block, 0, st, k, lim, pa);
  });
  HIP_TRY(hipGetLastError());
  return ASLR_OK;
}

} // namespace aslr
