// aslr_mpc_plant_team.inc.hpp -- the plant phase of a receding-horizon run on a mismatched plant for the larger chain
// (7-DoF SEA / VSA): aslr_mpc_run_plant_all, include/aslr_to_amd_mpc_plant_all.h, DESIGN.md 4.18.
//
//   mpc_plant_team_kernel   A TEAM OF 8 LANES PER TRAJECTORY.  The plant step is TeamStep's (aslr_team_step.hpp); on top
//                           of it lane c < NJ owns row c of the control law (rows c and NJ + c for VSA).  The definition is
//                           mpc_plant_kernel's (aslr_mpc_plant.inc.hpp): `hold` knots of the plan in XS / US / KGAIN applied
//                           to the trajectory's own plant.  What is this kernel's own, against policy_rollout_team_kernel
//                           (aslr_policy_team.inc.hpp):
//     - there is ONE plant per trajectory, so the eight teams of a wave are eight trajectories and share nothing: no
//       per-wave stage.  A block is one wave; the grid is over ceil(B / 8) waves;
//     - every team reads [K_j | xs_j | us_j] of ITS trajectory straight from KGAIN / XS / US, one knot ahead: lane c its
//       row(s) of K_j as 16-byte pieces into registers, entries 4c .. 4c + 3 of xs_j (to the team's LDS at the top of the
//       next knot), its own entries of us_j (they stay in registers: the lane that reads them is the lane that owns the
//       row), of the reference placement and of the disturbance;
//     - every applied knot is node 0's action model (the running knots share one model: aslr_mpc_run's refusals), so the
//       model rows, dt and the box are read once, before the loop;
//     - knot 0 forms no feedback term: x IS XS[0], and KGAIN[0] never enters the arithmetic (it may hold Inf or NaN);
//     - the sums of a run continue over its control steps in place (pa.first), there is no terminal cost;
//     - it writes nothing but the caller's buffers.
#pragma once
#include "aslr_team_step.hpp"

namespace aslr {

template <int NJ, int DAM>
__global__ void __launch_bounds__(64) mpc_plant_team_kernel(KArgs a, ModelLimits lim, MpcPlantArgs pa) {
  using C = FwdTeam<NJ, DAM>;
  constexpr int NX = C::NX, NU = C::NU;
  constexpr bool VSA = C::VSA;
  constexpr int TPB = 8; // teams (trajectories) per block = per wave
  // per team (doubles): FwdTeam's arrays, then xs_j and the reference placement of the knot
  constexpr int tXr = C::TEAM_LDS, tFr = tXr + NX, TEAM = tFr + 12;
  static_assert(NX % 4 == 0 && NX / 4 == NJ, "lane c < NJ moves entries 4c .. 4c + 3 of a state row");
  __shared__ double sm[TPB * TEAM];
  const int lane = threadIdx.x, team = lane >> 3, c = lane & 7;
  const int B = a.B, hold = pa.hold;
  // teams past B run on a clamped index (the arithmetic of a trajectory is the same instruction stream wherever it sits);
  // only their stores are guarded
  const int bq = blockIdx.x * TPB + team, b = bq < B ? bq : B - 1;
  const bool on = bq < B;
  double *tm_ = sm + team * TEAM;
  const TeamStep<NJ, VSA, C> ts(tm_, c);
  double *const xT = ts.xT, *const uT = ts.uT, *xrT = tm_ + tXr, *frT = tm_ + tFr;
  const bool jl = ts.jl; // this lane owns joint / row cj
  const int cj = ts.cj;
  const DevDesc &D = *a.desc;
  const aslr_chain_t &ch = D.chain;
  const chain_cp chc = chain_const(&D.chain);
  const unsigned long long team_bits = 0xffull << (team * 8);

  __shared__ double jtab[8][12];
  stage_joint_table<NJ>(jtab, ch, lane); // (fenced by the wave_sync at the top of knot 0)

  // ---- the model of every applied knot, and the plant of this team, entry cj: the caller's arrays [nj][B] where given,
  // else the trajectory's row of the parameter table where one is set, else the row of the model ----
  const int mi = node_model_at(a, 0);
  const DevModel &dm = D.models[mi];
  const bool table = pa.table != 0, use_k = pa.plant_stiffness || table, use_b = pa.plant_motor_inertia || table;
  double k_cj = 0.0, b_cj = 0.0, lb_c = 0.0, ub_c = 0.0, lb_s = 0.0, ub_s = 0.0; // (lb_s / ub_s: the stiffness row, VSA)
  if (table) {
    // (team_table_row's text: through the helper this kernel alone issues each of these loads twice)
    const double *tp = traj_params_at(D, b);
    k_cj = tp[(size_t)cj * B];
    b_cj = tp[(size_t)(NJ + cj) * B];
    lb_c = tp[(size_t)(2 * NJ + cj) * B];
    ub_c = tp[(size_t)(2 * NJ + NU + cj) * B];
    if (VSA) { lb_s = tp[(size_t)(3 * NJ + cj) * B]; ub_s = tp[(size_t)(3 * NJ + NU + cj) * B]; }
  } else {
    lb_c = lim.lb[mi][cj];
    ub_c = lim.ub[mi][cj];
    if (VSA) { lb_s = lim.lb[mi][NJ + cj]; ub_s = lim.ub[mi][NJ + cj]; }
  }
  if (pa.plant_stiffness) k_cj = pa.plant_stiffness[(size_t)cj * B + b];
  if (pa.plant_motor_inertia) b_cj = 1.0 / pa.plant_motor_inertia[(size_t)cj * B + b];
  double Krow[NJ], Srow[NJ], Brow[NJ];
  team_model_rows<NJ, NU, VSA>(dm, cj, pa.diagonal, use_k, k_cj, use_b, b_cj, Krow, Srow, Brow);
  const double dt = dm.m.dt;
  const bool clamp = pa.clamp && lim.has[mi];

  // XS[0] into the team's state: where the solve started, and the plant is now
  if (jl) {
    const double *x0 = a.xs + (size_t)b * NX + 4 * c;
    const double2 v0 = *reinterpret_cast<const double2 *>(x0), v1 = *reinterpret_cast<const double2 *>(x0 + 2);
    xT[4 * c] = v0.x; xT[4 * c + 1] = v0.y; xT[4 * c + 2] = v1.x; xT[4 * c + 3] = v1.y;
  }

  // ---- what is read one knot ahead: this lane's row(s) of K_j, entries 4c .. 4c + 3 of xs_j, entries cj (and NJ + cj) of
  // us_j, entries c and 8 + c of the reference placement of row min(row0 + j, last), and entries cj, NJ + cj, 2 NJ + cj,
  // 3 NJ + cj of the disturbance ----
  double Kn[NX], Ksn[VSA ? NX : 2], xn[4] = {0.0, 0.0, 0.0, 0.0}, un = 0.0, usn = 0.0, fn[2] = {0.0, 0.0}, wn[4] = {0.0, 0.0, 0.0, 0.0};
  ASLR_UNROLL for (int i = 0; i < NX; ++i) Kn[i] = 0.0;
  ASLR_UNROLL for (int i = 0; i < (VSA ? NX : 2); ++i) Ksn[i] = 0.0;
  const double *wsrc = pa.disturbance ? pa.disturbance + (size_t)b * NX + cj : nullptr; // knot j at + j B NX
  auto prefetch = [&](int j) {
    const double *us = a.us + ((size_t)j * B + b) * NU;
    un = us[cj];
    if constexpr (VSA) usn = us[NJ + cj];
    if (a.frame_ref) {
      const double *fr = a.frame_ref + 12 * ((size_t)min(a.ref_row0 + j, a.ref_last) * B + b); // (the applied knot's row of the path)
      fn[0] = fr[c];
      fn[1] = fr[8 + (c & 3)];
    }
    if (wsrc) { ASLR_UNROLL for (int k = 0; k < 4; ++k) wn[k] = wsrc[(size_t)j * B * NX + k * NJ]; }
  };
  // (not for knot 0: x IS xs[0], no feedback term is formed -- x - xs would be +0, but K may hold Inf or NaN)
  auto prefetch_gains = [&](int j) {
    {
      const double *K = a.kgain + ((size_t)j * B + b) * NU * NX, *xr = a.xs + ((size_t)j * B + b) * NX + 4 * cj;
      ASLR_UNROLL for (int p = 0; p < NX / 2; ++p) {
        const double2 v = *reinterpret_cast<const double2 *>(K + cj * NX + 2 * p);
        Kn[2 * p] = v.x; Kn[2 * p + 1] = v.y;
      }
      if constexpr (VSA) {
        ASLR_UNROLL for (int p = 0; p < NX / 2; ++p) {
          const double2 v = *reinterpret_cast<const double2 *>(K + (NJ + cj) * NX + 2 * p);
          Ksn[2 * p] = v.x; Ksn[2 * p + 1] = v.y;
        }
      }
      const double2 v0 = *reinterpret_cast<const double2 *>(xr), v1 = *reinterpret_cast<const double2 *>(xr + 2);
      xn[0] = v0.x; xn[1] = v0.y; xn[2] = v1.x; xn[3] = v1.y;
    }
  };
  double *x_o = pa.x_rec + (size_t)b * NX + 4 * cj, *u_o = pa.u_rec + (size_t)b * NU; // knot j at + j B NX / + j B NU
  auto store_x = [&](int j) { // the team's state as row j of this step's records, 4 contiguous entries per lane
    if (on && jl) team_store_state_row(x_o + (size_t)j * B * NX, xT, c);
  };
  const typename Chain3D<NJ>::Consts cc(D, true);
  ModelRegs<NJ, NU> mr; // (the cost stack reads none of it)

  // the sums of a run continue over its control steps: step 0 starts them, a later step picks up what the one before left
  double J = 0.0;
  int failed = -1;
  if (!pa.first) {
    if (pa.closed_cost) J = pa.closed_cost[b];
    if (pa.failed_knot) failed = pa.failed_knot[b];
  }
  bool failed_here = false;
  prefetch(0);
  for (int j = 0; j < hold; ++j) {
    wave_sync(); // the previous knot's readers of xs_j and the placement are done, its state is written (knot 0: the joint table, XS[0])
    if (jl && j > 0) { ASLR_UNROLL for (int k = 0; k < 4; ++k) xrT[4 * c + k] = xn[k]; }
    frT[c] = fn[0];
    if (c < 4) frT[8 + c] = fn[1];
    wave_sync();
    // ---- control law, row cj: u = us_j - K_j (x - xs_j) from knot 1 on, box clamp when asked for ----
    double u_c = un, u_s = usn; // this lane's entries of the applied control (u_s: the stiffness command, VSA)
    if (j > 0) {
      ASLR_UNROLL for (int jx = 0; jx < NX; ++jx) u_c -= Kn[jx] * (xT[jx] - xrT[jx]);
      if constexpr (VSA) { ASLR_UNROLL for (int jx = 0; jx < NX; ++jx) u_s -= Ksn[jx] * (xT[jx] - xrT[jx]); }
    }
    if (clamp) {
      u_c = fmin(fmax(u_c, lb_c), ub_c);
      if constexpr (VSA) u_s = fmin(fmax(u_s, lb_s), ub_s);
    }
    if (jl) {
      uT[c] = u_c;
      if constexpr (VSA) uT[NJ + c] = u_s;
    }
    wave_sync();
    // ---- running cost of the applied knot: the team's state and the applied control, BEFORE the loads of the next knot
    // are issued (the cost stack reads its terms from global memory, and behind those loads its waits would be waits for
    // the prefetch) ----
    {
      double x[NX], u[NU], xnext[NX], cst = 0.0;
      ASLR_UNROLL for (int i = 0; i < NX; ++i) x[i] = xT[i];
      ASLR_UNROLL for (int i = 0; i < NU; ++i) u[i] = uT[i];
      knot_eval<NJ, DAM, kEvalCost, Chain3D<NJ>>(cc, mr, dm, a.frame_ref ? frT : nullptr, x, u, xnext, cst, nullptr);
      J += cst; // (applied control, knot order)
    }
    double w[4];
    ASLR_UNROLL for (int k = 0; k < 4; ++k) w[k] = wn[k];
    // in flight while the dynamics of knot j compute.  Unconditional, so that these registers are dead from the top of the
    // knot to here, across the cost: the last knot reads its own row again, which nothing uses
    const int jn = min(j + 1, hold - 1);
    prefetch(jn);
    // (the records of a knot go out after the loads of the next one)
    store_x(j);
    if (on && jl) {
      u_o[(size_t)j * B * NU + c] = u_c;
      if constexpr (VSA) u_o[(size_t)j * B * NU + NJ + c] = u_s;
    }
    // ---- the plant step (aslr_team_step.hpp) ----
    ts.rotation(jtab);
    wave_sync();
    ts.torques(Krow, Srow);
    ts.mass_columns(chc);
    wave_sync();
    // the row(s) of K and the entries of xs of the knot ahead: 28 / 56 doubles per lane, issued behind the RNEA -- the
    // register peak of the knot, where they would be spilled to the private segment -- and in flight over the inverse, the
    // accelerations and the Euler step
    prefetch_gains(jn);
    ts.minv_column();
    wave_sync();
    double nxt[4]; // this lane's entries {q_l, v_l, q_m, v_m} of xnext
    const bool bad = ts.euler(Brow, dt, nxt);
    if (__ballot(bad) & team_bits) { // NaN / Inf / |xnext|_inf >= 1e30, as the solver's rollout
      failed_here = true;
      if (failed < 0) failed = pa.k0 + j;
    }
    wave_sync(); // every lane of the team has read the old state
    if (jl) {
      if (wsrc) { xT[c] = nxt[0] + w[0]; xT[NJ + c] = nxt[2] + w[1]; xT[2 * NJ + c] = nxt[1] + w[2]; xT[3 * NJ + c] = nxt[3] + w[3]; }
      else { xT[c] = nxt[0]; xT[NJ + c] = nxt[2]; xT[2 * NJ + c] = nxt[1]; xT[3 * NJ + c] = nxt[3]; }
    }
  }
  wave_sync(); // the state behind the last applied knot is written
  if (!on) return;
  // x+: the row behind the last record (the next step's first record, or x_closed[N]); mpc_advance_kernel reads it there
  store_x(hold);
  if (c == 0) {
    if (pa.closed_cost) pa.closed_cost[b] = failed_here ? NAN : J; // (NaN stays NaN through the sums of the later steps)
    if (pa.failed_knot) pa.failed_knot[b] = failed;
  }
}

// the nx = 28 sizes: one block = one wave = 8 teams = 8 trajectories
template <int NJ, int DAM>
int launch_mpc_plant_team(const KArgs &k, const ModelLimits &lim, const MpcPlantArgs &pa, hipStream_t st) {
  const dim3 grid((k.B + 7) / 8), block(64);
  hipLaunchKernelGGL((mpc_plant_team_kernel<NJ, DAM>), grid, block, 0, st, k, lim, pa);
  HIP_TRY(hipGetLastError());
  return ASLR_OK;
}

} // namespace aslr
