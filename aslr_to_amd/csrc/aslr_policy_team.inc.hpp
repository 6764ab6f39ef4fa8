// aslr_policy_team.inc.hpp -- closed-loop roll-outs of the stored policy on a perturbed plant for the larger chain
// (7-DoF SEA / VSA): aslr_policy_rollout_all, include/aslr_to_amd_policy_all.h, DESIGN.md 4.17.
//
//   policy_rollout_team_kernel   A TEAM OF 8 LANES PER (trajectory, SAMPLE).  The plant step is TeamStep's
//                                (aslr_team_step.hpp); on top of it lane c < NJ owns row c of the control law (rows c and
//                                NJ + c for VSA).  What is this kernel's own:
//     - the team index is the sample: one block = 2 waves = 16 samples of ONE trajectory, so what the samples share --
//       [K_t | xs_t | us_t | reference placement of the knot] -- is staged once per wave and prefetched one knot ahead;
//     - every team has its own plant: lane c holds K_cc and 1 / B_cc of its sample (the caller's arrays, else the row of
//       the parameter table, else the model's row -- the full row, so a non-diagonal model without a plant argument still
//       rolls out), its entries of the initial-state offset and of the disturbance;
//     - the node cost is evaluated inside the kernel (knot_eval<..., kEvalCost> on the team's state and applied control)
//       and summed per sample in knot order: S x B costs leave the device unless trajectories are asked for.  Every lane
//       of the team evaluates the cost of its team's knot: one instruction stream, no divergence inside the wave, and
//       the time of one evaluation -- what a single lane per team would take, the other seven masked off;
//     - it writes nothing but the caller's buffers.
#pragma once
#include "aslr_team_step.hpp"
#include "aslr_policy_noise.hpp"

namespace aslr {

// PA: where the perturbations come from, as in policy_rollout_kernel (aslr_policy.inc.hpp).  With PolicyNoiseArgs lane c
// draws the pairs that hold the entries it owns (the other half of a pair is thrown away: what matters is that every entry
// has the value of the definition).
template <int NJ, int DAM, class PA = PolicyArgs>
__global__ void __launch_bounds__(128) policy_rollout_team_kernel(KArgs a, ModelLimits lim, PA pa) {
  using C = FwdTeam<NJ, DAM>;
  constexpr bool DRAW = std::is_same_v<PA, PolicyNoiseArgs>;
  constexpr int NX = C::NX, NU = C::NU;
  constexpr bool VSA = C::VSA;
  constexpr int TPB = 16; // teams (samples) per block
  // per-wave stage (doubles): K, xs, us of the current knot and its reference placement
  constexpr int oK = 0, oXr = oK + NU * NX, oU = oXr + NX, oFr = (oU + NU + 1) / 2 * 2, STG = oFr + 12, NSLOT = (STG + 63) / 64;
  __shared__ double sm[2 * STG + TPB * C::TEAM_LDS];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, team = tid >> 3, c = tid & 7;
  const int B = a.B, T = a.T, S = pa.S, b = blockIdx.x;
  // teams past S run on clamped indices (the arithmetic of a sample is the same instruction stream wherever it sits);
  // only their stores are guarded
  const int sq = blockIdx.y * TPB + team, s = sq < S ? sq : S - 1;
  const bool on = sq < S;
  double *stg = sm + wv * STG, *tm_ = sm + 2 * STG + team * C::TEAM_LDS;
  const TeamStep<NJ, VSA, C> ts(tm_, c);
  double *const xT = ts.xT, *const uT = ts.uT;
  const bool jl = ts.jl; // this lane owns joint / row cj
  const int cj = ts.cj;
  const DevDesc &D = *a.desc;
  const aslr_chain_t &ch = D.chain;
  const chain_cp chc = chain_const(&D.chain);
  const unsigned long long team_bits = 0xffull << ((lane >> 3) * 8);

  // ---- stage slots: element idx = lane + 64 q of [K | xs | us | placement] at knot t ----
  const double *sp0[NSLOT];
  size_t sstr[NSLOT];
  bool son[NSLOT], sctl[NSLOT];
  ASLR_UNROLL for (int q = 0; q < NSLOT; ++q) {
    const int idx = lane + 64 * q;
    sp0[q] = a.xs; sstr[q] = 0; son[q] = false; sctl[q] = false;
    if (idx < oXr) { sp0[q] = a.kgain + (size_t)b * NU * NX + idx; sstr[q] = (size_t)B * NU * NX; son[q] = true; sctl[q] = true; }
    else if (idx < oU) { sp0[q] = a.xs + (size_t)b * NX + (idx - oXr); sstr[q] = (size_t)B * NX; son[q] = true; sctl[q] = true; }
    else if (idx < oU + NU) { sp0[q] = a.us + (size_t)b * NU + (idx - oU); sstr[q] = (size_t)B * NU; son[q] = true; sctl[q] = true; }
    else if (idx >= oFr && idx < STG && a.frame_ref) { sp0[q] = a.frame_ref + (size_t)b * 12 + (idx - oFr); sstr[q] = (size_t)B * 12; son[q] = true; }
  }
  double pf[NSLOT];
  auto prefetch = [&](int t) {
    const size_t row = (size_t)min(a.ref_row0 + t, a.ref_last); // (the knot's row of the reference path)
    ASLR_UNROLL for (int q = 0; q < NSLOT; ++q) {
      pf[q] = 0.0;
      if (son[q] && (!sctl[q] || t < T)) pf[q] = sp0[q][(sctl[q] ? (size_t)t : row) * sstr[q]];
    }
  };

  // ---- the plant of this team, entry cj: the caller's arrays [nj][S][B] where given, else the trajectory's row of the
  // parameter table where one is set, else (use_k / use_b false) the row of the knot's model ----
  bool drawn_k = false, drawn_b = false;
  if constexpr (DRAW) { drawn_k = pa.stiffness_rel_std != nullptr; drawn_b = pa.motor_inertia_rel_std != nullptr; }
  const bool table = pa.table != 0, use_k = pa.plant_stiffness || table || drawn_k, use_b = pa.plant_motor_inertia || table || drawn_b;
  double k_cj = 0.0, b_cj = 0.0, lb_c = 0.0, ub_c = 0.0, lb_s = 0.0, ub_s = 0.0; // (lb_s / ub_s: the stiffness row, VSA)
  if (table) team_table_row<NJ, NU, VSA>(traj_params_at(D, b), cj, B, k_cj, b_cj, lb_c, ub_c, lb_s, ub_s);
  if (pa.plant_stiffness) k_cj = pa.plant_stiffness[((size_t)cj * S + s) * B + b];
  if (pa.plant_motor_inertia) b_cj = 1.0 / pa.plant_motor_inertia[((size_t)cj * S + s) * B + b];
  if constexpr (DRAW) {
    // K_cj = Knom exp(sigma z), B_cj likewise: the nominal is the trajectory's row of the table (for B the reciprocal of the
    // row, which holds 1 / B), else the diagonal the models share (the host's fact)
    if (drawn_k) {
      k_cj = noise_settled((table ? k_cj : pa.knom[cj]) * exp(pa.stiffness_rel_std[(size_t)b * NJ + cj] * noise_entry(pa.key, kNoiseStiffness, 0, s, b, cj)));
      if (on && jl && pa.drawn_stiffness) pa.drawn_stiffness[((size_t)cj * S + s) * B + b] = k_cj;
    }
    if (drawn_b) {
      const double bi = noise_settled((table ? 1.0 / b_cj : pa.bnom[cj]) * exp(pa.motor_inertia_rel_std[(size_t)b * NJ + cj] * noise_entry(pa.key, kNoiseMotorInertia, 0, s, b, cj)));
      if (on && jl && pa.drawn_motor_inertia) pa.drawn_motor_inertia[((size_t)cj * S + s) * B + b] = bi;
      b_cj = 1.0 / bi;
    }
  }
  double Krow[NJ], Srow[NJ], Brow[NJ], dt = 0.0;
  ASLR_UNROLL for (int j = 0; j < NJ; ++j) { Krow[j] = 0.0; Srow[j] = 0.0; Brow[j] = 0.0; }
  bool has_lim = false;
  int m_loaded = -1;

  __shared__ double jtab[8][12];
  stage_joint_table<NJ>(jtab, ch, threadIdx.x);
  __syncthreads();

  // x0 (+ the sample's offset) into the team's state
  ASLR_UNROLL for (int k = 0; k < 4; ++k) {
    const int e = c + 8 * k;
    if (e < NX) {
      double v = a.x0[(size_t)b * NX + e];
      if (pa.dx0) v += pa.dx0[((size_t)s * B + b) * NX + e]; // (no `+ 0.0` without it: the sign of a zero is a bit too)
      if constexpr (DRAW) {
        if (pa.dx0_std) {
          const double d = noise_settled(pa.dx0_std[(size_t)b * NX + e] * noise_entry(pa.key, kNoiseDx0, 0, s, b, e));
          v += d;
          if (on && pa.drawn_dx0) pa.drawn_dx0[((size_t)s * B + b) * NX + e] = d;
        }
      }
      xT[e] = v;
    }
  }
  // the disturbance of the knot ahead, this lane's entries cj, NJ + cj, 2 NJ + cj, 3 NJ + cj of the state
  const double *wsrc = pa.disturbance ? pa.disturbance + ((size_t)s * T * B + b) * NX + cj : nullptr; // knot t at + t B NX
  double wn[4] = {0.0, 0.0, 0.0, 0.0};
  auto load_w = [&](int t) {
    ASLR_UNROLL for (int k = 0; k < 4; ++k) wn[k] = wsrc[(size_t)t * B * NX + k * NJ];
  };
  if (wsrc && T > 0) load_w(0);
  // the drawing form: wdraw stands where wsrc does; the lane's four entries of the row of knot t are drawn where they would
  // be loaded and, when drawn_disturbance is given, stored with the optional stores of the knot
  bool wdraw = false;
  double wsd[4] = {0.0, 0.0, 0.0, 0.0};
  double *wd_o = nullptr;
  if constexpr (DRAW) {
    wdraw = pa.noise_std != nullptr;
    if (wdraw) {
      ASLR_UNROLL for (int k = 0; k < 4; ++k) wsd[k] = pa.noise_std[(size_t)b * NX + cj + k * NJ];
      if (pa.drawn_disturbance) wd_o = pa.drawn_disturbance + ((size_t)s * T * B + b) * NX + cj;
    }
  }
  auto draw_w = [&](int t) {
    if constexpr (DRAW) {
      ASLR_UNROLL for (int k = 0; k < 4; ++k) wn[k] = noise_settled(wsd[k] * noise_entry(pa.key, kNoiseDisturbance, t, s, b, cj + k * NJ));
    }
  };
  auto store_w = [&](int t) { // wn, the row of knot t
    if (on && jl && wd_o) { ASLR_UNROLL for (int k = 0; k < 4; ++k) wd_o[(size_t)t * B * NX + k * NJ] = wn[k]; }
  };
  if (wdraw && T > 0) { draw_w(0); store_w(0); }
  double *xs_o = pa.xs_closed ? pa.xs_closed + ((size_t)s * (T + 1) * B + b) * NX : nullptr; // knot t at + t B NX
  double *us_o = pa.us_closed ? pa.us_closed + ((size_t)s * T * B + b) * NU : nullptr;
  auto store_x = [&](int t) { // the team's state as row t of xs_closed, 4 contiguous entries per lane
    if (on && jl && xs_o) team_store_state_row(xs_o + (size_t)t * B * NX + 4 * c, xT, c);
  };
  const typename Chain3D<NJ>::Consts cc(D, true);
  ModelRegs<NJ, NU> mr; // (the cost stack reads none of it)

  double J = 0.0;
  int failed = -1;
  prefetch(0);
  for (int t = 0; t <= T; ++t) {
    wave_sync(); // the previous knot's readers of the stage are done, its state is written
    ASLR_UNROLL for (int q = 0; q < NSLOT; ++q) { if (lane + 64 * q < STG) stg[lane + 64 * q] = pf[q]; }
    const int mi = node_model_at(a, t);
    wave_sync();
    const DevModel &dm = D.models[mi];
    if (t < T && mi != m_loaded) { // wave-uniform: model constants and control limits, re-read only when the model changes
      dt = dm.m.dt;
      team_model_rows<NJ, NU, VSA>(dm, cj, pa.diagonal, use_k, k_cj, use_b, b_cj, Krow, Srow, Brow);
      has_lim = lim.has[mi] != 0;
      if (!table) {
        lb_c = lim.lb[mi][cj];
        ub_c = lim.ub[mi][cj];
        if (VSA) { lb_s = lim.lb[mi][NJ + cj]; ub_s = lim.ub[mi][NJ + cj]; }
      }
      m_loaded = mi;
    }
    // ---- control law, row cj: u = us - K (x - xs), box clamp when asked for ----
    double u_c = 0.0, u_s = 0.0; // this lane's entries of the applied control (u_s: the stiffness command, VSA)
    if (t < T) {
      u_c = stg[oU + cj];
      ASLR_UNROLL for (int jx = 0; jx < NX; ++jx) u_c -= stg[oK + cj * NX + jx] * (xT[jx] - stg[oXr + jx]);
      if (pa.clamp && has_lim) u_c = fmin(fmax(u_c, lb_c), ub_c);
      if (jl) uT[c] = u_c;
      if constexpr (VSA) { // row NJ + cj: the stiffness command of joint cj
        u_s = stg[oU + NJ + cj];
        ASLR_UNROLL for (int jx = 0; jx < NX; ++jx) u_s -= stg[oK + (NJ + cj) * NX + jx] * (xT[jx] - stg[oXr + jx]);
        if (pa.clamp && has_lim) u_s = fmin(fmax(u_s, lb_s), ub_s);
        if (jl) uT[NJ + c] = u_s;
      }
    }
    wave_sync();
    // ---- node cost of the team's knot: its state and the applied control; the terminal node with the model's "u is None"
    // default.  One call site for both, BEFORE the loads of the next knot are issued: the cost stack reads its terms from
    // global memory, and behind those loads its waits would be waits for the prefetch ----
    {
      double x[NX], u[NU], xnext[NX], cst = 0.0;
      ASLR_UNROLL for (int i = 0; i < NX; ++i) x[i] = xT[i];
      ASLR_UNROLL for (int i = 0; i < NU; ++i) u[i] = uT[i];
      knot_eval<NJ, DAM, kEvalCost, Chain3D<NJ>>(cc, mr, dm, a.frame_ref ? stg + oFr : nullptr, x, t < T ? u : nullptr, xnext, cst, nullptr);
      J += cst; // (knot order)
    }
    if (t == T) { store_x(t); break; }
    double w[4];
    ASLR_UNROLL for (int k = 0; k < 4; ++k) w[k] = wn[k];
    prefetch(t + 1); // in flight while the dynamics of knot t compute
    if (wsrc && t + 1 < T) load_w(t + 1);
    if (wdraw && t + 1 < T) { draw_w(t + 1); store_w(t + 1); }
    // (the optional stores of a knot go out after the loads of the next one)
    store_x(t);
    if (on && jl && us_o) {
      us_o[(size_t)t * B * NU + c] = u_c;
      if constexpr (VSA) us_o[(size_t)t * B * NU + NJ + c] = u_s;
    }
    // ---- the plant step (aslr_team_step.hpp) ----
    ts.rotation(jtab);
    wave_sync();
    ts.torques(Krow, Srow);
    ts.mass_columns(chc);
    wave_sync();
    ts.minv_column();
    wave_sync();
    double nxt[4]; // this lane's entries {q_l, v_l, q_m, v_m} of xnext
    const bool bad = ts.euler(Brow, dt, nxt);
    if ((__ballot(bad) & team_bits) && failed < 0) failed = t; // NaN / Inf / |xnext|_inf >= 1e30, as the solver's rollout
    wave_sync(); // every lane of the team has read the old state
    if (jl) {
      if (wsrc || wdraw) { xT[c] = nxt[0] + w[0]; xT[NJ + c] = nxt[2] + w[1]; xT[2 * NJ + c] = nxt[1] + w[2]; xT[3 * NJ + c] = nxt[3] + w[3]; }
      else { xT[c] = nxt[0]; xT[NJ + c] = nxt[2]; xT[2 * NJ + c] = nxt[1]; xT[3 * NJ + c] = nxt[3]; }
    }
  }
  if (!on) return;
  const size_t sb = (size_t)s * B + b;
  if (c == 0) {
    if (pa.cost) pa.cost[sb] = failed >= 0 ? NAN : J;
    if (pa.failed_knot) pa.failed_knot[sb] = failed;
  }
  // (the state of knot T: nothing has written it since the loop's last fence)
  if (jl && pa.x_final) team_store_state_row(pa.x_final + sb * NX + 4 * c, xT, c);
}

// the nx = 28 sizes: grid (trajectories, groups of 16 samples), one block = 2 waves of 8 teams.  One launcher body for both
// argument types.
template <int NJ, int DAM, class PA>
int launch_policy_rollout_team(const KArgs &k, const ModelLimits &lim, const PA &pa, hipStream_t st) {
  const dim3 grid(k.B, (pa.S + 15) / 16), block(128);
  hipLaunchKernelGGL((policy_rollout_team_kernel<NJ, DAM, PA>), grid, block, 0, st, k, lim, pa);
  HIP_TRY(hipGetLastError());
  return ASLR_OK;
}

} // namespace aslr
