// aslr_forward_team.inc.hpp -- rollout of the larger chain (7-DoF SEA / VSA): A TEAM OF 8 LANES PER (trajectory, alpha).
//
// Same arithmetic as rollout_kernel (aslr_forward.inc.hpp) -- SolverDDP / FDDP / BoxDDP forwardPass, SURVEY.md
// B.2, B.4, B.5 -- with the knot evaluation spread over the lanes of the team: the plant step is TeamStep's
// (aslr_team_step.hpp, which also says which lane does what); on top of it lane c < NJ takes row c of the control law and
// of the box (rows c and NJ + c for VSA actuation, nu = 2 NJ).
//
// One block = 2 waves = the 10 step lengths of one trajectory (teams 10..15 idle): the C5 shard of 512 trajectories is
// 1024 waves, one per SIMD.  Per-knot inputs shared by the step lengths (K, k, us, xs, gaps, Vxx f) are staged per wave
// in LDS and prefetched one knot ahead.
#pragma once
#include "aslr_team_step.hpp"

namespace aslr {

// TP: this lane's diagonal entries of K / B^-1 and its bounds come from the trajectory's row of the parameter table, read
// once before the knot loop; a model change re-reads dt / S / has_u_limits only.
template <int NJ, bool FDDP, int DAM = ASLR_DAM_SEA, bool TP = false>
__global__ void __launch_bounds__(128) rollout_team_kernel(KArgs a, SolverDev sp, ModelLimits lim) {
  using C = FwdTeam<NJ, DAM>;
  constexpr int NX = C::NX, NU = C::NU, NSLOT = C::NSLOT;
  constexpr bool VSA = C::VSA;
  __shared__ double sm[2 * C::STG + 16 * C::TEAM_LDS];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, team = tid >> 3, c = tid & 7;
  const int B = a.B, T = a.T, b = a.b0 + blockIdx.x;
  int32_t *TI = a.traj_i;
  double *TF = a.traj_f;
  if (!sp.standalone && TI[ASLR_TI_DONE * B + b]) return;
  double *stg = sm + wv * C::STG, *tm_ = sm + 2 * C::STG + team * C::TEAM_LDS;
  const TeamStep<NJ, VSA, C> ts(tm_, c);
  double *const xT = ts.xT, *const uT = ts.uT;
  const bool team_on = team < ASLR_NALPHA;
  const int ai = team_on ? team : ASLR_NALPHA - 1;
  const double alpha = 1.0 / (double)(1 << ai);
  const int feasible = TI[ASLR_TI_FEASIBLE * B + b];
  const bool fddp = FDDP && sp.solver == ASLR_SOLVER_FDDP, box = sp.solver == ASLR_SOLVER_BOXDDP;
  const bool use_gaps = fddp && !(feasible || alpha == 1.0);
  const bool need_dv = fddp && !feasible;
  const bool jl = ts.jl; // this lane owns joint / row cj
  const int cj = ts.cj;
  const DevDesc &D = *a.desc;
  const aslr_chain_t &ch = D.chain;
  const chain_cp chc = chain_const(&D.chain);
  const size_t TB1 = (size_t)(T + 1) * B, TB = (size_t)T * B;
  const unsigned long long team_bits = 0xffull << ((lane >> 3) * 8);

  // ---- stage slots: element idx = lane + 64 q of [K | us | k | xs | gaps | Vxx f] at knot t ----
  const double *sp0[NSLOT];
  size_t sstr[NSLOT];
  bool son[NSLOT], sctl[NSLOT];
  ASLR_UNROLL for (int q = 0; q < NSLOT; ++q) {
    const int idx = lane + 64 * q;
    sp0[q] = a.xs; sstr[q] = 0; son[q] = false; sctl[q] = false;
    if (idx < C::oU) { sp0[q] = a.kgain + (size_t)b * NU * NX + idx; sstr[q] = (size_t)B * NU * NX; son[q] = true; sctl[q] = true; }
    else if (idx < C::oKf) { sp0[q] = a.us + (size_t)b * NU + (idx - C::oU); sstr[q] = (size_t)B * NU; son[q] = true; sctl[q] = true; }
    else if (idx < C::oXr) { sp0[q] = a.kff + (size_t)b * NU + (idx - C::oKf); sstr[q] = (size_t)B * NU; son[q] = true; sctl[q] = true; }
    else if (idx < C::oFg) { sp0[q] = a.xs + (size_t)b * NX + (idx - C::oXr); sstr[q] = (size_t)B * NX; son[q] = true; }
    else if (idx < C::oVf) { sp0[q] = a.gaps + (size_t)b * NX + (idx - C::oFg); sstr[q] = (size_t)B * NX; son[q] = need_dv; }
    else if (idx < C::oVf + NX) { sp0[q] = a.vxxf + (size_t)b * NX + (idx - C::oVf); sstr[q] = (size_t)B * NX; son[q] = need_dv; }
  }
  double pf[NSLOT];
  auto prefetch = [&](int t) {
    ASLR_UNROLL for (int q = 0; q < NSLOT; ++q) {
      pf[q] = 0.0;
      if (son[q] && (!sctl[q] || t < T)) pf[q] = sp0[q][(size_t)t * sstr[q]];
    }
  };

  // model rows of this lane (reloaded when the node's model changes; wave-uniform)
  double Krow[NJ], Srow[NJ], Brow[NJ], dt = 0.0, lb_c = 0.0, ub_c = 0.0, lb_s = 0.0, ub_s = 0.0; // (lb_s / ub_s: the stiffness row, VSA)
  bool has_lim = false;
  int m_loaded = -1;
  double k_cj = 0.0, b_cj = 0.0; // TP: K[cj][cj], 1 / B[cj][cj] of this trajectory
  if constexpr (TP) {
    team_table_row<NJ, NU, VSA>(traj_params_at(D, b), cj, B, k_cj, b_cj, lb_c, ub_c, lb_s, ub_s);
  }
  __shared__ double jtab[8][12];
  stage_joint_table<NJ>(jtab, ch, threadIdx.x);
  __syncthreads();

  // x0 into the team's state
  ASLR_UNROLL for (int k = 0; k < 4; ++k) {
    const int e = c + 8 * k;
    if (e < NX) xT[e] = a.x0[(size_t)b * NX + e];
  }
  double dv = 0.0;
  bool fail = false;
  ASLR_PROF_DECL;
  prefetch(0);
  for (int t = 0; t <= T; ++t) {
    const size_t tb = (size_t)t * B + b;
    ASLR_PROF(7);
    ASLR_PROF_COUNT(15);
    wave_sync(); // the previous knot's readers of the stage are done
    ASLR_UNROLL for (int q = 0; q < NSLOT; ++q) { if (lane + 64 * q < C::STG) stg[lane + 64 * q] = pf[q]; }
    const int mi = node_model_at(a, t);
    wave_sync();
    if (t < T) prefetch(t + 1);
    if (use_gaps) {
      ASLR_UNROLL for (int k = 0; k < 4; ++k) {
        const int e = c + 8 * k;
        if (e < NX) xT[e] = xT[e] + stg[C::oFg + e] * (alpha - 1.0);
      }
    }
    if (fddp) wave_sync();
    if (team_on && jl) { // candidate state, 4 contiguous entries per lane
      double *o = a.xs_try + ((size_t)ai * TB1 + tb) * NX + 4 * c;
      ASLR_UNROLL for (int k = 0; k < 4; ++k) o[k] = xT[4 * c + k];
    }
    if (need_dv && c == 0) { // dv -= fs . Vxx (xs - xs_try), summed in state order
      double s = 0.0;
      for (int i = 0; i < NX; ++i) s += stg[C::oVf + i] * (stg[C::oXr + i] - xT[i]);
      dv -= s;
    }
    if (t == T) break;
    const DevModel &dm = D.models[mi];
    if (mi != m_loaded) {
      dt = dm.m.dt;
      ASLR_UNROLL for (int j = 0; j < NJ; ++j) {
        if (!VSA) { Krow[j] = TP ? ((j == cj) ? k_cj : 0.0) : dm.m.K[cj * NJ + j]; Srow[j] = dm.m.S[cj * NU + j]; }
        Brow[j] = TP ? ((j == cj) ? b_cj : 0.0) : dm.Binv[cj * NJ + j];
      }
      has_lim = lim.has[mi] != 0;
      if constexpr (!TP) {
        lb_c = lim.lb[mi][cj];
        ub_c = lim.ub[mi][cj];
        if (VSA) { lb_s = lim.lb[mi][NJ + cj]; ub_s = lim.ub[mi][NJ + cj]; }
      }
      // the values are consumed HERE, so the wait for these loads sits inside this rarely-taken branch and not at
      // the join, where it would drain the prefetch of every knot
      if (VSA) { ASLR_UNROLL for (int j = 0; j < NJ; ++j) asm volatile("" : "+v"(Brow[j])); asm volatile("" : "+v"(lb_s), "+v"(ub_s)); }
      else { ASLR_UNROLL for (int j = 0; j < NJ; ++j) asm volatile("" : "+v"(Krow[j]), "+v"(Srow[j]), "+v"(Brow[j])); }
      asm volatile("" : "+v"(dt), "+v"(lb_c), "+v"(ub_c));
      m_loaded = mi;
    }
    ASLR_PROF(0);
    // ---- control law, row cj: u = us - alpha k - K (x - xs), box clamp ----
    {
      double s = stg[C::oU + cj] - stg[C::oKf + cj] * alpha;
      ASLR_UNROLL for (int jx = 0; jx < NX; ++jx) s -= stg[C::oK + cj * NX + jx] * (xT[jx] - stg[C::oXr + jx]);
      if (box && has_lim) s = fmin(fmax(s, lb_c), ub_c);
      if (jl) uT[c] = s;
      if (team_on && jl) a.us_try[((size_t)ai * TB + tb) * NU + c] = s;
      if constexpr (VSA) { // row NJ + cj: the stiffness command of joint cj
        double s2 = stg[C::oU + NJ + cj] - stg[C::oKf + NJ + cj] * alpha;
        ASLR_UNROLL for (int jx = 0; jx < NX; ++jx) s2 -= stg[C::oK + (NJ + cj) * NX + jx] * (xT[jx] - stg[C::oXr + jx]);
        if (box && has_lim) s2 = fmin(fmax(s2, lb_s), ub_s);
        if (jl) uT[NJ + c] = s2;
        if (team_on && jl) a.us_try[((size_t)ai * TB + tb) * NU + NJ + c] = s2;
      }
    }
    ASLR_PROF(1);
    // ---- the plant step (aslr_team_step.hpp), piece by piece ----
    ts.rotation(jtab);
    wave_sync();
    ASLR_PROF(2);
    ts.torques(Krow, Srow);
    ASLR_PROF(3);
    ts.mass_columns(chc);
    wave_sync();
    ASLR_PROF(4);
    ts.minv_column();
    wave_sync();
    ASLR_PROF(5);
    {
      double nxt[4]; // this lane's entries {q_l, v_l, q_m, v_m} of xnext
      const bool bad = ts.euler(Brow, dt, nxt);
      if (__ballot(bad) & team_bits) fail = true; // NaN / Inf / >= 1e30 in the state ("forward_error")
      wave_sync(); // every lane of the team has read the old state
      if (jl) { xT[c] = nxt[0]; xT[NJ + c] = nxt[2]; xT[2 * NJ + c] = nxt[1]; xT[3 * NJ + c] = nxt[3]; }
    }
  }
  ASLR_PROF(6);
  ASLR_PROF_FLUSH;
  if (team_on && c == 0) {
    TI[(ASLR_TI_TRYFAIL0 + ai) * B + b] = fail ? 1 : 0;
    TF[(ASLR_TF_DVTRY0 + ai) * B + b] = dv;
  }
}

} // namespace aslr
