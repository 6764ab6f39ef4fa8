// aslr_team_step.hpp -- the plant step of the larger chain (7-DoF SEA / VSA) on A TEAM OF 8 LANES, one copy for the team
// kernels: rollout_team_kernel (aslr_forward_team.inc.hpp), policy_rollout_team_kernel (aslr_policy_team.inc.hpp) and
// mpc_plant_team_kernel (aslr_mpc_plant_team.inc.hpp) take every piece, phase 0 of dyn_team_kernel (aslr_calc_team.inc.hpp)
// the M columns, the M^-1 column and the accelerations.
//
// A knot of the 7-joint chain is 8 recursive Newton-Euler sweeps (one per column of the joint-space inertia plus the
// nonlinear effects) followed by a 7 x 7 inverse; in one lane its ~170 live doubles spill, so it is spread over a team:
//
//   lane c < NJ : joint c's rotation, entry c of the coupling and motor torques, column c of M (RNEA with unit
//                 acceleration e_c, no velocity, no gravity: adding the exact zeros of the general recursion changes no
//                 bit), column c of M^-1, entry c of the accelerations and of the semi-implicit Euler step;
//   lane NJ     : the nonlinear effects (RNEA with the velocity and gravity, zero acceleration).
//
// All 8 lanes run ONE instruction stream (the general RNEA) on different inputs.  Team-shared data (state, control,
// torques, joint rotations, M, M^-1) lives in LDS at the offsets of a layout class (FwdTeam, CalcTeam); the teams of a
// wave never interact, so a wave-level LDS fence is the only synchronisation -- and the fences stay with the kernels, like
// everything in which they differ: what they issue between the pieces, the ballot over the team, what a failure records
// and the write-back of the new state.  VSA actuation (nu = 2 NJ: motor torques, then joint stiffnesses): the coupling
// torque of joint c uses the stiffness commanded at the knot (free_fwddyn_vsa.py:34-47; the arithmetic of
// knot_eval<..., ASLR_DAM_VSA>).
#pragma once
#include "aslr_common.hpp"

namespace aslr {

// RNEA(q, v, a) of rnea<NJ, false>() with the joint rotations read from LDS (Rl[NJ][9], row-major)
template <int NJ>
ASLR_DEV void rnea_lds(chain_cp cp, const double *Rl, const double (&vv)[NJ], const double (&aa)[NJ], V3 grav,
                       double (&tau)[NJ]) {
  SV vp = sv_zero(), ap = SV{neg(grav), V3{0, 0, 0}};
  SV f[NJ];
  ASLR_UNROLL for (int i = 0; i < NJ; ++i) {
    SE3d X;
    X.R = m3(Rl + 9 * i);
    X.p = v3(cp->joint_p[i]);
    const V3 ax = v3(cp->axis[i]);
    const SV vJ = SV{V3{0, 0, 0}, vv[i] * ax};
    const SV Xv = motion_actinv(X, vp);
    const SV vi = Xv + vJ;
    const SV Xa = motion_actinv(X, ap);
    SV ai = Xa + crm(vi, vJ);
    ai.ang = ai.ang + aa[i] * ax;
    const V3 com = v3(cp->com[i]);
    const M3 I = m3(cp->inertia[i]);
    const SV h = inertia_mul(cp->mass[i], com, I, vi);
    f[i] = inertia_mul(cp->mass[i], com, I, ai) + crf(vi, h);
    vp = vi;
    ap = ai;
  }
  ASLR_UNROLL for (int i = NJ - 1; i >= 0; --i) {
    tau[i] = dot(v3(cp->axis[i]), f[i].ang);
    if (i > 0) {
      SE3d X;
      X.R = m3(Rl + 9 * i);
      X.p = v3(cp->joint_p[i]);
      f[i - 1] = f[i - 1] + force_act(X, f[i]);
    }
  }
}

// column jc (runtime) of A^-1 exactly as spd_inverse_fast<N>() computes it (terms it skips are exact zeros here)
template <int N>
ASLR_DEV void spd_inverse_col(const double (&A)[N][N], int jc, double (&e)[N]) {
  double L[N][N], rinv[N];
  ASLR_UNROLL for (int j = 0; j < N; ++j) {
    double d = A[j][j];
    ASLR_UNROLL for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    d = sqrt(d);
    L[j][j] = d;
    rinv[j] = 1.0 / d;
    ASLR_UNROLL for (int i = j + 1; i < N; ++i) {
      double s = A[i][j];
      ASLR_UNROLL for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
      L[i][j] = s * rinv[j];
    }
  }
  ASLR_UNROLL for (int i = 0; i < N; ++i) {
    double s = (i == jc) ? 1.0 : 0.0;
    ASLR_UNROLL for (int k = 0; k < i; ++k) s -= L[i][k] * e[k];
    e[i] = (i < jc) ? 0.0 : s * rinv[i];
  }
  ASLR_UNROLL for (int i = N - 1; i >= 0; --i) {
    double s = e[i];
    ASLR_UNROLL for (int k = i + 1; k < N; ++k) s -= L[k][i] * e[k];
    e[i] = s * rinv[i];
  }
}

template <int NJ, int DAM = ASLR_DAM_SEA>
struct FwdTeam {
  static_assert(NJ >= 2 && NJ <= 7, "team of 8 lanes: NJ inertia columns + the nonlinear effects");
  static constexpr bool VSA = DAM == ASLR_DAM_VSA;
  static constexpr int NX = 4 * NJ, NU = VSA ? 2 * NJ : NJ;
  // per-wave stage (doubles): K, us, k, xs, gaps, Vxx f of the current knot
  static constexpr int oK = 0, oU = oK + NU * NX, oKf = oU + NU, oXr = oKf + NU, oFg = oXr + NX, oVf = oFg + NX,
                       STG = (oVf + NX + 1) / 2 * 2;
  static constexpr int NSLOT = (STG + 63) / 64;
  // per-team arrays (doubles)
  static constexpr int tX = 0, tU = tX + NX, tTc = tU + (VSA ? 16 : 8), tTm = tTc + 8, tR = tTm + 8, tM = tR + (NJ * 9 + 1) / 2 * 2,
                       tMi = tM + 8 * 8, TEAM_LDS = tMi + 8 * 8;
};

// The step of lane c of the team whose arrays start at tm_ (LDS), piece by piece; L gives the offsets (FwdTeam, CalcTeam).
template <int NJ, bool VSA, class L>
struct TeamStep {
  double *xT, *uT, *tcL, *tmL, *RL, *ML, *MiL;
  int c, cj; // cj: the joint / row this lane owns (lane NJ computes on NJ - 1 and stores nothing)
  bool jl;
  ASLR_DEV TeamStep(double *tm_, int c_)
      : xT(tm_ + L::tX), uT(tm_ + L::tU), tcL(tm_ + L::tTc), tmL(tm_ + L::tTm), RL(tm_ + L::tR), ML(tm_ + L::tM), MiL(tm_ + L::tMi),
        c(c_), cj(c_ < NJ ? c_ : NJ - 1), jl(c_ < NJ) {}

  // rotation of joint cj into RL; jtab: stage_joint_table's
  ASLR_DEV void rotation(const double (*jtab)[12]) const {
    if (jl) {
      const M3 R = mul(m3(jtab[cj]), axis_angle(v3(jtab[cj] + 9), xT[cj]));
      ASLR_UNROLL for (int k = 0; k < 9; ++k) RL[9 * c + k] = R.a[k];
    }
  }
  // coupling and motor torques, entry cj
  ASLR_DEV void torques(const double (&Krow)[NJ], const double (&Srow)[NJ]) const {
    if (jl) {
      double s = 0.0, s2 = 0.0;
      if constexpr (VSA) { // K = diag(stiffness commands), tau_m = the torque commands (the sum over the zeros of K included)
        ASLR_UNROLL for (int j = 0; j < NJ; ++j) s += (j == c ? uT[NJ + c] : 0.0) * (xT[j] - xT[NJ + j]);
        s2 = uT[c];
      } else {
        ASLR_UNROLL for (int j = 0; j < NJ; ++j) { s += Krow[j] * (xT[j] - xT[NJ + j]); s2 += Srow[j] * uT[j]; }
      }
      tcL[c] = s;
      tmL[c] = s2;
    }
  }
  // one RNEA per lane: column c of M (lanes c < NJ), nonlinear effects (lane NJ)
  ASLR_DEV void mass_columns(chain_cp chc) const {
    if (c <= NJ) {
      double vv[NJ], aa[NJ], tau[NJ];
      const bool nl = c == NJ;
      ASLR_UNROLL for (int i = 0; i < NJ; ++i) { vv[i] = nl ? xT[2 * NJ + i] : 0.0; aa[i] = (!nl && i == c) ? 1.0 : 0.0; }
      const V3 g = v3(chc->gravity);
      const V3 grav = nl ? g : V3{0.0, 0.0, 0.0};
      rnea_lds<NJ>(chc, RL, vv, aa, grav, tau);
      ASLR_UNROLL for (int i = 0; i < NJ; ++i) ML[8 * c + i] = tau[i];
    }
  }
  // column cj of M^-1 (M symmetrised like Chain3D::mass) into MiL; OUT (dyn_team_kernel's DYN record): the lanes with
  // `store` set also write entry i to o[i * stride].  The column stays local to this member: handed out through a reference
  // parameter it cost rollout_team_kernel 16 to 48 scalar spills and 2.7 % of the forward pass (profiles/team_step/)
  template <bool OUT = false>
  ASLR_DEV void minv_column(double *o = nullptr, int stride = 0, bool store = false) const {
    double Ms[NJ][NJ], e[NJ];
    ASLR_UNROLL for (int i = 0; i < NJ; ++i)
      ASLR_UNROLL for (int j = 0; j <= i; ++j) {
        Ms[i][j] = (i == j) ? ML[8 * j + i] : 0.5 * (ML[8 * j + i] + ML[8 * i + j]);
        Ms[j][i] = Ms[i][j];
      }
    spd_inverse_col<NJ>(Ms, cj, e);
    if (jl) {
      ASLR_UNROLL for (int i = 0; i < NJ; ++i) MiL[8 * c + i] = e[i];
      if constexpr (OUT) { if (store) { ASLR_UNROLL for (int i = 0; i < NJ; ++i) o[i * stride] = e[i]; } }
    }
  }
  // accelerations, entry cj: link side and motor side
  ASLR_DEV void accelerations(const double (&Brow)[NJ], double &al, double &am) const {
    al = 0.0;
    am = 0.0;
    ASLR_UNROLL for (int j = 0; j < NJ; ++j) {
      al += MiL[8 * j + cj] * (-ML[8 * NJ + j] - tcL[j]);
      am += Brow[j] * (tmL[j] + tcL[j]);
    }
  }
  // semi-implicit Euler, entries cj of q_l, v_l, q_m, v_m into nxt (the caller writes them back behind a fence).  True: this
  // lane's entries of xnext hold a NaN / Inf / >= 1e30 (the |xnext|_inf test of the solver's rollout, entry by entry)
  ASLR_DEV bool euler(const double (&Brow)[NJ], double dt, double (&nxt)[4]) const {
    double al, am;
    accelerations(Brow, al, am);
    const double ql = xT[cj], qm = xT[NJ + cj], vl = xT[2 * NJ + cj], vm = xT[3 * NJ + cj];
    const double nql = ql + (vl * dt + al * dt * dt), nvl = vl + al * dt;
    const double nqm = qm + (vm * dt + am * dt * dt), nvm = vm + am * dt;
    nxt[0] = nql; nxt[1] = nvl; nxt[2] = nqm; nxt[3] = nvm;
    return jl && inf_norm_bad<4>(fabs(nql) + fabs(nvl) + fabs(nqm) + fabs(nvm), nxt);
  }
};

// lane cj's entries of a trajectory's row of the parameter table (tp: traj_params_at): K[cj][cj] and 1 / B[cj][cj] ...
template <int NJ>
ASLR_DEV void team_table_row(const double *tp, int cj, int B, double &k_cj, double &b_cj) {
  k_cj = tp[(size_t)cj * B];
  b_cj = tp[(size_t)(NJ + cj) * B];
}
// ... and its bounds (lb_s / ub_s: the stiffness row, VSA)
template <int NJ, int NU, bool VSA>
ASLR_DEV void team_table_row(const double *tp, int cj, int B, double &k_cj, double &b_cj, double &lb_c, double &ub_c,
                             double &lb_s, double &ub_s) {
  team_table_row<NJ>(tp, cj, B, k_cj, b_cj);
  lb_c = tp[(size_t)(2 * NJ + cj) * B];
  ub_c = tp[(size_t)(2 * NJ + NU + cj) * B];
  if (VSA) { lb_s = tp[(size_t)(3 * NJ + cj) * B]; ub_s = tp[(size_t)(3 * NJ + NU + cj) * B]; }
}

// joint placements and axes: constants of the chain, staged once in LDS (as global loads inside the knot loop they cost a
// vmcnt(0) per knot, which also waits for the prefetch issued just before; in registers they spill).  The caller fences.
template <int NJ>
ASLR_DEV void stage_joint_table(double (*jtab)[12], const aslr_chain_t &ch, int lane) {
  if (lane < NJ) {
    ASLR_UNROLL for (int k = 0; k < 9; ++k) jtab[lane][k] = ch.joint_R[lane][k];
    ASLR_UNROLL for (int k = 0; k < 3; ++k) jtab[lane][9 + k] = ch.axis[lane][k];
  }
}

// rows cj of K, S and B^-1 of a plant kernel's team: with `diagonal` (the host's fact: a plant array or a table, both of
// which need diagonal models) one entry on the diagonal -- the plant's where use_k / use_b say so, else the model's -- and
// literal zeros; without it the model's full row, so a non-diagonal model without a plant argument still rolls out
template <int NJ, int NU, bool VSA>
ASLR_DEV void team_model_rows(const DevModel &dm, int cj, bool diagonal, bool use_k, double k_cj, bool use_b, double b_cj,
                              double (&Krow)[NJ], double (&Srow)[NJ], double (&Brow)[NJ]) {
  ASLR_UNROLL for (int j = 0; j < NJ; ++j) {
    if (!VSA) {
      Krow[j] = diagonal ? ((j == cj) ? (use_k ? k_cj : dm.m.K[cj * NJ + cj]) : 0.0) : dm.m.K[cj * NJ + j];
      Srow[j] = dm.m.S[cj * NU + j];
    } else {
      Krow[j] = 0.0; Srow[j] = 0.0;
    }
    Brow[j] = diagonal ? ((j == cj) ? (use_b ? b_cj : dm.Binv[cj * NJ + cj]) : 0.0) : dm.Binv[cj * NJ + j];
  }
}

// entries 4c .. 4c + 3 of the team's state to o (this lane's piece of a state row), as two 16-byte stores
ASLR_DEV void team_store_state_row(double *o, const double *xT, int c) {
  *reinterpret_cast<double2 *>(o) = make_double2(xT[4 * c], xT[4 * c + 1]);
  *reinterpret_cast<double2 *>(o + 2) = make_double2(xT[4 * c + 2], xT[4 * c + 3]);
}

} // namespace aslr
