// aslr_policy.inc.hpp -- closed-loop roll-outs of the stored policy on a perturbed plant (aslr_policy_rollout,
// include/aslr_to_amd_policy.h):
//
//   policy_rollout_kernel   16-lane team per trajectory as in rollout_kernel (aslr_forward.inc.hpp), but lane a is SAMPLE
//                           16 g + a of the trajectory instead of a step length: it rolls u_t = us_t - K_t (x_t - xs_t) out on
//                           its own plant (diagonals of K and B, initial-state offset, additive disturbance) and sums the
//                           node costs of its own closed loop in knot order, so nothing but S x B costs has to leave the
//                           device.  The policy [K | xs | us] and the knot's reference placement are what the 16 samples
//                           share: they arrive once per team, one knot ahead, through the same LDS-DMA double buffer.
//
// The kernel writes nothing but the caller's buffers: no workspace region, no solver state.
#pragma once
#include "aslr_common.hpp"
#include "aslr_policy_noise.hpp"

namespace aslr {

#ifndef ASLR_POLICY_FUSED
#define ASLR_POLICY_FUSED 1 // 1: dynamics and cost of a knot from one knot_eval; 0: two evaluations (dynamics, then cost alone)
#endif

// PA: where the perturbations come from.  PolicyArgs (the default): the caller's arrays.  PolicyNoiseArgs
// (aslr_policy_rollout_noise, the instantiations of aslr_policy_noise_nj2.hip): the lane draws them (aslr_policy_noise.hpp) at
// the places where the arrays are read, and writes them out where a drawn_* buffer is given.
template <int NJ, int DAM, bool PLANAR, class PA = PolicyArgs>
__global__ void __launch_bounds__(64) policy_rollout_kernel(KArgs a, ModelLimits lim, PA pa) {
  constexpr int NX = 4 * NJ, NU = ModelDims<NJ, DAM>::nu;
  constexpr bool DRAW = std::is_same_v<PA, PolicyNoiseArgs>;
  constexpr int TEAM = 16, TPW = 4;
  using CH = std::conditional_t<PLANAR, ChainPlanar<NJ>, Chain3D<NJ>>;
  const int lane = threadIdx.x, team = lane / TEAM, al = lane % TEAM;
  const int B = a.B, T = a.T, S = pa.S;
  // teams past B and lanes past S run on clamped indices (the arithmetic of a sample is the same instruction stream
  // wherever it sits); only their stores are guarded
  const int bq = blockIdx.x * TPW + team, sq = blockIdx.y * TEAM + al;
  const int b = bq < B ? bq : B - 1, s = sq < S ? sq : S - 1;
  const bool on = bq < B && sq < S;
  const DevDesc &D = *a.desc;

  double x[NX];
  {
    const double *x0 = a.x0 + (size_t)b * NX;
    ASLR_UNROLL for (int i = 0; i < NX; ++i) x[i] = x0[i];
    if (pa.dx0) { // (no `+ 0.0` without it: the sign of a zero is a bit too)
      const double *d0 = pa.dx0 + ((size_t)s * B + b) * NX;
      ASLR_UNROLL for (int p = 0; p < NX / 2; ++p) {
        const double2 v = *reinterpret_cast<const double2 *>(d0 + 2 * p);
        x[2 * p] += v.x; x[2 * p + 1] += v.y;
      }
    }
    if constexpr (DRAW) {
      if (pa.dx0_std) {
        const double *sd = pa.dx0_std + (size_t)b * NX;
        ASLR_UNROLL for (int p = 0; p < NX / 2; ++p) {
          double za, zb;
          noise_pair(pa.key, kNoiseDx0, 0, s, b, p, za, zb);
          const double2 v = make_double2(noise_settled(sd[2 * p] * za), noise_settled(sd[2 * p + 1] * zb));
          x[2 * p] += v.x; x[2 * p + 1] += v.y;
          if (on && pa.drawn_dx0) *reinterpret_cast<double2 *>(pa.drawn_dx0 + ((size_t)s * B + b) * NX + 2 * p) = v;
        }
      }
    }
  }
  // the plant of this lane: diag K and diag 1 / B -- the caller's arrays [nj][S][B] where given, else the trajectory's row
  // of the parameter table where one is set, else (use_k / use_b false) the diagonal of the knot's model
  bool drawn_k = false, drawn_b = false;
  if constexpr (DRAW) { drawn_k = pa.stiffness_rel_std != nullptr; drawn_b = pa.motor_inertia_rel_std != nullptr; }
  const bool table = pa.table != 0, use_k = pa.plant_stiffness || table || drawn_k, use_b = pa.plant_motor_inertia || table || drawn_b;
  double pk[NJ], pbinv[NJ], lim_lb[NU], lim_ub[NU];
  ASLR_UNROLL for (int i = 0; i < NJ; ++i) { pk[i] = 0.0; pbinv[i] = 0.0; }
  ASLR_UNROLL for (int i = 0; i < NU; ++i) { lim_lb[i] = 0.0; lim_ub[i] = 0.0; }
  if (table) {
    const double *tp = traj_params_at(D, b);
    ASLR_UNROLL for (int i = 0; i < NJ; ++i) { pk[i] = tp[(size_t)i * B]; pbinv[i] = tp[(size_t)(NJ + i) * B]; }
    ASLR_UNROLL for (int i = 0; i < NU; ++i) { lim_lb[i] = tp[(size_t)(2 * NJ + i) * B]; lim_ub[i] = tp[(size_t)(2 * NJ + NU + i) * B]; }
  }
  if (pa.plant_stiffness) {
    ASLR_UNROLL for (int i = 0; i < NJ; ++i) pk[i] = pa.plant_stiffness[((size_t)i * S + s) * B + b];
  }
  if (pa.plant_motor_inertia) {
    ASLR_UNROLL for (int i = 0; i < NJ; ++i) pbinv[i] = 1.0 / pa.plant_motor_inertia[((size_t)i * S + s) * B + b];
  }
  if constexpr (DRAW) {
    // K_j = Knom_j exp(sigma_j z), B_j likewise: the nominal is the trajectory's row of the table (for B the reciprocal of
    // the row, which holds 1 / B), else the diagonal the models share (the host's fact)
    ASLR_UNROLL for (int p = 0; p < (NJ + 1) / 2; ++p) {
      double z[2];
      if (drawn_k) {
        noise_pair(pa.key, kNoiseStiffness, 0, s, b, p, z[0], z[1]);
        ASLR_UNROLL for (int h = 0; h < 2; ++h) {
          const int i = 2 * p + h;
          if (i < NJ) {
            pk[i] = noise_settled((table ? pk[i] : pa.knom[i]) * exp(pa.stiffness_rel_std[(size_t)b * NJ + i] * z[h]));
            if (on && pa.drawn_stiffness) pa.drawn_stiffness[((size_t)i * S + s) * B + b] = pk[i];
          }
        }
      }
      if (drawn_b) {
        noise_pair(pa.key, kNoiseMotorInertia, 0, s, b, p, z[0], z[1]);
        ASLR_UNROLL for (int h = 0; h < 2; ++h) {
          const int i = 2 * p + h;
          if (i < NJ) {
            const double bi = noise_settled((table ? 1.0 / pbinv[i] : pa.bnom[i]) * exp(pa.motor_inertia_rel_std[(size_t)b * NJ + i] * z[h]));
            if (on && pa.drawn_motor_inertia) pa.drawn_motor_inertia[((size_t)i * S + s) * B + b] = bi;
            pbinv[i] = 1.0 / bi;
          }
        }
      }
    }
  }
  const typename CH::Consts cc(D, true);
  ModelRegs<NJ, NU> mr;
  int m_loaded = -1, lim_has = 0;

  // Per-knot inputs shared by the samples of a trajectory -- [K | xs | us | reference placement] -- fetched once per team,
  // one knot ahead, straight into LDS (the layout and the addressing of rollout_body: lane lt fetches the 16-byte pieces
  // lt and lt + 16; element e of team tm lands at (e / 32) * 128 + 32 tm + e % 32 of the parity buffer).  The placement
  // sits inside one row of 32 so that the cost stack reads it through one pointer.
  constexpr int oK = 0, oXr = oK + NU * NX, oU = oXr + NX, oEnd = oU + NU, BS = 2 * TEAM, DMAW = 128,
                oFr = (oEnd / BS == (oEnd + 11) / BS) ? oEnd : (oEnd + BS - 1) / BS * BS, NE = oFr + 12,
                NPI = (NE / 2 + TEAM - 1) / TEAM;
  static_assert(NU % 2 == 0 && NX % 2 == 0 && oFr % 2 == 0 && oFr / BS == (oFr + 11) / BS, "16-byte pieces; the placement in one row");
  __shared__ __attribute__((aligned(16))) double stgD[2][NPI * DMAW];
  const char *dsrc[NPI];
  size_t dstr[NPI];
  bool don[NPI], dctl[NPI], dref[NPI];
  ASLR_UNROLL for (int q = 0; q < NPI; ++q) {
    const int e = 2 * (al + TEAM * q); // first element of this lane's piece
    dsrc[q] = reinterpret_cast<const char *>(a.xs); dstr[q] = 0; don[q] = false; dctl[q] = false; dref[q] = false;
    if (e < oXr) { dsrc[q] = reinterpret_cast<const char *>(a.kgain + (size_t)b * NU * NX + e); dstr[q] = (size_t)B * NU * NX * 8; don[q] = true; dctl[q] = true; }
    else if (e < oU) { dsrc[q] = reinterpret_cast<const char *>(a.xs + (size_t)b * NX + (e - oXr)); dstr[q] = (size_t)B * NX * 8; don[q] = true; dctl[q] = true; }
    else if (e < oEnd) { dsrc[q] = reinterpret_cast<const char *>(a.us + (size_t)b * NU + (e - oU)); dstr[q] = (size_t)B * NU * 8; don[q] = true; dctl[q] = true; }
    else if (e >= oFr && e < NE && a.frame_ref) { dsrc[q] = reinterpret_cast<const char *>(a.frame_ref + (size_t)b * 12 + (e - oFr)); dstr[q] = (size_t)B * 12 * 8; don[q] = true; dref[q] = true; }
  }
  int mi_next = 0;
  auto prefetch = [&](int t) {
    unsigned base = lds_address(stgD[t & 1]);
    // (the drawing form feeds t to VALU work, and the compiler then keeps the knot counter in a vector register: the DMA's
    // M0 operand needs the scalar)
    if constexpr (DRAW) base = __builtin_amdgcn_readfirstlane(base);
    const size_t row = (size_t)min(a.ref_row0 + t, a.ref_last); // (the knot's row of the reference path)
    ASLR_UNROLL for (int q = 0; q < NPI; ++q) {
      if (don[q] && (!dctl[q] || t < T)) dma16<0, false>(dsrc[q] + (dref[q] ? row : (size_t)t) * dstr[q], base + q * DMAW * 8);
    }
    mi_next = node_model_at(a, t);
  };
  // the stores of a knot are issued AFTER the loads of the next one and may stay in flight over its wait (explicit vmcnt,
  // as in rollout_body); they are optional, so their number -- a lower bound of it -- is a run-time fact of the launch
  const int nst = (pa.xs_closed ? NX / 2 : 0) + (pa.us_closed ? NU / 2 : 0);
  const double *wsrc = pa.disturbance ? pa.disturbance + ((size_t)s * T * B + b) * NX : nullptr; // knot t at + t B NX
  double wn[NX]; // the disturbance of the knot ahead
  ASLR_UNROLL for (int i = 0; i < NX; ++i) wn[i] = 0.0;
  auto load_w = [&](int t) {
    ASLR_UNROLL for (int p = 0; p < NX / 2; ++p) {
      const double2 v = *reinterpret_cast<const double2 *>(wsrc + (size_t)t * B * NX + 2 * p);
      wn[2 * p] = v.x; wn[2 * p + 1] = v.y;
    }
  };
  if (wsrc && T > 0) load_w(0);
  // the drawing form: wdraw stands where wsrc does; the row of knot t is drawn where it would be loaded and, when
  // drawn_disturbance is given, stored with the optional stores of the knot (nsw of them, behind the loads of the prefetch)
  bool wdraw = false;
  int nsw = 0;
  double wsd[DRAW ? NX : 1];
  double *wd_o = nullptr;
  if constexpr (DRAW) {
    wdraw = pa.noise_std != nullptr;
    if (wdraw) {
      ASLR_UNROLL for (int i = 0; i < NX; ++i) wsd[i] = pa.noise_std[(size_t)b * NX + i];
      if (pa.drawn_disturbance) { wd_o = pa.drawn_disturbance + ((size_t)s * T * B + b) * NX; nsw = NX / 2; }
    }
  }
  auto draw_w = [&](int t) {
    if constexpr (DRAW) {
      ASLR_UNROLL for (int p = 0; p < NX / 2; ++p) {
        double za, zb;
        noise_pair(pa.key, kNoiseDisturbance, t, s, b, p, za, zb);
        wn[2 * p] = noise_settled(wsd[2 * p] * za); wn[2 * p + 1] = noise_settled(wsd[2 * p + 1] * zb);
      }
    }
  };
  auto store_w = [&](int t) { // wn, the row of knot t
    if (on && wd_o) {
      ASLR_UNROLL for (int p = 0; p < NX / 2; ++p)
        *reinterpret_cast<double2 *>(wd_o + (size_t)t * B * NX + 2 * p) = make_double2(wn[2 * p], wn[2 * p + 1]);
    }
  };
  if (wdraw && T > 0) { draw_w(0); store_w(0); }
  double *xs_o = pa.xs_closed ? pa.xs_closed + ((size_t)s * (T + 1) * B + b) * NX : nullptr; // knot t at + t B NX
  double *us_o = pa.us_closed ? pa.us_closed + ((size_t)s * T * B + b) * NU : nullptr;

  double J = 0.0;
  int failed = -1;
  prefetch(0);
  for (int t = 0; t <= T; ++t) {
    const int nsk = nst + (t < T ? nsw : 0); // (knot t - 1 stored a drawn row only if knot t has one)
    if (t == 0 || nsk == 0) wait_vmcnt<0>();
    else if (nsk >= NX / 2 + NU / 2) wait_vmcnt<NX / 2 + NU / 2>();
    else if (nsk >= NX / 2) wait_vmcnt<NX / 2>();
    else wait_vmcnt<NU / 2>();
    wave_sync();
    const double *stgT = stgD[t & 1] + team * BS;
    auto SH = [&](int e) -> double { return stgT[(e / BS) * DMAW + e % BS]; };
    const double *fref = a.frame_ref ? stgT + (oFr / BS) * DMAW + oFr % BS : nullptr;
    const int mi = mi_next;
    const DevModel &dm = D.models[mi];
    double w[NX];
    ASLR_UNROLL for (int i = 0; i < NX; ++i) w[i] = wn[i];
    if (t < T) {
      if (wsrc && t + 1 < T) load_w(t + 1); // in flight while knot t computes
      if (wdraw && t + 1 < T) draw_w(t + 1);
      prefetch(t + 1);
      if (wdraw && t + 1 < T) store_w(t + 1);
    }
    if (on && xs_o) {
      ASLR_UNROLL for (int p = 0; p < NX / 2; ++p)
        *reinterpret_cast<double2 *>(xs_o + (size_t)t * B * NX + 2 * p) = make_double2(x[2 * p], x[2 * p + 1]);
    }
    double xnext[NX], c = 0.0;
    if (t == T) { // terminal node: its cost with the model's "u is None" default
      knot_eval<NJ, DAM, kEvalCost, CH>(cc, mr, dm, fref, x, nullptr, xnext, c, nullptr);
      J += c;
      break;
    }
    double u[NU];
    ASLR_UNROLL for (int i = 0; i < NU; ++i) {
      double sm = SH(oU + i);
      ASLR_UNROLL for (int jx = 0; jx < NX; ++jx) sm -= SH(oK + i * NX + jx) * (x[jx] - SH(oXr + jx));
      u[i] = sm;
    }
    if (mi != m_loaded) { // wave-uniform: model constants and control limits, re-read only when the model changes
      mr.load(dm);
      m_loaded = mi;
      lim_has = lim.has[mi];
      if (pa.diagonal) { // (the host's fact: a plant array or a table, both of which need diagonal models)
        TrajDiag<NJ> d;
        ASLR_UNROLL for (int i = 0; i < NJ; ++i) { d.k[i] = use_k ? pk[i] : mr.K[i][i]; d.binv[i] = use_b ? pbinv[i] : mr.Binv[i][i]; }
        mr.set_traj(d);
      }
      if (!table) { ASLR_UNROLL for (int i = 0; i < NU; ++i) { lim_lb[i] = lim.lb[mi][i]; lim_ub[i] = lim.ub[mi][i]; } }
    }
    if (pa.clamp && lim_has) {
      ASLR_UNROLL for (int i = 0; i < NU; ++i) u[i] = fmin(fmax(u[i], lim_lb[i]), lim_ub[i]);
    }
    if (on && us_o) {
      ASLR_UNROLL for (int p = 0; p < NU / 2; ++p)
        *reinterpret_cast<double2 *>(us_o + (size_t)t * B * NU + 2 * p) = make_double2(u[2 * p], u[2 * p + 1]);
    }
#if ASLR_POLICY_FUSED
    knot_eval<NJ, DAM, kEvalDyn | kEvalCost, CH>(cc, mr, dm, fref, x, u, xnext, c, nullptr);
#else
    knot_eval<NJ, DAM, kEvalDyn, CH>(cc, mr, dm, nullptr, x, u, xnext, c, nullptr);
    knot_eval<NJ, DAM, kEvalCost, CH>(cc, mr, dm, fref, x, u, xnext, c, nullptr);
#endif
    J += c; // (applied control, knot order)
    double mx = 0.0;
    ASLR_UNROLL for (int i = 0; i < NX; ++i) mx += fabs(xnext[i]);
    if (inf_norm_bad<NX>(mx, xnext) && failed < 0) failed = t; // NaN / Inf / |xnext|_inf >= 1e30, as the solver's rollout
    if (wsrc || wdraw) { ASLR_UNROLL for (int i = 0; i < NX; ++i) x[i] = xnext[i] + w[i]; }
    else { ASLR_UNROLL for (int i = 0; i < NX; ++i) x[i] = xnext[i]; }
  }
  if (!on) return;
  const size_t sb = (size_t)s * B + b;
  if (pa.cost) pa.cost[sb] = failed >= 0 ? NAN : J;
  if (pa.failed_knot) pa.failed_knot[sb] = failed;
  if (pa.x_final) {
    ASLR_UNROLL for (int p = 0; p < NX / 2; ++p)
      *reinterpret_cast<double2 *>(pa.x_final + sb * NX + 2 * p) = make_double2(x[2 * p], x[2 * p + 1]);
  }
}

// the nx = 8 sizes; the 7-joint team form is policy_rollout_team_kernel (aslr_policy_team.inc.hpp, aslr_policy_rollout_all).
// One launcher body for both argument types.
template <int NJ, int DAM, class PA>
int launch_policy_rollout(const KArgs &k, const ModelLimits &lim, const PA &pa, hipStream_t st) {
  const dim3 grid((k.B + 3) / 4, (pa.S + 15) / 16), block(64);
  with_planar<NJ>(k, [&](auto P) {
    hipLaunchKernelGGL((policy_rollout_kernel<NJ, DAM, decltype(P)::value, PA>), grid, block, 0, st, k, lim, pa);
  });
  HIP_TRY(hipGetLastError());
  return ASLR_OK;
}

} // namespace aslr
