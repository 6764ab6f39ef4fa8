// aslr_wave_gains.hpp -- control gains of ONE knot for a wide control vector (nu = 14: VSA on the 7-joint arm),
// worked by the lanes of ONE wavefront on operands that live in LDS
// (SolverDDP::computeGains, SolverBoxDDP::computeGains + BoxQP::solve).
//
// Why this exists: lane_gains<NU> / boxqp<NU> (aslr_backward.inc.hpp) keep Quu, the free-set factor and every work
// vector of the projected-Newton iteration in one lane's registers -- ~100 doubles at nu = 4, ~450 at nu = 14, which
// spills.  Here nothing but loop scalars lives in registers:
//
//   * Quu, q, the iterate x, its gradient, the 0/1 free mask, the bounds, the trial point and the factor L are LDS
//     arrays; lane i < nu owns ROW i of every matrix-vector product, of the masked matrix and of the factor
//     (one column of L per step, the pivot row read by every lane), and entry i of every element-wise update;
//   * the scalars that steer the iteration (|g|_inf over the free set, the number of free entries, f(x), the
//     line-search test) are sums over nu LDS entries that every lane forms in the same order: the wave holds ONE
//     problem, so every branch is wave-uniform by construction and needs no ballot;
//   * the one right-hand side of the Newton step is solved by lane 0, the nx + 1 solves with the FINAL free-set
//     factor (k and the columns of K) take one column per lane, L read from LDS at wave-uniform addresses.
//
// The arithmetic per ENTRY is that of boxqp<NU> / chol_rs / chol_solve_r and of the CPU restatement the tests check
// against (its BoxQP, chol, chol_solve): same operations, same order; the free / clamped split is carried by exact
// 0/1 masks as there (the masked matrix has the factor of Hff in its free block and identity rows elsewhere).  The
// iteration itself follows the oracle step for step -- first active-set test on the clamped warm start, Newton step on
// the free set, halving line search on the clamped step, stop on |g_f|_inf <= th_grad, an empty free set, a rejected
// line search or maxiter -- without the two shortcuts lane_gains<NU> takes for an interior start.
//
// The source is written in two kinds of sections so that it also compiles for the host, where the 64 lanes run one
// after the other (tests/host/wave_gains_emul.cpp): ASLR_WG_FOR(l, n) { ... } is executed by the lanes l < n, each
// writing only its own LDS slots; everything outside is wave-uniform (every lane computes the same value from LDS)
// and writes nothing.  ASLR_WG_SYNC() separates a section's LDS writes from their readers in other lanes.  The host
// build checks the distribution and the order of the arithmetic; it cannot see a missing ASLR_WG_SYNC().
#pragma once

#ifdef ASLR_WG_EMUL
#include <cmath>
#define ASLR_WG_FN inline
#define ASLR_WG_FOR(l, n) for (int l = 0; l < (n); ++l)
#define ASLR_WG_SYNC()
#define ASLR_WG_RSQRT(d) (1.0 / std::sqrt(d))
#define ASLR_WG_UNROLL
#define ASLR_WG_SCHED_FENCE()
#else
#define ASLR_WG_FN __device__ __forceinline__
#define ASLR_WG_FOR(l, n) if (const int l = (int)(threadIdx.x & 63u); l < (n))
#define ASLR_WG_SYNC() aslr::wave_sync()
#define ASLR_WG_RSQRT(d) rsqrt(d)
#define ASLR_WG_UNROLL _Pragma("unroll")
// the instruction scheduler does not move anything across this point: without it the unrolled substitutions issue
// the LDS reads of the whole factor ahead of their use and hold it in registers (scratch, next to the sweep's prefetch)
#define ASLR_WG_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
#endif

namespace aslr {

struct WaveQPParams {
  int maxiter;
  double th_acceptstep, th_grad, reg;
  int nalpha;
};

// LDS work space of wave_gains<NU, NX> (doubles).  Rows of L are LP = odd doubles apart: the lanes of a column step
// read one entry of their own row each, and an odd stride spreads them over the banks.
template <int NU>
struct WaveGainsLds {
  static constexpr int NUP = (NU + 1) / 2 * 2, LP = NU | 1;
  static constexpr int oX = 0, oG = oX + NUP, oMk = oG + NUP, oMkL = oMk + NUP, oLb = oMkL + NUP, oUb = oLb + NUP,
                       oXn = oUb + NUP, oTv = oXn + NUP, oGd = oTv + NUP, oDx = oGd + NUP, oRh = oDx + NUP,
                       oRinv = oRh + NUP, oKv = oRinv + NUP, oL = oKv + NUP, SIZE = (oL + NU * LP + 1) / 2 * 2;
};

// Factor of the masked matrix  mk_i mk_j H_ij + (1 - mk_i) delta_ij  (+ reg on the free diagonal) with rsqrt pivots,
// entry by entry the arithmetic of chol_rs<NU>.  Returns "a pivot was not positive" (wave-uniform).
template <int NU>
ASLR_WG_FN bool wave_factor(const double *H, double *w, double reg) {
  using W = WaveGainsLds<NU>;
  double *L = w + W::oL, *mk = w + W::oMk, *mkL = w + W::oMkL, *rinv = w + W::oRinv;
  ASLR_WG_FOR(i, NU) {
    const double mi = mk[i];
    mkL[i] = mi;
    ASLR_WG_UNROLL for (int j = 0; j < NU; ++j)
      L[i * W::LP + j] = (mi * mk[j]) * H[i * NU + j] + (i == j ? (mi * reg + (1.0 - mi)) : 0.0);
  }
  ASLR_WG_SYNC();
  bool bad = false;
  // (runtime loops on purpose: unrolled, the 14 column steps keep most of L in registers next to the sweep's prefetch)
  for (int j = 0; j < NU; ++j) {
    const double *Lj = L + j * W::LP;
    double d = Lj[j];
    for (int k = 0; k < j; ++k) d -= Lj[k] * Lj[k];
    if (!(d > 0.0)) bad = true;
    const double ri = ASLR_WG_RSQRT(d);
    ASLR_WG_FOR(i, NU) {
      if (i == j) {
        L[j * W::LP + j] = d * ri;
        rinv[j] = ri;
      } else if (i > j) {
        double *Li = L + i * W::LP;
        double s = Li[j];
        for (int k = 0; k < j; ++k) s -= Li[k] * Lj[k];
        Li[j] = s * ri;
      }
    }
    ASLR_WG_SYNC();
  }
  return bad;
}

// L L^T z = b on a register vector, L and the reciprocal pivots read from LDS: chol_solve_r<NU>
template <int NU>
ASLR_WG_FN void wave_solve(const double *w, double (&b)[NU]) {
  using W = WaveGainsLds<NU>;
  const double *L = w + W::oL, *rinv = w + W::oRinv;
  ASLR_WG_UNROLL for (int i = 0; i < NU; ++i) {
    double s = b[i];
    ASLR_WG_UNROLL for (int k = 0; k < i; ++k) s -= L[i * W::LP + k] * b[k];
    b[i] = s * rinv[i];
    if (i % 4 == 3) ASLR_WG_SCHED_FENCE();
  }
  ASLR_WG_UNROLL for (int i = NU - 1; i >= 0; --i) {
    double s = b[i];
    ASLR_WG_UNROLL for (int k = i + 1; k < NU; ++k) s -= L[k * W::LP + i] * b[k];
    b[i] = s * rinv[i];
    if (i % 4 == 3) ASLR_WG_SCHED_FENCE();
  }
}

// computeGains of one knot.
// In (LDS): H = Quu (nu x nu, regularised), q = Qu, Qux (nu x nx, row stride NX); for a boxed node lb / ub (the
// model's bounds minus the node's u) at w + oLb / oUb and the warm start k0 (the stored k).
// Out (LDS): w + oKv = k, K (nu x nx, row stride NX), q with the clamped entries zeroed; *iters = projected-Newton
// iterations as the oracle counts them (-1: not a boxed node).  Returns "backward_error" (wave-uniform).
template <int NU, int NX, bool BOXC>
ASLR_WG_FN bool wave_gains(const double *H, double *q, const double *Qux, double *K, double *w, bool boxed,
                           const double *k0, const WaveQPParams &P, int *iters) {
  using W = WaveGainsLds<NU>;
  double *x = w + W::oX, *g = w + W::oG, *mk = w + W::oMk, *xn = w + W::oXn, *tv = w + W::oTv, *gd = w + W::oGd,
         *dx = w + W::oDx, *rh = w + W::oRh, *kv = w + W::oKv;
  const double *mkL = w + W::oMkL, *lb = w + W::oLb, *ub = w + W::oUb;
  bool bad = false;
  int its = -1;
  if (BOXC && boxed) {
    // clamped warm start, its objective value f(x) = 1/2 x^T H x + q^T x and gradient q + H x
    ASLR_WG_FOR(i, NU) x[i] = fmax(fmin(k0[i], ub[i]), lb[i]);
    ASLR_WG_SYNC();
    ASLR_WG_FOR(i, NU) {
      double s = 0.0, sg = q[i];
      ASLR_WG_UNROLL for (int j = 0; j < NU; ++j) { s += H[i * NU + j] * x[j]; sg += H[i * NU + j] * x[j]; }
      tv[i] = 0.5 * x[i] * s + q[i] * x[i];
      g[i] = sg;
    }
    ASLR_WG_SYNC();
    double fold = 0.0;
    ASLR_WG_UNROLL for (int i = 0; i < NU; ++i) fold += tv[i];
    bool fresh = false; // the factor in LDS belongs to the mask in LDS
    for (its = 0; its < P.maxiter; ++its) {
      ASLR_WG_FOR(j, NU) {
        const bool at_lb = (x[j] == lb[j]) & (g[j] > 0.0), at_ub = (x[j] == ub[j]) & (g[j] < 0.0);
        mk[j] = (at_lb | at_ub) ? 0.0 : 1.0;
      }
      ASLR_WG_SYNC();
      double gnorm = 0.0, nfree = 0.0;
      bool same = fresh;
      ASLR_WG_UNROLL for (int j = 0; j < NU; ++j) {
        gnorm = fmax(gnorm, mk[j] * fabs(g[j]));
        nfree += mk[j];
        same = same && (mkL[j] == mk[j]);
      }
      fresh = same;
      if (gnorm <= P.th_grad || nfree == 0.0) break;
      // Newton step on the free subspace
      if (wave_factor<NU>(H, w, P.reg)) { bad = true; break; }
      fresh = true;
      ASLR_WG_FOR(i, NU) {
        double s = -q[i];
        ASLR_WG_UNROLL for (int j = 0; j < NU; ++j) s -= H[i * NU + j] * ((1.0 - mk[j]) * x[j]);
        rh[i] = mk[i] * s;
      }
      ASLR_WG_SYNC();
      ASLR_WG_FOR(l, 1) {
        double b[NU];
        ASLR_WG_UNROLL for (int i = 0; i < NU; ++i) b[i] = rh[i];
        wave_solve<NU>(w, b);
        ASLR_WG_UNROLL for (int i = 0; i < NU; ++i) dx[i] = mk[i] * (b[i] - x[i]);
      }
      ASLR_WG_SYNC();
      // halving line search on the clamped step
      double alpha = 1.0;
      bool found = false;
      for (int al = 0; al < P.nalpha; ++al, alpha *= 0.5) {
        ASLR_WG_FOR(i, NU) xn[i] = fmax(fmin(x[i] + alpha * dx[i], ub[i]), lb[i]);
        ASLR_WG_SYNC();
        ASLR_WG_FOR(i, NU) {
          double s = 0.0;
          ASLR_WG_UNROLL for (int j = 0; j < NU; ++j) s += H[i * NU + j] * xn[j];
          tv[i] = 0.5 * xn[i] * s + q[i] * xn[i];
          gd[i] = g[i] * (x[i] - xn[i]);
        }
        ASLR_WG_SYNC();
        double fnew = 0.0, gdot = 0.0;
        ASLR_WG_UNROLL for (int i = 0; i < NU; ++i) { fnew += tv[i]; gdot += gd[i]; }
        ASLR_WG_SYNC(); // (tv / gd / xn are rewritten by the next trial)
        if (fold - fnew > P.th_acceptstep * gdot) {
          ASLR_WG_FOR(i, NU) x[i] = xn[i];
          ASLR_WG_SYNC();
          fold = fnew;
          found = true;
          break;
        }
      }
      // No step length accepted: x is unchanged, so every remaining iteration would recompute the same gradient,
      // active set and rejected steps and return this x with this factor.  Stop here with that result.
      if (!found) { ++its; break; }
      ASLR_WG_FOR(i, NU) { // gradient at the new point, accumulated in the oracle's order (q first)
        double s = q[i];
        ASLR_WG_UNROLL for (int j = 0; j < NU; ++j) s += H[i * NU + j] * x[j];
        g[i] = s;
      }
      ASLR_WG_SYNC();
    }
    // factor of the final free block: the one at hand unless the active set changed in the last step
    if (!bad && !fresh) {
      double nfree = 0.0;
      ASLR_WG_UNROLL for (int j = 0; j < NU; ++j) nfree += mk[j];
      if (wave_factor<NU>(H, w, P.reg) && nfree > 0.0) bad = true;
    }
    ASLR_WG_FOR(i, NU) {
      kv[i] = -x[i];
      if (mk[i] == 0.0) q[i] = 0.0;
    }
  } else {
    // plain gains: every entry free, no regularisation (the mask form then reproduces Quu itself)
    ASLR_WG_FOR(i, NU) mk[i] = 1.0;
    ASLR_WG_SYNC();
    bad = wave_factor<NU>(H, w, 0.0);
  }
  ASLR_WG_SYNC();
  // K = Quu_inv Qux with Quu_inv = Hff^-1 on the free block and zero elsewhere: one column per lane; a plain node's k
  // = Quu^-1 Qu is one more column
  ASLR_WG_FOR(l, NX + 1) {
    const bool kcol = l == NX;
    if (!kcol || !(BOXC && boxed)) {
      double b[NU];
      ASLR_WG_UNROLL for (int c = 0; c < NU; ++c) b[c] = (kcol ? q[c] : Qux[c * NX + l]) * mk[c];
      wave_solve<NU>(w, b);
      ASLR_WG_UNROLL for (int c = 0; c < NU; ++c) {
        if (kcol) kv[c] = b[c] * mk[c];
        else K[c * NX + l] = b[c] * mk[c];
      }
    }
  }
  ASLR_WG_SYNC();
  if (iters) *iters = its;
  return bad;
}

} // namespace aslr
