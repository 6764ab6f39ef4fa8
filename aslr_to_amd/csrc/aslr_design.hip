// aslr_design.hip -- the outer step of aslr_design_descent (include/aslr_to_amd_design.h):
// design_step_kernel, what lies between the gradient sweep of one outer step and the solve of the next.
//
// One 256-thread block per trajectory.  Lane 0 reads the cost of the finalized candidate and its gradient, decides
// (evaluable? accepted?), updates the accepted design, its cost, its gradient and the step length, and writes the next
// candidate into the trajectory's column of TRAJ_PARAMS; its decision reaches the other lanes through LDS.  Then all lanes
// stride over the trajectory's XS / US words -- to the best plan when the candidate was accepted, from it otherwise -- and
// zero the trajectory's GAPS / VXXF / KFF, as mpc_advance_kernel does for the next solve of a receding-horizon run.
//
// The arithmetic of the rule is stated operation by operation (tests/_design.py restates it in numpy and must reproduce
// the bits): every product and sum is rounded on its own.  The operations are the explicitly rounded intrinsics, and the
// Makefile compiles this unit with -ffp-contract=off: the intrinsics are inline functions of the HIP headers, and under the
// compiler's default their bodies are fused with their neighbours after inlining.
#include "aslr_common.hpp"

namespace aslr {

namespace {

// theta_try_j from the accepted entry, its gradient and the step length: a step of -eta in z_j = log theta_j to first
// order, limited to max_rel in relative size, then to [lo, hi].  The comparisons let a NaN through unchanged.
__device__ __forceinline__ double design_candidate(double th, double g, double eta, double max_rel, double lo, double hi) {
  double dz = -__dmul_rn(eta, __dmul_rn(th, g));
  dz = dz < -max_rel ? -max_rel : (dz > max_rel ? max_rel : dz);
  const double t = __dmul_rn(th, __dadd_rn(1.0, dz));
  return t < lo ? lo : (t > hi ? hi : t);
}

__global__ void __launch_bounds__(256) design_step_kernel(DesignStepArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x, B = a.B, T = a.T, nx = a.nx, nu = a.nu, nj = a.nj;
  __shared__ int to_best; // 1: XS / US -> xs_best / us_best, 0: the other way
  if (tid == 0) {
    const double J = a.traj_f[(size_t)ASLR_TF_COST * B + b];
    const double eta_in = a.s == 0 ? a.eta0 : a.eta[b];
    const bool frozen = a.s > 0 && eta_in < 0.0;
    const bool stepped = a.s > 0 && !frozen; // the candidate differs from the accepted design: it came from a step of eta_in
    // ---- evaluable?  the predicted decrease of the step that produced the candidate ----
    bool evaluable = isfinite(J);
    double pred = 0.0;
    for (int r = 0; r < 2 * nj; ++r) {
      if (!(r < nj ? a.opt_k : a.opt_b)) continue;
      const size_t i = (size_t)r * B + b;
      evaluable = evaluable && isfinite(a.grad[i]);
      if (stepped) {
        const double th = a.theta[i], g = a.g_acc[i];
        const double tt = design_candidate(th, g, eta_in, a.max_rel, a.lo[i], a.hi[i]);
        pred = __dadd_rn(pred, __dmul_rn(g, __dsub_rn(tt, th)));
      }
    }
    // ---- the decision ----
    bool accept;
    if (a.s == 0) accept = evaluable;
    else if (frozen) accept = false;
    else accept = evaluable && J <= __dadd_rn(a.cost_best[b], __dmul_rn(a.c1, pred));
    const bool freeze = frozen || (a.s == 0 && !evaluable);
    const double eta_out = freeze ? -1.0 : __dmul_rn(eta_in, accept ? a.grow : a.shrink);
    if (a.hist_f) {
      a.hist_f[b] = J;
      a.hist_f[(size_t)B + b] = stepped ? eta_in : 0.0;
      a.hist_f[2 * (size_t)B + b] = pred;
    }
    if (a.hist_i) a.hist_i[b] = (freeze || !evaluable) ? -1 : (accept ? 1 : 0);
    // ---- the accepted design; the next candidate into the trajectory's column of the table ----
    for (int r = 0; r < 2 * nj; ++r) {
      const size_t i = (size_t)r * B + b;
      const bool active = r < nj ? a.opt_k : a.opt_b;
      double th = a.theta[i];
      if (!active) {
        if (a.theta_hist) a.theta_hist[i] = th;
        continue;
      }
      double g = a.g_acc[i];
      const double tt = stepped ? design_candidate(th, g, eta_in, a.max_rel, a.lo[i], a.hi[i]) : th;
      if (a.theta_hist) a.theta_hist[i] = tt;
      if (accept) {
        th = tt; g = a.grad[i];
        a.theta[i] = th; a.g_acc[i] = g;
      } else if (a.s == 0) {
        a.g_acc[i] = 0.0; // (frozen: never read again, but defined)
      }
      const double next = (a.last || freeze) ? th : design_candidate(th, g, eta_out, a.max_rel, a.lo[i], a.hi[i]);
      // K as it is; the motor row is the reciprocal, by IEEE division like the host's row builder
      a.traj_params[i] = r < nj ? next : __ddiv_rn(1.0, next);
    }
    if (accept || a.s == 0) a.cost_best[b] = J;
    a.eta[b] = eta_out;
    to_best = accept || a.s == 0;
  }
  __syncthreads();
  const bool out = to_best != 0;
  for (int e = tid; e < (T + 1) * nx; e += 256) {
    const int t = e / nx, i = e - t * nx;
    const size_t w = ((size_t)t * B + b) * nx + i;
    if (out) a.xs_best[w] = a.xs[w]; else a.xs[w] = a.xs_best[w];
    a.gaps[w] = 0.0;
    a.vxxf[w] = 0.0;
  }
  for (int e = tid; e < T * nu; e += 256) {
    const int t = e / nu, i = e - t * nu;
    const size_t w = ((size_t)t * B + b) * nu + i;
    if (out) a.us_best[w] = a.us[w]; else a.us[w] = a.us_best[w];
    a.kff[w] = 0.0;
  }
}

} // namespace

int launch_design_step(const DesignStepArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(design_step_kernel, dim3(a.B), dim3(256), 0, st, a);
  HIP_TRY(hipGetLastError());
  return ASLR_OK;
}

} // namespace aslr
