// Host build of aslr_to_amd/csrc/aslr_wave_gains.hpp: the SAME template source the 7-joint VSA backward kernel
// instantiates for the lanes of a wavefront (nu = 14, operands in LDS) runs here with the 64 lanes one after the other
// on a plain array in place of LDS, so that the distribution of the gains / box QP over the lanes and the order of its
// arithmetic can be checked against the oracle's BoxQP (oracle/aslr_oracle.c, aslr_cpu_boxqp) without a GPU.  What it
// cannot check is the placement of the wave-level LDS fences.  Test infrastructure only (tests/test_vsa7_host.py
// builds it with g++).
#define ASLR_WG_EMUL 1
#include "../../aslr_to_amd/csrc/aslr_wave_gains.hpp"

namespace {
constexpr int NU = 14, NX = 28;
}

// One problem.  H [14][14], q / lb / ub / k0 [14], Qux [14][28] (control row, state column).
// Out: k [14], qz [14] (q with the clamped entries zeroed), K [14][28], mask [14] (1 = free), *iters.  Returns "bad".
extern "C" int emul_wave_gains(int box, int boxed, const double *H, const double *q, const double *lb, const double *ub,
                               const double *k0, const double *Qux, int maxiter, double th_acceptstep, double th_grad,
                               double reg, double *k, double *qz, double *K, double *mask, int *iters) {
  using W = aslr::WaveGainsLds<NU>;
  double w[W::SIZE], qv[NU];
  for (int i = 0; i < W::SIZE; ++i) w[i] = 0.0;
  for (int i = 0; i < NU; ++i) { qv[i] = q[i]; w[W::oLb + i] = lb[i]; w[W::oUb + i] = ub[i]; }
  const aslr::WaveQPParams P{maxiter, th_acceptstep, th_grad, reg, 10};
  const bool bad = box ? aslr::wave_gains<NU, NX, true>(H, qv, Qux, K, w, boxed != 0, k0, P, iters)
                       : aslr::wave_gains<NU, NX, false>(H, qv, Qux, K, w, false, k0, P, iters);
  for (int i = 0; i < NU; ++i) { k[i] = w[W::oKv + i]; qz[i] = qv[i]; mask[i] = w[W::oMk + i]; }
  return bad ? 1 : 0;
}
