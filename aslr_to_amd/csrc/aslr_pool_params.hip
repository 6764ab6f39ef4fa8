// aslr_pool_params.hip -- the refill of aslr_solve_pool_params: a pool whose problems carry their own K, 1 / B and control box
#include "aslr_pool_params.hpp"

namespace aslr {

// What pool_refill_kernel (aslr_abi.hip) does for a slot -- flush a stopped problem to the outputs, hand the slot the next
// problem of the pool -- and, in the refill branch, column jn of the pool's parameter table into column b of TRAJ_PARAMS, so
// that the TP kernels iterate the slot with its problem's parameters.  One 64-thread block per slot; nothing to do for a slot
// that is still iterating.  A kernel of its own, its stores written out once more: pool_refill_kernel stays the code
// aslr_solve_pool's bit-level tests pin (the comment above init_state_kernel says why not even a device function is shared).
// Plain vector stores throughout; the order is the old kernel's: the flush reads the slot's columns, a barrier, then the
// refill overwrites them.  (TRAJ_PARAMS is not read by the flush: its column could be written at any point after `skip`.)
__global__ void __launch_bounds__(64) pool_refill_params_kernel(KArgs a, PoolParamsDev pl, double reg0, int is_feasible) {
  const int b = blockIdx.x, tid = threadIdx.x, B = a.B, T = a.T, nx = pl.nx, nu = pl.nu;
  int32_t *TI = a.traj_i;
  double *TF = a.traj_f;
  __shared__ int next_j, skip;
  const int j = pl.slot_problem[b];
  if (tid == 0) { // one thread decides for the block (other blocks bump the counter during this launch)
    const int done = TI[ASLR_TI_DONE * B + b];
    skip = j >= 0 && !done; // still iterating
    if (j < 0 && __atomic_load_n(&pl.counters[0], __ATOMIC_RELAXED) >= pl.P) {
      // idle and nothing left to hand out: the slot must still be MARKED idle (pool_refill_kernel says why)
      TI[ASLR_TI_DONE * B + b] = 1;
      TI[ASLR_TI_ACCEPTED * B + b] = -1;
      skip = 1;
    }
  }
  __syncthreads();
  if (skip) return;
  if (j >= 0) { // ---- flush: the last accepted candidate is the solution (solver.xs / solver.us) ----
    const int acc = TI[ASLR_TI_ACCEPTED * B + b];
    double *xo = pl.xs_out + (size_t)j * (T + 1) * nx, *uo = pl.us_out + (size_t)j * T * nu;
    for (int t = tid; t <= T; t += 64) {
      for (int i = 0; i < nx; ++i) {
        const size_t src = acc >= 0 ? ((size_t)acc * (T + 1) + t) * ASLR_CAND_SLAB(B, nx) + ASLR_CAND_OFFSET(b, i, nx) : 0;
        xo[(size_t)t * nx + i] = acc >= 0 ? a.xs_try[src] : a.xs[((size_t)t * B + b) * nx + i];
      }
      if (t < T)
        for (int i = 0; i < nu; ++i) {
          const size_t src = acc >= 0 ? ((size_t)acc * T + t) * ASLR_CAND_SLAB(B, nu) + ASLR_CAND_OFFSET(b, i, nu) : 0;
          uo[(size_t)t * nu + i] = acc >= 0 ? a.us_try[src] : a.us[((size_t)t * B + b) * nu + i];
        }
    }
    if (tid == 0) {
      pl.stat_f[4 * (size_t)j + 0] = TF[ASLR_TF_COST * B + b];
      pl.stat_f[4 * (size_t)j + 1] = TF[ASLR_TF_STOP * B + b];
      pl.stat_f[4 * (size_t)j + 2] = TF[ASLR_TF_XREG * B + b];
      pl.stat_f[4 * (size_t)j + 3] = TF[ASLR_TF_STEP * B + b];
      pl.stat_i[2 * (size_t)j + 0] = TI[ASLR_TI_ITER * B + b];
      pl.stat_i[2 * (size_t)j + 1] = TI[ASLR_TI_STATUS * B + b];
      atomicAdd(&pl.counters[1], 1);
    }
  }
  __syncthreads(); // (the flush reads this slot's columns; the refill below overwrites them)
  if (tid == 0) {
    const int n = atomicAdd(&pl.counters[0], 1);
    next_j = n < pl.P ? n : -1;
  }
  __syncthreads();
  const int jn = next_j;
  if (jn < 0) { // pool exhausted: the slot idles (DONE stays set)
    if (tid == 0) { pl.slot_problem[b] = -1; TI[ASLR_TI_DONE * B + b] = 1; TI[ASLR_TI_ACCEPTED * B + b] = -1; }
    return;
  }
  // ---- refill: problem jn starts in slot b from its initial guess (zeros: solve([], [], maxiter)) ----
  for (int t = tid; t <= T; t += 64) {
    const size_t tb = (size_t)t * B + b;
    for (int i = 0; i < nx; ++i) {
      a.xs[tb * nx + i] = pl.xs_init ? pl.xs_init[((size_t)jn * (T + 1) + t) * nx + i] : 0.0;
      a.gaps[tb * nx + i] = 0.0; a.vxxf[tb * nx + i] = 0.0;
    }
    if (t < T)
      for (int i = 0; i < nu; ++i) {
        a.us[tb * nu + i] = pl.us_init ? pl.us_init[((size_t)jn * T + t) * nu + i] : 0.0;
        a.kff[tb * nu + i] = 0.0;
      }
  }
  if (tid < nx) const_cast<double *>(a.x0)[(size_t)b * nx + tid] = pl.x0[(size_t)jn * nx + tid];
  if (tid < 12 && pl.frame_ref && a.frame_ref) const_cast<double *>(a.frame_ref)[12 * (size_t)b + tid] = pl.frame_ref[12 * (size_t)jn + tid];
  // the problem's parameters: row r of the pool's table [rows][P] at column jn -> row r of TRAJ_PARAMS [rows][B] at column b
  for (int r = tid; r < pl.rows; r += 64) pl.traj_params[(size_t)r * B + b] = pl.params[(size_t)r * pl.P + jn];
  if (tid == 0) { // per-trajectory solver state, as init_state_kernel sets it
    for (int r = 0; r < ASLR_TF_COUNT; ++r) TF[r * B + b] = 0.0;
    for (int r = 0; r < ASLR_TI_COUNT; ++r) TI[r * B + b] = 0;
    TF[ASLR_TF_XREG * B + b] = reg0;
    TI[ASLR_TI_FEASIBLE * B + b] = is_feasible;
    TI[ASLR_TI_RECALC * B + b] = 1;
    TI[ASLR_TI_ACCEPTED * B + b] = -1;
    pl.slot_problem[b] = jn;
  }
}

int launch_pool_refill_params(const KArgs &k, const PoolParamsDev &pl, double reg0, int is_feasible, hipStream_t st) {
  hipLaunchKernelGGL(pool_refill_params_kernel, dim3(k.B), dim3(64), 0, st, k, pl, reg0, is_feasible);
  HIP_TRY(hipGetLastError());
  return ASLR_OK;
}

} // namespace aslr
