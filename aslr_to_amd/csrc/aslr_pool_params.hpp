// aslr_pool_params.hpp -- what aslr_abi.hip (the driver) and aslr_pool_params.hip (the kernel) of aslr_solve_pool_params share.
// Not part of aslr_common.hpp: no other translation unit reads it.
#pragma once
#include "aslr_common.hpp"

namespace aslr {

// the pool's arrays by value, as pool_refill_kernel's PoolDev, plus the parameter table
struct PoolParamsDev {
  int32_t P, nx, nu, rows;      // rows = 2 nj + 2 nu (traj_params_rows_c)
  const double *x0, *frame_ref, *xs_init, *us_init;
  double *xs_out, *us_out, *stat_f;
  int32_t *stat_i, *slot_problem, *counters;
  const double *params;         // [rows][P]: aslr_pool_params_t::params_dev after the upload
  double *traj_params;          // region TRAJ_PARAMS of the handle, [rows][B]
};
// flush the stopped slots and hand them their next problems, parameters included: one block per slot, k.B blocks
int launch_pool_refill_params(const KArgs &k, const PoolParamsDev &pl, double reg0, int is_feasible, hipStream_t st);

} // namespace aslr
