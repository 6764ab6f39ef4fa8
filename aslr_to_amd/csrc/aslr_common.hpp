// aslr_common.hpp -- shared by the per-kernel translation units of libaslr_to_hip.so
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "aslr_device.hpp"

namespace aslr {

// The one way a call fails: writes the thread's error string (aslr_last_error; printf-style) and returns `code`.  Every
// non-OK return of the C ABI comes from here.  A refused argument or condition is reported under the name of the entry
// point that was called; a failed HIP call (HIP_TRY) under the name of the function it sits in, which may be an internal
// launcher, with the call, HIP's error string, file and line.
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
constexpr int kErrLen = 512;

#define HIP_TRY(expr)                                                                                                  \
  do {                                                                                                                 \
    hipError_t e_ = (expr);                                                                                            \
    if (e_ != hipSuccess)                                                                                              \
      return aslr::fail(ASLR_E_HIP, "%s: %s -> %s (%s:%d)", __func__, #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

constexpr int rec_len_c(int nx, int nu) { return (2 * nx * nx + 2 * nx * nu + nu * nu + nx + nu + 15) / 16 * 16; }

// kernel argument block: device pointers into the workspace
struct KArgs {
  const DevDesc *desc;
  const int32_t *node_model;
  const double *x0;
  const double *frame_ref; // nullable
  double *xs, *us, *xnext, *cost, *deriv, *gaps, *kgain, *kff, *qu, *vx, *vxx, *xs_try, *us_try, *vxxf, *cost_try, *dyn;
  double *traj_f;
  int32_t *traj_i;
  int32_t B, T;
  // trajectories [b0, b1) of the shard this launch covers (the whole shard unless the handle iterates sub-shards on
  // their own streams, aslr_set_subshards): array strides stay B, grids are sized for b1 - b0
  int32_t b0, b1;
  int32_t planar; // the chain qualifies for the planar dynamics path (DevDesc::planar.ok)
  int32_t planar_reach; // ... and the frame-placement costs for the closed-form residual (DevDesc::planar.reach_ok)
  double *iter_log;  // per-iteration log [log_cap][ASLR_LOG_COUNT][B] (aslr_set_iteration_log), or nullptr
  int32_t log_cap;
  // knots [seg_t0, seg_t1] of the horizon this launch covers (kernels that can work on a part of it: the rollout carries
  // its state over through the candidate it has stored; the trial costs are per knot; the calc / calcDiff sweeps take
  // knots [0, seg_t1], seg_t0 is not theirs): the whole horizon = [0, T]
  int32_t seg_t0, seg_t1;
  int32_t pipeline; // forward pass in two launches: the trial costs of the first half of the horizon run in the launch that rolls
                    // out the second half (rollout_and_cost_kernel; planar 2-joint chains).  0: off, 1 or 2: two segments (default), 3, 4: more (measured: no better)
  // frame_ref is a path [ref_last + 1][B][12]: knot t of trajectory b reads row min(ref_row0 + t, ref_last), at
  // frame_ref + 12 ((size_t)row B + b).  The create-time table is a path of one row (0, 0); aslr_set_reference_path puts the
  // caller's buffer here and aslr_mpc_run advances ref_row0 by one per control step, on the host.  The knot is block-uniform
  // wherever the address is formed (it comes from blockIdx), so the row offset is scalar arithmetic on kernel arguments, and
  // a wave's 64 trajectories read one contiguous stretch of the row.  The expression is written out at its three sites
  // (calc_kernel, quasi_static_kernel, trial_cost_body): behind a helper that takes the argument block by reference the
  // trial-cost kernels kept their control vector in scratch memory (32 - 128 bytes per lane where there was none)
  int32_t ref_row0, ref_last;
};

// -DASLR_EXP_STAMP (tools/stamp_gaps.py): every kernel of an iteration records when its first wave started and its last one
// ended (s_memrealtime, 100 MHz) in the unused head of VXX: per sub-shard (quarter of the shard) 1024 words,
// [iteration][kernel 0..7][first start, last end]; word 1023 counts the iterations (select_kernel, the last kernel, bumps it).
#ifdef ASLR_EXP_STAMP
// (start: the first block of the grid -- blocks are dispatched in order; end: an atomic max over the blocks of the sweeps, whose
//  waves all run at once, and the LAST block of the large streaming grids, where 16 000 atomics on one word would be the kernel)
#define ASLR_STAMP_BEGIN(a, kid)                                                                                       \
  unsigned long long *stamp_w_ = reinterpret_cast<unsigned long long *>((a).vxx) + (size_t)((a).b0 * 4 / (a).B) * 1024;  \
  const unsigned long long stamp_it_ = *reinterpret_cast<volatile unsigned long long *>(stamp_w_ + 1023);               \
  if (threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && stamp_it_ < 60)                     \
    stamp_w_[(stamp_it_ * 8 + (kid)) * 2] = (unsigned long long)wall_clock64()
#define ASLR_STAMP_END(kid, every_block)                                                                               \
  do {                                                                                                                 \
    if (threadIdx.x == 0 && stamp_it_ < 60) {                                                                          \
      if (every_block) atomicMax(stamp_w_ + (stamp_it_ * 8 + (kid)) * 2 + 1, (unsigned long long)wall_clock64());      \
      else if (blockIdx.x == gridDim.x - 1 && blockIdx.y == gridDim.y - 1 && blockIdx.z == gridDim.z - 1)              \
        stamp_w_[(stamp_it_ * 8 + (kid)) * 2 + 1] = (unsigned long long)wall_clock64();                                \
    }                                                                                                                  \
  } while (0)
#define ASLR_STAMP_NEXT() do { if (blockIdx.x == 0 && threadIdx.x == 0) stamp_w_[1023] = stamp_it_ + 1; } while (0)
#else
#define ASLR_STAMP_BEGIN(a, kid)
#define ASLR_STAMP_END(kid, every_block)
#define ASLR_STAMP_NEXT()
#endif

// Line-search candidates (XS_TRY / US_TRY, layout in include/aslr_to_amd.h): 16-byte piece p of trajectory b at knot t of
// step length ai; W = doubles per candidate, TK = knots stored (T + 1 or T)
template <int W>
ASLR_DEV size_t cand_piece(int ai, int t, int b, int p, int B, int TK) {
  const size_t slab = (size_t)ASLR_CAND_SLAB(B, W);
  const size_t in_slab = ASLR_CAND_INTERLEAVED(W) ? ((size_t)(b >> 2) * (W / 2) + p) * 8 + (size_t)(b & 3) * 2 : (size_t)b * W + 2 * p;
  return ((size_t)ai * TK + t) * slab + in_slab;
}

// node -> action-model index, read through the constant address space: the table is never written by a kernel, and a
// scalar load keeps it out of vmcnt (as a vector load its wait drained every prefetch issued just before it)
ASLR_DEV int node_model_at(const KArgs &a, int t) {
  return ((const int32_t __attribute__((address_space(4))) *)(a.node_model))[t];
}

// solver parameters by value
struct SolverDev {
  int32_t solver, fixed_iterations;
  double th_stop, th_grad, th_gaptol, th_stepdec, th_stepinc, th_acceptstep, th_acceptnegstep;
  double reg_min, reg_max, reg_incfactor, reg_decfactor;
  int32_t boxqp_maxiter;
  double boxqp_th_acceptstep, boxqp_th_grad, boxqp_reg;
  int32_t standalone; // 1: API-level single pass (no retry, no solver-state updates)
  int32_t store_v;    // 1: write VX / VXX
  int32_t maxiter_traj; // > 0: a trajectory stops by itself after this many iterations (pool solves); 0: the host loop bounds them
};

// control limits of the (at most ASLR_MAX_MODELS) action models, passed by value so the backward loop
// never chases model pointers
struct ModelLimits {
  int32_t has[ASLR_MAX_MODELS];
  double lb[ASLR_MAX_MODELS][ASLR_MAX_NU], ub[ASLR_MAX_MODELS][ASLR_MAX_NU];
};

__device__ __forceinline__ bool is_bad(double v) { return isnan(v) || isinf(v) || v >= 1e30; }
// Crocoddyl's raiseIfNaN(v.lpNorm<Infinity>()) on a short vector: `s1` is the 1-norm of the same entries, which the
// kernels accumulate anyway.  s1 < 1e30 proves every entry finite and below 1e30 (the common case: one compare);
// otherwise (NaN, Inf, or a 1-norm that crossed 1e30 while the inf-norm may not have) the entries decide one by one.
template <int N>
__device__ __forceinline__ bool inf_norm_bad(double s1, const double (&v)[N]) {
  if (__ballot(!(s1 < 1e30)) == 0ull) return false; // (wave-uniform: a real branch around the rare path)
  bool bad = false;
  _Pragma("unroll") for (int i = 0; i < N; ++i) bad = bad || is_bad(fabs(v[i]));
  return bad;
}

// calc_kernel mode bits
constexpr int kModeCommit = 1;    // copy the accepted candidate XS_TRY/US_TRY[acc] into XS/US
constexpr int kModeSolver = 2;    // honour RECALC/DONE flags and compute gaps
constexpr int kModeNoCompute = 4;
constexpr int kModeSkipConst = 8; // record chunks that depend on the model only are in place already: do not rewrite them

struct FrameArg { double R[9], p[3]; }; // local placement of a frame on its joint, by value

// ---- the launch layer ----
// What differs between the supported sizes (nj joints, DAM actuation: nx = 4 nj, nu = nj or 2 nj), as compile-time facts.
// Everything else about a launch is written once per kernel family, in the launcher at the end of its .inc.hpp.
template <int NJ, int DAM>
struct SizeTraits {
  static constexpr bool big_vsa = NJ == 7 && DAM == ASLR_DAM_VSA;
  // calcDiff: rigid-body part by 8-lane teams (dyn_team_kernel phases 0 and 1), then calc_kernel with PRE
  static constexpr bool team_dyn = NJ == 7 && DAM == ASLR_DAM_SEA;
  static constexpr bool skip_const = NJ == 2 || team_dyn; // a calcDiff variant without the model-only record chunks is built
  static constexpr bool team_rollout = NJ == 7;           // forward: one block of 8-lane teams per trajectory
  // (7, VSA): the solver kernels are built for SolverBoxDDP only (aslr_abi.hip, solver_unsupported): no FDDP rollout
  static constexpr bool boxddp_only = big_vsa;
  static constexpr int cost_tag = big_vsa ? 14 : NJ;      // instantiation tag of sum_cost_kernel / select_kernel
  static constexpr bool reg_column = !big_vsa;            // backward: the register-column kernel (ASLR_BWD_HS > 0) is built
  // adjoint / covariance / LQG / tangent / smoother sweeps: one wave per block, a team of 8 (nx = 8) or 32 (nx = 28) lanes per trajectory
  static constexpr int sweep_blocks(int B) { return NJ == 2 ? (B + 7) / 8 : (B + 1) / 2; }
};

// a run-time bool as a template argument: f(std::true_type) or f(std::false_type)
template <class F>
void with_bool(bool b, F &&f) {
  if (b) f(std::true_type{}); else f(std::false_type{});
}
// the PLANAR argument of a launch: planar kernels exist for nj = 2 only (picked when k.planar); nj = 7 always launches
// PLANAR = false, whatever k.planar says
template <int NJ, class F>
void with_planar(const KArgs &k, F &&f) {
  if constexpr (NJ == 2) with_bool(k.planar != 0, f); else f(std::false_type{});
}

// One launcher per kernel family, defined in the family's .inc.hpp and explicitly instantiated in the translation unit
// of the size.  frame_placement does not depend on the actuation: one instantiation per nj.
// TP: the per-trajectory parameter table (aslr_set_trajectory_params) replaces K, B^-1 and the control box in the kernel
// families that read them -- calc / calcDiff, quasi-static, rollout, backward; the TP = true launchers live in
// translation units of their own (aslr_*_tp.hip), so the default path's code objects are what they were.
template <int NJ, int DAM, bool TP = false> int launch_calc(const KArgs &k, bool diff, int mode, double th_gaptol, hipStream_t st);
template <int NJ, int DAM> int launch_dam_eval(const KArgs &k, int mi, int n, const double *x, const double *u, double *xout, double *cost,
                                               double *Fx, double *Fu, double *Lx, double *Lu, double *Lxx, double *Lxu, double *Luu, hipStream_t st);
template <int NJ, int DAM> int launch_dam_residuals(const KArgs &k, int mi, int n, const double *x, const double *u, double *r, int nr, hipStream_t st);
template <int NJ> int launch_frame_placement(const KArgs &k, int fj, const FrameArg &F, int n, const double *x, int64_t stride, double *out, hipStream_t st);
template <int NJ, int DAM, bool TP = false> int launch_quasi_static(const KArgs &k, int maxiter, double tol, int32_t *iters, hipStream_t st);
template <int NJ, int DAM, bool TP = false> int launch_forward(const KArgs &k, const SolverDev &sd, const ModelLimits &lim, hipStream_t st);
// hs: ASLR_BWD_HS (0: the size's default decomposition); mfma: ASLR_BLK_MFMA (block kernel of nx = 28 only)
template <int NJ, int DAM, bool TP = false> int launch_backward(const KArgs &k, int hs, bool mfma, const SolverDev &sd, const ModelLimits &lim, hipStream_t st);

// dt and the diagonals of K and 1 / B per action model, as the adjoint and the tangent sweep read them: the last member of
// both argument blocks (as a base struct it would come first and move every kernel-argument offset)
struct SweepPlant {
  double dt[ASLR_MAX_MODELS];
  double K[ASLR_MAX_MODELS][ASLR_MAX_NJ], Binv[ASLR_MAX_MODELS][ASLR_MAX_NJ]; // K = 0: no stiffness term (VSA)
};

// Adjoint sweep (aslr_cost_sensitivity, aslr_adjoint.inc.hpp): what adjoint_kernel reads and writes, by value.  One template
// serves handles with and without a parameter table (traj_params == nullptr: K and 1 / B of the node's model, `plant`),
// so the TP rows of the table of kernel sets share the launcher with the plain rows.
struct AdjointArgs {
  const double *deriv, *xs, *xnext;
  const int32_t *node_model;
  const double *traj_params; // region TRAJ_PARAMS while a table is set, else nullptr
  double *d_stiffness, *d_motor_inertia, *d_x0; // [nj][B], [nj][B], [nx][B]; each nullable
  double *costate;                              // [T+1][B][nx]; nullable
  int32_t B, T;
  SweepPlant plant;
};
template <int NJ, int DAM> int launch_adjoint(const AdjointArgs &a, hipStream_t st);

// Closed-loop covariance sweep (aslr_policy_covariance, aslr_covariance.inc.hpp): what covariance_kernel reads and writes, by
// value.  It reads no model constant: one launcher per size, shared by its two rows.
struct CovarianceArgs {
  const double *deriv, *kgain;
  const double *sigma0, *noise_var;                         // [B][nx][nx], [T][B][nx]; each nullable (zero)
  double *x_var, *u_var, *cov_final, *cov, *cost_increase; // [T+1][B][nx], [T][B][nu], [B][nx][nx], [T+1][B][nx][nx], [B]; each nullable
  int32_t B, T;
};
template <int NJ, int DAM> int launch_covariance(const CovarianceArgs &a, hipStream_t st);

// Output-feedback covariance sweep (aslr_policy_lqg, aslr_lqg.inc.hpp): what lqg_kernel reads and writes, by value.  Like the
// covariance sweep it reads no model constant: one launcher per size, shared by its two rows.
struct LqgArgs {
  const double *deriv, *kgain;
  const double *meas_var;           // [B][ny]
  const double *sigma0, *noise_var; // [B][nx][nx], [T][B][nx]; each nullable (zero)
  double *x_var, *u_var, *est_var;  // [T+1][B][nx], [T][B][nu], [T+1][B][nx]; every output nullable
  double *cov_final, *est_cov_final, *kalman_gain, *cost_increase; // [B][nx][nx], [B][nx][nx], [T+1][B][nx][ny], [B]
  int32_t B, T, ny;
  int32_t meas[ASLR_MAX_NX]; // the measured state entries: the first ny, distinct, each in [0, nx)
};
template <int NJ, int DAM> int launch_lqg(const LqgArgs &a, hipStream_t st);

// Tangent sweep (aslr_policy_plant_sensitivity, aslr_plant_sens.inc.hpp): what plant_sens_kernel reads and writes, by value.
// The parameters of a trajectory are taken as AdjointArgs has them, and the rows share the launcher in the same way.
struct PlantSensArgs {
  const double *deriv, *kgain, *xs, *xnext;
  const int32_t *node_model;
  const double *traj_params;                       // region TRAJ_PARAMS while a table is set, else nullptr
  const double *stiffness_var, *motor_inertia_var; // [nj][B]; each nullable (zero)
  double *dx_k, *dx_b;                             // [T+1][B][nx][nj]; every output nullable
  double *dxT_k, *dxT_b;                           // [B][nx][nj]
  double *dcost_k, *dcost_b;                       // [nj][B]
  double *x_var, *u_var;                           // [T+1][B][nx], [T][B][nu]
  int32_t B, T;
  int32_t stiff; // the stiffness columns are computed (some stiffness quantity is asked for; never on a VSA size)
  SweepPlant plant;
};
template <int NJ, int DAM> int launch_plant_sens(const PlantSensArgs &a, hipStream_t st);

// Closed-loop policy roll-outs (aslr_policy_rollout, aslr_policy.inc.hpp): the caller's arrays, by value, beside the KArgs and
// ModelLimits of the handle.  One template serves handles with and without a parameter table (`table`), as the adjoint
// kernel does, and the rows share its launcher likewise.
struct PolicyArgs {
  const double *plant_stiffness, *plant_motor_inertia; // [nj][S][B], each nullable
  const double *dx0, *disturbance;                     // [S][B][nx], [S][T][B][nx], each nullable
  double *cost;                                        // [S][B]; every output nullable
  int32_t *failed_knot;                                // [S][B]
  double *x_final, *xs_closed, *us_closed;             // [S][B][nx], [S][T+1][B][nx], [S][T][B][nu]
  int32_t S, clamp;
  int32_t table;    // a parameter table is set: K, 1 / B and the control box of a trajectory are its row
  int32_t diagonal; // a plant array or a table is in use (every model's K and B is diagonal then): diagonals through ModelRegs::set_traj
};

// The same roll-outs with the perturbations drawn inside the kernel (aslr_policy_rollout_noise, aslr_policy_noise.hpp): the
// input pointers of the PolicyArgs part are NULL, the sigma arrays stand in their place.  The same kernel templates, with this
// type as their argument type, in units of their own (aslr_policy_noise_nj2.hip, aslr_policy_noise_team.hip).
struct NoiseKey { uint32_t k0, k1, sample0, trajectory0; }; // the Philox key (seed, low and high word) and the counter offsets
struct PolicyNoiseArgs : PolicyArgs {
  const double *noise_std, *dx0_std;                       // [B][nx], each nullable (that source is absent)
  const double *stiffness_rel_std, *motor_inertia_rel_std; // [B][nj], each nullable
  double *drawn_stiffness, *drawn_motor_inertia;           // [nj][S][B]; every output nullable
  double *drawn_dx0, *drawn_disturbance;                   // [S][B][nx], [S][T][B][nx]
  NoiseKey key;
  double knom[ASLR_MAX_NJ], bnom[ASLR_MAX_NJ]; // the diagonals of K and B the models share: the nominal while no table is set
};
// PA: PolicyArgs or PolicyNoiseArgs, two entries of a row.  Two names for two bodies in two headers: a sample per lane (nx = 8,
// aslr_policy.inc.hpp) and 8-lane teams (nx = 28, aslr_policy_team.inc.hpp); a row takes the one SizeTraits::team_rollout names
template <int NJ, int DAM, class PA> int launch_policy_rollout(const KArgs &k, const ModelLimits &lim, const PA &pa, hipStream_t st);
template <int NJ, int DAM, class PA> int launch_policy_rollout_team(const KArgs &k, const ModelLimits &lim, const PA &pa, hipStream_t st);

// The plant phase of one control step of aslr_mpc_run_plant (aslr_mpc_plant.inc.hpp): the caller's arrays, by value, beside
// the KArgs and ModelLimits of the handle; `table` and `diagonal` as in PolicyArgs.
struct MpcPlantArgs {
  const double *plant_stiffness, *plant_motor_inertia; // [nj][B], each nullable
  const double *disturbance;                           // [hold][B][nx] of this step, nullable
  double *x_rec, *u_rec;                               // x_closed[s hold] ([hold + 1] rows are written), u_closed[s hold]
  double *closed_cost;                                 // [B], nullable: started in the first step, continued after
  int32_t *failed_knot;                                // [B], nullable: likewise
  int32_t hold, k0;                                    // knots applied per step; the applied-knot index of this step's first
  int32_t first, clamp;                                // first: step 0 of the run
  int32_t table, diagonal;
};
// per-lane (nx = 8, aslr_mpc_plant.inc.hpp) and team (nx = 28, aslr_mpc_plant_team.inc.hpp) forms, as the roll-out's
template <int NJ, int DAM> int launch_mpc_plant(const KArgs &k, const ModelLimits &lim, const MpcPlantArgs &pa, hipStream_t st);
template <int NJ, int DAM> int launch_mpc_plant_team(const KArgs &k, const ModelLimits &lim, const MpcPlantArgs &pa, hipStream_t st);

// One outer step of aslr_design_descent (aslr_design.hip): what design_step_kernel reads and writes, by value.  The workspace
// pointers are the handle's; everything else is the caller's (include/aslr_to_amd_design.h).  Like the adjoint kernel it
// depends on no model size at compile time: one launcher, no entry in the table of kernel sets.
struct DesignStepArgs {
  double *xs, *us, *gaps, *vxxf, *kff;     // XS / US are copied to or from the best plan; the others are zeroed
  const double *traj_f;                    // TF_COST: the cost of the finalized candidate
  double *traj_params;                     // region TRAJ_PARAMS: column b takes the next candidate
  const double *lo, *hi, *grad;            // [2 nj][B]: bounds, the gradient at the candidate
  double *theta, *cost_best;               // [2 nj][B], [B]: the accepted design and its cost
  double *xs_best, *us_best;               // [T+1][B][nx], [T][B][nu]
  double *g_acc, *eta;                     // [2 nj][B], [B]; eta < 0 marks a frozen trajectory
  double *hist_f;                          // [3][B] of this step, nullable
  int32_t *hist_i;                         // [B] of this step, nullable
  double *theta_hist;                      // [2 nj][B] of this step, nullable
  int32_t B, T, nx, nu, nj;
  int32_t s, last;                         // the step index; last: the table takes the accepted design, not a candidate
  int32_t opt_k, opt_b;
  double eta0, grow, shrink, c1, max_rel;
};
int launch_design_step(const DesignStepArgs &a, hipStream_t st);

// aslr_plant_identify (aslr_identify.inc.hpp; include/aslr_to_amd_identify.h): what identify_normal_kernel reads and writes, by
// value.  It reads no K and no B (the columns of Jz are the parameter derivatives times the parameter): dt alone, per model.
struct IdentifyNormalArgs {
  const double *deriv, *xs, *xnext;
  const int32_t *node_model;
  const double *weights;            // [nx][B], nullable (ones)
  double *sse, *grad, *information; // [B], [np][B], [np (np+1)/2][B] of the candidate
  int32_t B, T;
  int32_t stiff;  // the stiffness columns are computed (never on a VSA size)
  int32_t np_out; // entries stored: all np of the kernel, or nj where the stiffness alone is fitted (the K block)
  double dt[ASLR_MAX_MODELS];
};
template <int NJ, int DAM> int launch_identify_normal(const IdentifyNormalArgs &a, hipStream_t st);

// ... and identify_step_kernel: the decision on the candidate, the accepted set, the damped solve, the next candidate into
// the trajectory's column of TRAJ_PARAMS.  Everything but the table is the caller's.
struct IdentifyStepArgs {
  double *traj_params;                              // region TRAJ_PARAMS
  const double *lo, *hi;                            // [np][B]
  double *theta_try;                                // [np][B]: the candidate evaluated; takes the next one
  const double *sse_try, *g_try, *h_try;            // [B], [np][B], [nh][B]: what the normal kernel made of it
  double *theta, *sse, *grad, *information, *mu;    // the accepted set and the damping (mu < 0: frozen)
  int32_t *identifiable, *n_accepted;               // [np][B], [B]
  double *hist_theta, *hist_sse;                    // [np][B], [B] of this step, nullable
  int32_t *hist_decision;                           // [B] of this step, nullable
  int32_t B, nj, np;
  int32_t row0;                                     // table row of parameter 0: 0 (stiffness fitted) or nj (motor inertia alone)
  int32_t s, last;
  double mu0, mu_min, mu_max, grow, shrink, max_rel, min_curv;
};
template <int NJ, int DAM> int launch_identify_step(const IdentifyStepArgs &a, hipStream_t st);

// aslr_state_smooth (aslr_smooth.inc.hpp; include/aslr_to_amd_smooth.h): what smooth_filter_kernel and smooth_adjoint_kernel
// read and write in one iteration, by value.  Like the LQG sweep they read no model constant: one pair of launchers per size,
// shared by its two rows.  The caller's scratch `work` holds, time-major with N = (T+1) B knots of trajectories:
//   Pm [N][nx][nx] (word [c][j]: lane j's entry c) | L^T [N][ny][nx] | m^- [N][nx] | w [N][ny]
struct SmoothArgs {
  const double *deriv, *xnext;
  double *xs;                                  // XS of the handle: the nominal (both kernels read it), then the relaxed estimate
  const double *ys, *meas_var, *x0_mean;       // [T+1][B][ny], [B][ny], [B][nx]
  const double *sigma0, *noise_var;            // [B][nx][nx], [T][B][nx]; each nullable (zero)
  double *work;
  double *xs_smooth, *x_filt, *est_var, *nis;  // [T+1][B][nx] x 3, [T+1][B]; every output nullable (set in the last iteration)
  double *neg_log_lik, *step_norm;             // [B] of this iteration, each nullable
  double relax;
  int32_t B, T, ny;
  int32_t meas[ASLR_MAX_NX]; // the measured state entries: the first ny, distinct, each in [0, nx)
  int32_t slot[ASLR_MAX_NX]; // slot[i]: where state entry i stands in meas, or -1 (not measured)
};
template <int NJ, int DAM> int launch_smooth_filter(const SmoothArgs &a, hipStream_t st);
template <int NJ, int DAM> int launch_smooth_adjoint(const SmoothArgs &a, hipStream_t st);

// the launchers of one supported size: a row of the table in aslr_abi.hip, looked up once by aslr_problem_create
struct KernelSet {
  int nj, dam;
  bool traj_params; // the row of the handles that have a per-trajectory parameter table set
  bool boxddp_only;
  decltype(&launch_calc<2, 0>) calc;
  decltype(&launch_dam_eval<2, 0>) dam_eval;
  decltype(&launch_dam_residuals<2, 0>) dam_residuals;
  decltype(&launch_frame_placement<2>) frame_placement;
  decltype(&launch_quasi_static<2, 0>) quasi_static;
  decltype(&launch_forward<2, 0>) forward;
  decltype(&launch_backward<2, 0>) backward;
  decltype(&launch_adjoint<2, 0>) adjoint; // the extension calls: the TP rows share these with the plain rows
  decltype(&launch_covariance<2, 0>) covariance;
  decltype(&launch_lqg<2, 0>) lqg;
  decltype(&launch_plant_sens<2, 0>) plant_sens;
  decltype(&launch_policy_rollout<2, 0, PolicyArgs>) policy_rollout;
  decltype(&launch_policy_rollout<2, 0, PolicyNoiseArgs>) policy_rollout_noise;
  decltype(&launch_mpc_plant<2, 0>) mpc_plant;
  decltype(&launch_identify_normal<2, 0>) identify_normal;
  decltype(&launch_identify_step<2, 0>) identify_step;
  decltype(&launch_smooth_filter<2, 0>) smooth_filter;
  decltype(&launch_smooth_adjoint<2, 0>) smooth_adjoint;
};

#ifdef ASLR_BWD_PROFILE
// profile builds only: read / reset the region table of THIS translation unit (static like the table itself; each unit
// exports it under its own name: aslr_debug_bwd_prof, _bwd_prof28, _calc_prof, _fwd_prof7, tools/*_regions*.py)
static int prof_table(unsigned long long *out32, int reset) {
  if (out32 && hipMemcpyFromSymbol(out32, HIP_SYMBOL(aslr_bwd_prof_dev), 32 * sizeof(unsigned long long)) != hipSuccess) return -1;
  if (reset) {
    unsigned long long z[32] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(aslr_bwd_prof_dev), z, sizeof(z)) != hipSuccess) return -1;
  }
  return 0;
}
#endif

} // namespace aslr
