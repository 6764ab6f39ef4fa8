/*
 * aslr_to_amd_policy_noise.h -- extension of the C ABI (aslr_to_amd.h): Monte-Carlo roll-outs of the stored policy whose
 * perturbations are drawn on the device, for every model size.
 *
 * A header of its own, exported from the same libaslr_to_hip.so, for the reason aslr_to_amd_sens.h gives: the set of
 * functions aslr_to_amd.h declares, the structs aslr_sizeof knows and ASLR_ABI_VERSION are what existing bindings check
 * against, and this entry point changes none of them (plain pointers and integers, no new struct).  aslr_policy_rollout and
 * aslr_policy_rollout_all keep their behaviour; a binding that wants this call declares it next to the base set
 * (INTEGRATION.md 5a); one that does not is unaffected.  Conventions and the error contract are those of aslr_to_amd.h.
 *
 * aslr_policy_rollout takes every perturbation as an array: the disturbance alone is 8 S T B nx bytes, which the host has to
 * draw, upload and keep in device memory.  Here the kernel draws them from a counter-based generator, so the number of
 * samples is bounded by time alone, a run is reproducible from one integer, a shard of a multi-GPU batch draws what the
 * single-GPU batch would (trajectory0), and any one sample can be replayed alone (sample0) with its trajectory kept.
 *
 * THE GENERATOR (one definition: this header, DESIGN.md 4.19, tests/_policy_noise.py)
 *
 * Block function: Philox4x32-10.  Multipliers M0 = 0xD2511F53, M1 = 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85; ten
 * rounds.  A round computes, with the 64-bit products p0 = M0 c0 and p1 = M1 c2,
 *     (c0, c1, c2, c3) <- (hi(p1) ^ c1 ^ k0,  lo(p1),  hi(p0) ^ c3 ^ k1,  lo(p0))
 * and then adds the increments to (k0, k1).  Known answers (counter / key -> output):
 *     00000000 00000000 00000000 00000000 / 00000000 00000000 -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8
 *     ffffffff ffffffff ffffffff ffffffff / ffffffff ffffffff -> 408f276d 41c83b0e a20bc7c6 6d5451fd
 *     243f6a88 85a308d3 13198a2e 03707344 / a4093822 299f31d0 -> d16cfe09 94fdcceb 5001e420 24126ea1
 * Key and counter:  k = (seed & 0xffffffff, seed >> 32);  c = (t, sample0 + s, trajectory0 + b, kind << 16 | pair), 32-bit
 * words, with kind = 0 disturbance, 1 dx0, 2 stiffness, 3 motor inertia, and t = 0 for kinds 1 to 3.
 * Uniforms: the output words w0..w3 give  u_a = ((w0 >> 5) 2^26 + (w1 >> 6) + 1) 2^-53  and u_b likewise from w2, w3: exact
 * in double, in (0, 1].  Normals: with r = sqrt(-2 log u_a), pair p holds those of entries 2 p and 2 p + 1,
 *     z_{2p} = r cos(2 pi u_b),   z_{2p+1} = r sin(2 pi u_b)        (|z| <= 8.58),
 * in double with the device library's log, sqrt and sincospi(2 u_b).  An odd count (nj = 7) discards the last sine.
 * Draws (sigma arrays are per trajectory):
 *     disturbance[s][t][b][i] = noise_std[b][i] z(0; t, s, b, i)
 *     dx0[s][b][i]            = dx0_std[b][i] z(1; s, b, i)
 *     K_j = Knom_j(b) exp(stiffness_rel_std[b][j] z(2; s, b, j)),    B_j = Bnom_j(b) exp(motor_inertia_rel_std[b][j] z(3; s, b, j))
 * Knom and Bnom are the trajectory's own values: its row of the parameter table if one is set, else the model's diagonal.
 * (The table stores 1 / B, formed on the host: with a table Bnom is the reciprocal of the stored row, within one rounding of
 * the value given to aslr_set_trajectory_params.)
 */
#ifndef ASLR_TO_AMD_POLICY_NOISE_H
#define ASLR_TO_AMD_POLICY_NOISE_H

#include "aslr_to_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The roll-out, the five outputs cost .. us_closed and their layouts are those of aslr_policy_rollout
 * (aslr_to_amd_policy.h), with the perturbations of sample s of trajectory b drawn as above instead of read.  A NULL sigma
 * pointer switches that source off exactly as a NULL input does there: no `+ 0.0`, and the knot's own model.
 *
 * All pointers are DEVICE pointers, 16-byte aligned.  Inputs, at least one given; their values are device data and are not
 * checked:
 *   noise_std              [B][nx]     dx0_std                [B][nx]
 *   stiffness_rel_std      [B][nj]     (SEA only: a VSA model takes its stiffness from u)
 *   motor_inertia_rel_std  [B][nj]
 * Outputs, each optional (NULL: nothing written), at least one of the first five given:
 *   cost [S][B],  failed_knot [S][B] (int32),  x_final [S][B][nx],  xs_closed [S][T+1][B][nx],  us_closed [S][T][B][nu];
 *   drawn_stiffness, drawn_motor_inertia [nj][S][B],  drawn_dx0 [S][B][nx],  drawn_disturbance [S][T][B][nx]: what was
 *   drawn, in exactly the layouts aslr_policy_rollout takes as inputs -- passed back to that call (or to
 *   aslr_policy_rollout_all) they give this call's outputs.  The drawn_* buffer of a source whose sigma is NULL is not written.
 *
 * Sizes: every handle aslr_policy_rollout_all accepts (2 joints; 7 joints, SEA and VSA).  Nothing in the workspace is
 * written; covers the whole shard on the caller's stream; enqueues only.
 * ASLR_E_INVALID (aslr_last_error starts with "aslr_policy_rollout_noise:"; nothing is written): what
 * aslr_policy_rollout_all refuses of handle, n_samples and outputs; all four sigma pointers NULL; sample0 < 0, trajectory0 < 0
 * or sample0 + n_samples overflowing; stiffness_rel_std on a VSA model; a plant sigma while K or B of a model is not
 * diagonal; a plant sigma with no parameter table while the models of the problem differ in that diagonal (there is then no
 * single nominal). */
int aslr_policy_rollout_noise(aslr_problem_t *p, int n_samples, int sample0, int trajectory0, uint64_t seed,
                              const double *noise_std,
                              const double *dx0_std,
                              const double *stiffness_rel_std,
                              const double *motor_inertia_rel_std,
                              int clamp,
                              double *cost,
                              int32_t *failed_knot,
                              double *x_final,
                              double *xs_closed,
                              double *us_closed,
                              double *drawn_stiffness,
                              double *drawn_motor_inertia,
                              double *drawn_dx0,
                              double *drawn_disturbance,
                              void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ASLR_TO_AMD_POLICY_NOISE_H */
