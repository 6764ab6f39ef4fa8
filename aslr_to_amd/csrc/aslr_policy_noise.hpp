// aslr_policy_noise.hpp -- the counter-based generator behind aslr_policy_rollout_noise (include/aslr_to_amd_policy_noise.h,
// DESIGN.md 4.19): Philox4x32-10, two 53-bit uniforms per block, one Box-Muller pair per block.  A draw is a function of
// (seed, knot, sample, trajectory, kind, entry) alone -- no state, no LDS, no synchronisation: 32-bit integer VALU work
// (v_mul_hi_u32 / v_mul_lo_u32) and the device library's log, sqrt and sincospi in double.
#pragma once
#include "aslr_common.hpp"

namespace aslr {

enum : unsigned { kNoiseDisturbance = 0, kNoiseDx0 = 1, kNoiseStiffness = 2, kNoiseMotorInertia = 3 };

struct Philox4 { unsigned w0, w1, w2, w3; };

// ten rounds of (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), the key bumped after each
ASLR_DEV Philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
  constexpr unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
  ASLR_UNROLL for (int r = 0; r < 10; ++r) {
    const unsigned h0 = __umulhi(M0, c0), l0 = M0 * c0, h1 = __umulhi(M1, c2), l1 = M1 * c2;
    c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    k0 += W0; k1 += W1;
  }
  return Philox4{c0, c1, c2, c3};
}

// ((hi >> 5) 2^26 + (lo >> 6) + 1) 2^-53: every step exact in double, the result in (0, 1]
ASLR_DEV double noise_uniform(unsigned hi, unsigned lo) {
  return ((double)(hi >> 5) * 67108864.0 + (double)(lo >> 6) + 1.0) * 0x1p-53;
}

// A drawn value enters the roll-out the way a value read from the caller's array does: as a finished double.  The empty
// statement pins it to a register, so that the multiply that formed it cannot be contracted into the add that consumes it
// (x + sigma z as one fma would not be the bits aslr_policy_rollout gives on the stored array).
ASLR_DEV double noise_settled(double v) {
  asm volatile("" : "+v"(v));
  return v;
}

// (NoiseKey, aslr_common.hpp: the key and the offsets of sample and trajectory, what identifies the draws of one launch)
// the normals of entries 2 p and 2 p + 1 of source `kind` at knot t of (sample s, trajectory b): z_a = r cos(2 pi u_b),
// z_b = r sin(2 pi u_b), r = sqrt(-2 log u_a)
ASLR_DEV void noise_pair(const NoiseKey &nk, unsigned kind, unsigned t, unsigned s, unsigned b, unsigned p, double &za, double &zb) {
  const Philox4 w = philox4x32_10(t, nk.sample0 + s, nk.trajectory0 + b, (kind << 16) | p, nk.k0, nk.k1);
  const double r = sqrt(-2.0 * log(noise_uniform(w.w0, w.w1)));
  double sn, cs;
  sincospi(2.0 * noise_uniform(w.w2, w.w3), &sn, &cs);
  za = r * cs; zb = r * sn;
}

// the normal of entry e alone (the other half of its pair is thrown away)
ASLR_DEV double noise_entry(const NoiseKey &nk, unsigned kind, unsigned t, unsigned s, unsigned b, unsigned e) {
  double za, zb;
  noise_pair(nk, kind, t, s, b, e >> 1, za, zb);
  return (e & 1u) ? zb : za;
}

} // namespace aslr
