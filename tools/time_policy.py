"""Times of the closed-loop policy roll-out (aslr_policy_rollout) beside the forward pass of the same handle, with HIP events
on the launch stream: tools/time_policy.py [repeats]

Shape: two_dof_vsa_boxddp, B = 4096, T = 100 (nx = 8, nu = 4).  The policy is what five solver iterations from a cold start
leave.  Median over `repeats` (default 20) of
  forward           aslr_forward_pass: rollout_kernel + trial_cost_kernel + sum_cost_kernel (+ select_kernel), ten step
                    lengths per trajectory: B / 4 rollout waves (existing code, for comparison; it runs the same on the
                    parent commit);
  policy S          aslr_policy_rollout with costs only (cost, failed_knot, x_final), S = 16, 64, 256 samples per trajectory,
                    all four inputs given (plant inertia within +-30 %, |dx0| <= 1e-2, |w| <= 1e-3), clamp on:
                    (B / 4) * (S / 16) waves; per wave = time * CUs * 4 SIMDs / waves when the waves outnumber the SIMDs,
                    else the time itself;
  policy S kept     the same with xs_closed and us_closed written."""
import sys

import torch

from _timing import STANDARD_SHAPES, planned, ptr, timed


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    e, sp = planned(STANDARD_SHAPES["two_dof_vsa_boxddp"], 5)
    B, T = e.B, e.T
    simds = torch.cuda.get_device_properties(e.device).multi_processor_count * 4
    fwd = lambda: e.forward_pass(sp)
    fwd()
    torch.cuda.synchronize()
    t_fwd = timed(fwd, repeats)
    print("forward pass (rollout + trial costs + sums + line search, 10 step lengths): %.3f ms, %d rollout waves on %d SIMDs"
          % (t_fwd, B // 4, simds))
    gen = torch.Generator(device=e.device).manual_seed(1)
    rnd = lambda lo, hi, *shape: lo + (hi - lo) * torch.rand(shape, dtype=torch.float64, device=e.device, generator=gen)
    for S in (16, 64, 256):
        pb = 1e-3 * rnd(0.7, 1.3, 2, S, B)
        dx0, w = rnd(-1e-2, 1e-2, S, B, 8), rnd(-1e-3, 1e-3, S, T, B, 8)
        cost = torch.zeros((S, B), dtype=torch.float64, device=e.device)
        failed = torch.zeros((S, B), dtype=torch.int32, device=e.device)
        xf = torch.zeros((S, B, 8), dtype=torch.float64, device=e.device)
        for kept in (False, True):
            xs = torch.zeros((S, T + 1, B, 8), dtype=torch.float64, device=e.device) if kept else None
            us = torch.zeros((S, T, B, 4), dtype=torch.float64, device=e.device) if kept else None
            call = lambda: e._call("aslr_policy_rollout", S, None, ptr(pb), ptr(dx0), ptr(w), 1, ptr(cost), ptr(failed), ptr(xf),
                                   ptr(xs), ptr(us), e._stream())
            call()
            torch.cuda.synchronize()
            ms = timed(call, repeats)
            waves = (B // 4) * (S // 16)
            per_wave = ms * min(1.0, simds / waves)
            print("policy S=%3d%s: %.3f ms, %d waves, %.3f ms per wave, %.2f ns per (sample, trajectory); failed samples %d"
                  % (S, " kept" if kept else "     ", ms, waves, per_wave, 1e6 * ms / (S * B), int((failed >= 0).sum().item())))
            del xs, us
    e.close()


if __name__ == "__main__":
    main()
