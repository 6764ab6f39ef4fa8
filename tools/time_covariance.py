"""Times of the closed-loop covariance sweep (aslr_policy_covariance) beside the calcDiff sweep and the backward sweep of the
same handle, with HIP events on the launch stream: tools/time_covariance.py [repeats]

Shapes: two_dof_vsa_boxddp (B = 4096, T = 100, nx = 8, nu = 4), talos_arm_sea and talos_arm_vsa (B = 512, T = 150, nx = 28,
nu = 7 and 14).  Per shape, the median over `repeats` (default 20) of
  calc_diff         aslr_calc_diff alone;
  covariance        aslr_policy_covariance with sigma0 and noise_var and every output but cov (what the Python facade asks
                    for): the calcDiff sweep and covariance_kernel, back to back on one stream;
  states only       the same with x_var and cov_final alone: the kernel without its control terms;
  sweep             covariance - calc_diff (and states only - calc_diff): the C ABI has no entry point that launches
                    covariance_kernel alone;
  backward          aslr_backward_pass of the same handle on the same records (existing code, for comparison).
The candidate and the gains are what five solver iterations from a cold start leave."""
import sys

import torch

from _timing import STANDARD_SHAPES, planned, ptr, seeded_spread, timed


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    for name, make in STANDARD_SHAPES.items():
        e, sp = planned(make, 5)
        s0, w, _ = seeded_spread(e)
        new = lambda *s: torch.zeros(s, dtype=torch.float64, device=e.device)
        xv, uv, cf, ci = new(e.T + 1, e.B, e.nx), new(e.T, e.B, e.nu), new(e.B, e.nx, e.nx), new(e.B)
        cov = lambda: e._call("aslr_policy_covariance", ptr(s0), ptr(w), ptr(xv), ptr(uv), ptr(cf), None, ptr(ci), e._stream())
        states = lambda: e._call("aslr_policy_covariance", ptr(s0), ptr(w), ptr(xv), None, ptr(cf), None, None, e._stream())
        for fn in (e.calc_diff, cov, states, lambda: e.backward_pass(sp)):  # warm-up: code objects loaded, records in place
            fn()
        torch.cuda.synchronize()
        t_calc = timed(e.calc_diff, repeats)
        t_cov = timed(cov, repeats)
        t_states = timed(states, repeats)
        t_bwd = timed(lambda: e.backward_pass(sp), repeats)
        assert bool(torch.isfinite(xv).all()) and bool(torch.isfinite(ci).all())
        print("%s B=%d T=%d nx=%d nu=%d: calc_diff %.3f ms, covariance %.3f ms (sweep %.3f ms), states only %.3f ms (sweep %.3f ms), "
              "backward %.3f ms" % (name, e.B, e.T, e.nx, e.nu, t_calc, t_cov, t_cov - t_calc, t_states, t_states - t_calc, t_bwd))
        e.close()


if __name__ == "__main__":
    main()
