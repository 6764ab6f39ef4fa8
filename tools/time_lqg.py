"""Times of the output-feedback covariance sweep (aslr_policy_lqg) beside the calcDiff sweep and the closed-loop covariance
sweep (aslr_policy_covariance) of the same handle, in the same run, with HIP events on the launch stream:
tools/time_lqg.py [repeats]

Shapes: two_dof_vsa_boxddp (B = 4096, T = 100, nx = 8, nu = 4), talos_arm_sea and talos_arm_vsa (B = 512, T = 150, nx = 28,
nu = 7 and 14).  Per shape, the median over `repeats` (default 20) of
  calc_diff         aslr_calc_diff alone;
  covariance        aslr_policy_covariance as tools/time_covariance.py times it (existing code, for comparison);
  lqg               aslr_policy_lqg with the positions measured (ny = nx / 2), sigma0 and noise_var and every output but
                    kalman_gain (what the Python facade asks for): the calcDiff sweep and lqg_kernel, back to back on one stream;
  lqg all           the same with every state entry measured (ny = nx): the largest factorisation;
  filter only       est_var and kalman_gain alone, ny = nx / 2: the kernel without the estimate's half;
  sweep             each of them - calc_diff: the C ABI has no entry point that launches a sweep kernel alone.
The candidate and the gains are what five solver iterations from a cold start leave, as in tools/time_covariance.py, except on
talos_arm_sea: there that solve has diverged on some trajectories by the last knots (|Fx| up to 6e28, |K| up to 1e16), which
is past the call's limit of validity (include/aslr_to_amd_lqg.h), so its plan is the empty candidate with the gains of one
backward sweep on it.  Every output of every form is checked to be finite."""
import sys

import torch

from _timing import STANDARD_SHAPES, planned, ptr, seeded_spread, timed

# solver iterations from a cold start that make the plan; 0: the empty candidate and one backward sweep
ITERATIONS = {"two_dof_vsa_boxddp": 5, "talos_arm_sea": 0, "talos_arm_vsa": 5}


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    for name, make in STANDARD_SHAPES.items():
        e, sp = planned(make, ITERATIONS[name])
        s0, w, r = seeded_spread(e)   # r: [B][ny] for ny = nx
        rh = r[:, :e.nx // 2].contiguous()
        new = lambda *s: torch.zeros(s, dtype=torch.float64, device=e.device)
        xv, uv, ev, ci = new(e.T + 1, e.B, e.nx), new(e.T, e.B, e.nu), new(e.T + 1, e.B, e.nx), new(e.B)
        cf, ef, kg = new(e.B, e.nx, e.nx), new(e.B, e.nx, e.nx), new(e.T + 1, e.B, e.nx, e.nx // 2)
        outputs = (xv, uv, ev, cf, ef, ci, kg)
        cov = lambda: e._call("aslr_policy_covariance", ptr(s0), ptr(w), ptr(xv), ptr(uv), ptr(cf), None, ptr(ci), e._stream())
        lqg = lambda: e._call("aslr_policy_lqg", e.nx // 2, None, ptr(rh), ptr(s0), ptr(w), ptr(xv), ptr(uv), ptr(ev), ptr(cf), ptr(ef),
                              None, ptr(ci), e._stream())
        lqg_all = lambda: e._call("aslr_policy_lqg", e.nx, None, ptr(r), ptr(s0), ptr(w), ptr(xv), ptr(uv), ptr(ev), ptr(cf), ptr(ef),
                                  None, ptr(ci), e._stream())
        filt = lambda: e._call("aslr_policy_lqg", e.nx // 2, None, ptr(rh), ptr(s0), ptr(w), None, None, ptr(ev), None, None,
                               ptr(kg), None, e._stream())
        for fn in (e.calc_diff, cov, lqg_all, filt, lqg):  # warm-up: code objects loaded, records in place
            fn()
            torch.cuda.synchronize()
            assert all(bool(torch.isfinite(t).all()) for t in outputs), name
        t_calc = timed(e.calc_diff, repeats)
        t_cov = timed(cov, repeats)
        t_lqg = timed(lqg, repeats)
        t_all = timed(lqg_all, repeats)
        t_filt = timed(filt, repeats)
        assert all(bool(torch.isfinite(t).all()) for t in outputs), name
        print("%s B=%d T=%d nx=%d nu=%d: calc_diff %.3f ms, covariance %.3f ms (sweep %.3f ms), lqg %.3f ms (sweep %.3f ms, %.2f x "
              "covariance's), lqg all %.3f ms (sweep %.3f ms, %.2f x), filter only %.3f ms (sweep %.3f ms)"
              % (name, e.B, e.T, e.nx, e.nu, t_calc, t_cov, t_cov - t_calc, t_lqg, t_lqg - t_calc, (t_lqg - t_calc) / (t_cov - t_calc),
                 t_all, t_all - t_calc, (t_all - t_calc) / (t_cov - t_calc), t_filt, t_filt - t_calc))
        e.close()


if __name__ == "__main__":
    main()
