"""Times of the tangent sweep (aslr_policy_plant_sensitivity) beside the calcDiff sweep and the covariance sweep of the same
handle, with HIP events on the launch stream: tools/time_plant_sens.py [repeats]

Shapes: two_dof_vsa_boxddp (B = 4096, T = 100, nx = 8, nu = 4), talos_arm_sea and talos_arm_vsa (B = 512, T = 150, nx = 28,
nu = 7 and 14).  Per shape, the median over `repeats` (default 20) of
  calc_diff         aslr_calc_diff alone;
  plant sens        aslr_policy_plant_sensitivity with every variance the model has and every output but the two
                    dx_d* trajectories (what the Python facade asks for): the calcDiff sweep and plant_sens_kernel, back to
                    back on one stream;
  motor only        the same with the motor-inertia outputs and variance alone (on a VSA model: the same call);
  derivatives only  dxT_* and dcost_* of every kind, no variance;
  covariance        aslr_policy_covariance as tools/time_covariance.py times it (existing code, for comparison);
  sweep             each call - calc_diff: the C ABI has no entry point that launches the sweep kernels alone.
The candidate and the gains are what five solver iterations from a cold start leave."""
import sys

import torch

from _timing import STANDARD_SHAPES, planned, ptr, seeded_spread, timed
from aslr_to_amd import _abi


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    for name, make in STANDARD_SHAPES.items():
        e, _ = planned(make, 5)
        sea = e.low.dam == _abi.DAM_SEA
        nj = e.nx // 4
        gen = torch.Generator(device="cpu").manual_seed(0)
        new = lambda *s: torch.zeros(s, dtype=torch.float64, device=e.device)
        var = lambda: (0.1 + 0.9 * torch.rand((nj, e.B), generator=gen, dtype=torch.float64)).to(e.device)
        vk, vb = (var() if sea else None), var()
        fk, ck = (new(e.B, e.nx, nj), new(nj, e.B)) if sea else (None, None)
        fb, cb, xv, uv = new(e.B, e.nx, nj), new(nj, e.B), new(e.T + 1, e.B, e.nx), new(e.T, e.B, e.nu)
        s0, w, _ = seeded_spread(e, gen)
        cf, ci = new(e.B, e.nx, e.nx), new(e.B)
        call = lambda *a: e._call("aslr_policy_plant_sensitivity", *[ptr(t) for t in a], e._stream())
        full = lambda: call(vk, vb, None, None, fk, fb, ck, cb, xv, uv)
        motor = lambda: call(None, vb, None, None, None, fb, None, cb, xv, uv)
        deriv = lambda: call(None, None, None, None, fk, fb, ck, cb, None, None)
        cov = lambda: e._call("aslr_policy_covariance", ptr(s0), ptr(w), ptr(xv), ptr(uv), ptr(cf), None, ptr(ci), e._stream())
        for fn in (e.calc_diff, full, motor, deriv, cov):  # warm-up: code objects loaded, records in place
            fn()
        torch.cuda.synchronize()
        t_calc = timed(e.calc_diff, repeats)
        t = {k: timed(fn, repeats) for k, fn in (("plant sens", full), ("motor only", motor), ("derivatives only", deriv),
                                                 ("covariance", cov))}
        full()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(xv).all()) and bool(torch.isfinite(cb).all())
        print("%s B=%d T=%d nx=%d nu=%d: calc_diff %.3f ms, " % (name, e.B, e.T, e.nx, e.nu, t_calc)
              + ", ".join("%s %.3f ms (sweep %.3f ms)" % (k, v, v - t_calc) for k, v in t.items()))
        e.close()


if __name__ == "__main__":
    main()
