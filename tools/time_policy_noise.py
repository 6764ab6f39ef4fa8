"""Times of the Monte-Carlo policy roll-out that draws its noise on the device (aslr_policy_rollout_noise) beside the array
form (aslr_policy_rollout / aslr_policy_rollout_all) and beside what the array form costs the host, with HIP events on the
launch stream: tools/time_policy_noise.py [repeats] [S]

Shapes: two_dof_vsa_boxddp, B = 4096, T = 100 (nx = 8, nu = 4); talos_arm_sea and talos_arm_vsa, B = 512, T = 150 (nx = 28);
S = 64 samples per trajectory (default).  Every sigma the model admits is given (noise_std 3e-4, dx0_std 3e-3, plant 0.05
relative); both forms ask for cost, failed_knot and x_final.  Per shape, the median over `repeats` (default 20), after a
warm-up of every call, of
  drawn inside    aslr_policy_rollout_noise;
  from arrays     the array form on arrays that are already on the device (the drawn_* outputs of one noise call, so both
                  forms roll the same samples out);
and, once (wall clock, not a median: it takes seconds),
  host draw       numpy's standard_normal for the four arrays of the array form, scaled, and their upload.
Then, on the two-joint shape only, the noise call at growing S with `cost` as its only output: the array form's disturbance
alone would be 8 S T B nx bytes there."""
import ctypes as C
import sys
import time

import numpy as np
import torch

from _timing import STANDARD_SHAPES, planned, ptr, timed
from aslr_to_amd import _abi

NOISE_STD, DX0_STD, PLANT_REL_STD = 3e-4, 3e-3, 0.05
LARGE_S = (1024, 8192, 65536)
SEED = 2026


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    S = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    for name, make in STANDARD_SHAPES.items():
        e, sp = planned(make, 5)
        B, T, nx, nu, nj = e.B, e.T, e.nx, e.nu, e.nx // 4
        sea = e.low.dam == _abi.DAM_SEA
        clamp = 1 if sp.solver == _abi.SOLVER_BOXDDP else 0
        new = lambda dt, *s: torch.zeros(s, dtype=dt, device=e.device)
        full = lambda v, n: torch.full((B, n), v, dtype=torch.float64, device=e.device)
        sw, s0, sk, sb = full(NOISE_STD, nx), full(DX0_STD, nx), (full(PLANT_REL_STD, nj) if sea else None), full(PLANT_REL_STD, nj)
        cost, failed, xf = new(torch.float64, S, B), new(torch.int32, S, B), new(torch.float64, S, B, nx)
        pk, pb = (new(torch.float64, nj, S, B) if sea else None), new(torch.float64, nj, S, B)
        d0, w = new(torch.float64, S, B, nx), new(torch.float64, S, T, B, nx)
        noise = lambda n, outs, drawn: e._call("aslr_policy_rollout_noise", n, 0, 0, C.c_uint64(SEED), ptr(sw), ptr(s0), ptr(sk), ptr(sb), clamp,
                                               *[ptr(t) for t in outs], *[ptr(t) for t in drawn], e._stream())
        old = "aslr_policy_rollout" if nj == 2 else "aslr_policy_rollout_all"
        inside = lambda: noise(S, (cost, failed, xf, None, None), (None, None, None, None))
        arrays = lambda: e._call(old, S, ptr(pk), ptr(pb), ptr(d0), ptr(w), clamp, ptr(cost), ptr(failed), ptr(xf), None, None, e._stream())
        noise(S, (cost, failed, xf, None, None), (pk, pb, d0, w))  # the arrays of the array form: this seed's draws
        torch.cuda.synchronize()
        cost_inside = cost.clone()
        for fn in (inside, arrays):  # warm-up: code objects loaded
            fn()
        torch.cuda.synchronize()
        same = bool((cost.view(torch.int64) == cost_inside.view(torch.int64)).all())
        t_in, t_arr = timed(inside, repeats), timed(arrays, repeats)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rng = np.random.default_rng(SEED)
        host = [NOISE_STD * rng.standard_normal((S, T, B, nx)), DX0_STD * rng.standard_normal((S, B, nx)),
                np.exp(PLANT_REL_STD * rng.standard_normal((nj, S, B)))] + ([np.exp(PLANT_REL_STD * rng.standard_normal((nj, S, B)))] if sea else [])
        t_draw = time.perf_counter() - t0
        up = [torch.as_tensor(a).to(e.device) for a in host]
        torch.cuda.synchronize()
        t_up = time.perf_counter() - t0 - t_draw
        del host, up
        print("%s B=%d T=%d S=%d nx=%d nu=%d: failed samples %d of %d; the two forms give the same cost bits: %s"
              % (name, B, T, S, nx, nu, int((failed >= 0).sum()), S * B, same))
        for k, v in (("drawn inside", t_in), ("from arrays", t_arr)):
            print("  %-13s %9.3f ms  %8.3f ns per (sample, trajectory)  %7.3f ns per (sample, trajectory, knot)"
                  % (k, v, 1e6 * v / (S * B), 1e6 * v / (S * B * T)))
        print("  %-13s %9.1f ms draw + %.1f ms upload, %.2f GB of arrays (disturbance %.2f GB)"
              % ("host draw", 1e3 * t_draw, 1e3 * t_up, 8e-9 * (S * T * B * nx + S * B * nx + (2 if sea else 1) * nj * S * B), 8e-9 * S * T * B * nx))
        if nj == 2:
            del w, d0
            torch.cuda.empty_cache()
            for big in LARGE_S:
                c = new(torch.float64, big, B)
                run = lambda: noise(big, (c, None, None, None, None), (None, None, None, None))
                run()
                torch.cuda.synchronize()
                ms = timed(run, 3)
                print("  S = %-7d %9.1f ms  %8.3f ns per (sample, trajectory); failed %d; the array form's disturbance would be %.0f GB"
                      % (big, ms, 1e6 * ms / (big * B), int(torch.isnan(c).sum()), 8e-9 * big * T * B * nx))
                del c
        e.close()


if __name__ == "__main__":
    main()
