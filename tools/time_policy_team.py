"""Times of the 7-joint closed-loop policy roll-out (aslr_policy_rollout_all, policy_rollout_team_kernel) beside the solver's
forward pass of the same handle, with HIP events on the launch stream: tools/time_policy_team.py [repeats] [S]

Shapes: talos_arm_sea and talos_arm_vsa, B = 512, T = 150 (nx = 28, nu = 7 and 14), S = 64 samples per trajectory (default).
Per shape, the median over `repeats` (default 20), after a warm-up of every call, of
  costs only      the call with plant arrays, dx0 and a disturbance, asking for cost, failed_knot and x_final (what the Python
                  facade asks for without keep_trajectories);
  trajectories    the same with xs_closed and us_closed as well;
  nominal         every input NULL, costs only;
  forward pass    aslr_forward_pass (existing code, for comparison): rollout_team_kernel<7> over the 10 step lengths, then the
                  trial-cost and line-search kernels; the C ABI has no entry point that launches the roll-out kernel alone, so
                  the per-knot figure of that column is an upper bound for it.
Per-knot figures: time / T per launch (all teams run at once when they fit the device), and time / (S B T) resp.
time / (10 B T) per (sample or step length, trajectory, knot).  The candidate and the gains are what five solver iterations
from a cold start leave; the plants are the trajectories' own within +-30 %, |dx0| <= 1e-2, |w| <= 1e-3."""
import sys

import torch

from _timing import STANDARD_SHAPES, planned, ptr, timed
from aslr_to_amd import _abi

SHAPES = {name: STANDARD_SHAPES[name] for name in ("talos_arm_sea", "talos_arm_vsa")}
NALPHA = 10


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    S = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    for name, make in SHAPES.items():
        e, sp = planned(make, 5)
        low = e.low
        B, T, nx, nu, nj = e.B, e.T, e.nx, e.nu, e.nx // 4
        sea = low.dam == _abi.DAM_SEA
        gen = torch.Generator(device="cpu").manual_seed(0)
        rand = lambda lo, hi, *s: (lo + (hi - lo) * torch.rand(s, generator=gen, dtype=torch.float64)).to(e.device)
        m0 = low.desc.models[0]
        diag = lambda f: torch.tensor([getattr(m0, f)[j * nj + j] for j in range(nj)], dtype=torch.float64, device=e.device)
        pk = diag("K")[:, None, None] * rand(0.7, 1.3, nj, S, B) if sea else None
        pb = diag("B")[:, None, None] * rand(0.7, 1.3, nj, S, B)
        d0, w = rand(-1e-2, 1e-2, S, B, nx), rand(-1e-3, 1e-3, S, T, B, nx)
        new = lambda dt, *s: torch.zeros(s, dtype=dt, device=e.device)
        cost, failed, xf = new(torch.float64, S, B), new(torch.int32, S, B), new(torch.float64, S, B, nx)
        xs, us = new(torch.float64, S, T + 1, B, nx), new(torch.float64, S, T, B, nu)
        call = lambda ins, outs: e._call("aslr_policy_rollout_all", S, *[ptr(t) for t in ins], 0, *[ptr(t) for t in outs], e._stream())
        lean = lambda: call((pk, pb, d0, w), (cost, failed, xf, None, None))
        full = lambda: call((pk, pb, d0, w), (cost, failed, xf, xs, us))
        nominal = lambda: call((None, None, None, None), (cost, failed, xf, None, None))
        fwd = lambda: e.forward_pass(sp)
        for fn in (lean, full, nominal, fwd):  # warm-up: code objects loaded
            fn()
        torch.cuda.synchronize()
        t = {k: timed(fn, repeats) for k, fn in (("costs only", lean), ("trajectories", full), ("nominal", nominal))}
        t_fwd = timed(fwd, repeats)
        lean()
        torch.cuda.synchronize()
        print("%s B=%d T=%d S=%d nx=%d nu=%d: failed samples %d of %d" % (name, B, T, S, nx, nu, int((failed >= 0).sum()), S * B))
        for k, v in t.items():
            print("  %-14s %8.3f ms  %7.2f us per knot of the launch  %7.3f ns per (sample, trajectory, knot)"
                  % (k, v, 1e3 * v / T, 1e6 * v / (S * B * T)))
        print("  %-14s %8.3f ms  %7.2f us per knot of the launch  %7.3f ns per (step length, trajectory, knot)"
              % ("forward pass", t_fwd, 1e3 * t_fwd / T, 1e6 * t_fwd / (NALPHA * B * T)))
        e.close()


if __name__ == "__main__":
    main()
