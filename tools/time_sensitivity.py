"""Times of the adjoint sweep (aslr_cost_sensitivity) beside the two sweeps it sits between, with HIP events on the launch
stream: tools/time_sensitivity.py [repeats]

Shapes: C3 (two_dof_vsa_boxddp, B = 4096, T = 100, nx = 8, nu = 4) and C5 (talos_arm_sea, B = 512, T = 150, nx = 28).
Per shape, the median over `repeats` (default 20) of
  calc_diff         aslr_calc_diff alone;
  sensitivity       aslr_cost_sensitivity with all outputs (SEA) or all but the stiffness (VSA): the calcDiff sweep and
                    adjoint_kernel, back to back on one stream;
  adjoint           sensitivity - calc_diff: the C ABI has no entry point that launches adjoint_kernel alone;
  backward          aslr_backward_pass of the same handle on the same records (existing code, for comparison).
The candidate is what five solver iterations from a cold start leave, so that the backward sweep factors every knot."""
import sys

import torch

from _timing import STANDARD_SHAPES, planned, ptr, timed
from aslr_to_amd import _abi

SHAPES = {"C3": STANDARD_SHAPES["two_dof_vsa_boxddp"], "C5": STANDARD_SHAPES["talos_arm_sea"]}


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    for name, make in SHAPES.items():
        e, sp = planned(make, 5)
        nj, vsa = e.nx // 4, e.low.dam == _abi.DAM_VSA
        new = lambda *s: torch.zeros(s, dtype=torch.float64, device=e.device)
        dk, db, dx0, lam = (None if vsa else new(nj, e.B)), new(nj, e.B), new(e.nx, e.B), new(e.T + 1, e.B, e.nx)
        sens = lambda: e._call("aslr_cost_sensitivity", ptr(dk), ptr(db), ptr(dx0), ptr(lam), e._stream())
        for fn in (e.calc_diff, sens, lambda: e.backward_pass(sp)):  # warm-up: code objects loaded, records in place
            fn()
        torch.cuda.synchronize()
        t_calc = timed(e.calc_diff, repeats)
        t_sens = timed(sens, repeats)
        t_bwd = timed(lambda: e.backward_pass(sp), repeats)
        failed = int(((e.traj_i(_abi.TI_STATUS) & _abi.ST_BACKWARD_ERR) != 0).sum().item())
        print("%s B=%d T=%d nx=%d nu=%d: calc_diff %.3f ms, sensitivity %.3f ms, adjoint %.3f ms, backward %.3f ms "
              "(backward failed on %d trajectories)" % (name, e.B, e.T, e.nx, e.nu, t_calc, t_sens, t_sens - t_calc, t_bwd, failed))
        e.close()


if __name__ == "__main__":
    main()
