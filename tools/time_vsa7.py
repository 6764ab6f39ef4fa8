"""Per-iteration and per-phase times of SolverBoxDDP on the 7-joint VSA arm (nx = 28, nu = 14) at config 5's shape
(B = 512, T = 150), next to the 7-joint SEA arm with SolverDDP measured the same way in the same process.
Fixed-iteration mode (every trajectory iterates every time), cold start; HIP events per phase on one stream
(aslr_iterate_timed), wall clock over 20 iterations for the lock-step iteration with 1 and 4 sub-shards.
usage: python tools/time_vsa7.py [B] [T] [out.json]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aslr_to_amd import scenarios, _abi as A  # noqa: E402
from aslr_to_amd.engine import Engine  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 512
T = int(sys.argv[2]) if len(sys.argv) > 2 else 150
out = {}
for name, sc in (("talos_arm_vsa SolverBoxDDP", scenarios.talos_arm_vsa(B=B, T=T)),
                 ("talos_arm_sea SolverDDP", scenarios.talos_arm_sea(B=B, T=T))):
    low = scenarios.lower(sc)
    sp = scenarios.solver_params(sc, fixed_iterations=1)
    e = Engine(low)
    e.set_candidate(None, None)
    phases = []
    for i in range(30):
        phases.append(e.iterate_timed(sp, i == 0))
    ph = np.array(phases[10:])   # (the first iterations of a cold start are infeasible: plain gains)
    clamped = float((e.region(A.R_QU) == 0.0).double().mean().item())
    row = dict(B=B, T=T, nx=low.nx, nu=low.nu, calcdiff_ms=float(ph[:, 0].mean()), backward_ms=float(ph[:, 1].mean()),
               forward_ms=float(ph[:, 2].mean()), backward_ms_max=float(ph[:, 1].max()), share_of_Qu_clamped=clamped)
    for k in (1, 4):
        e2 = Engine(low)
        e2.set_subshards(k)
        e2.set_candidate(None, None)
        e2.iterate_n(sp, True, 10)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e2.iterate_n(sp, False, 20)
        torch.cuda.synchronize()
        row["iteration_ms_%d_subshards" % k] = (time.perf_counter() - t0) / 20 * 1e3
        del e2
    out[name] = row
    print(name, json.dumps(row))
if len(sys.argv) > 3:
    with open(sys.argv[3], "w") as f:
        json.dump(out, f, indent=1)
