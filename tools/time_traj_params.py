"""Per-iteration time of the c3 (B = 4096, 2-DoF VSA, T = 100, BoxDDP), c5 (B = 512, 7-DoF SEA, T = 150, DDP) and 7-DoF
VSA (B = 512, T = 50, BoxDDP) shapes
without a per-trajectory parameter table and with one (every row = the models' constants: same iterates, other kernels):
python tools/time_traj_params.py [iterations]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from aslr_to_amd import scenarios
from aslr_to_amd.engine import Engine

n = int(sys.argv[1]) if len(sys.argv) > 1 else 40
for name, sc in (("c3", scenarios.two_dof_vsa_boxddp(B=4096, T=100, seed=0)), ("c5", scenarios.talos_arm_sea(B=512, T=150, seed=0)),
                 ("vsa7", scenarios.talos_arm_vsa(B=512, T=50, seed=3))):  # (vsa7: 7-DoF VSA, BoxDDP: the block kernel reads the box)
    sp = scenarios.solver_params(sc, fixed_iterations=1)
    for table in (False, True):
        s = dict(sc)
        s["traj_params"] = scenarios.constant_traj_params(sc) if table else None
        e = Engine(scenarios.lower(s))
        e.set_subshards(4)
        e.set_candidate(None, None)
        e.iterate_n(sp, True, 10)
        torch.cuda.synchronize()
        best = 1e9
        for rep in range(3):
            t0 = time.perf_counter()
            e.iterate_n(sp, False, n)
            torch.cuda.synchronize()
            best = min(best, (time.perf_counter() - t0) / n * 1e3)
        print("%s %-13s %.3f ms / iteration (best of 3 x %d, 4 sub-shards)" % (name, "with table" if table else "without table", best, n))
        e.close()
