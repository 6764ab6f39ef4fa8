"""Per-iteration time of the c3 shape (B = 4096, 2-DoF VSA, T = 100, BoxDDP) without a reference path and with a full
[T + 1]-row path set (aslr_set_reference_path; every row = the create-time reference: same iterates, 96 B more read per
knot): python tools/time_ref_path.py [iterations]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from aslr_to_amd import scenarios
from aslr_to_amd.engine import Engine

n = int(sys.argv[1]) if len(sys.argv) > 1 else 40
sc = scenarios.two_dof_vsa_boxddp(B=4096, T=100, seed=0)
sp = scenarios.solver_params(sc, fixed_iterations=1)
full = np.repeat(np.asarray(sc["frame_refs"], dtype=np.float64)[:, None, :], 101, axis=1)
for rnd in range(2):
    for with_path in (False, True):
        e = Engine(scenarios.lower(sc))
        if with_path:
            e.set_reference_path(full)
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
        print("c3 %-26s %.3f ms / iteration (best of 3 x %d, 4 sub-shards)" % ("with a 101-row path" if with_path else "without a path", best, n))
        e.close()
