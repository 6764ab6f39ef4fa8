"""A design sweep three ways (profiles/pool_params/): two_dof_vsa_boxddp, T = 100, BoxDDP, th_stop 1e-7, maxiter 400,
P = 4 x 4096 designs (motor inertia x [1/2, 2] log-uniform per joint, control box x [0.6, 1]; the draw of tests/_pool_params.py),
4096 slots, 4 sub-shards.
  (a) four lock-step `solve` batches of 4096 with a parameter table each   -- what a design sweep takes without the feature
  (b) solve_pool with the parameters (aslr_solve_pool_params)
  (c) solve_pool of the same x0 / targets WITHOUT parameters (the models' constants: other problems, other iteration counts)
Useful knot-steps = sum over problems of the iterations each one needed, times T.  One warm-up of each path at a quarter of
the size, then `reps` timed repetitions, wall clock around the synchronised call; every repetition is printed.
python tools/time_pool_params.py [reps] [subshards]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

import numpy as np
import torch

import _pool_params as pp
from aslr_to_amd import _abi, scenarios
from aslr_to_amd.engine import Engine

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
nsub = int(sys.argv[2]) if len(sys.argv) > 2 else 4
B, T, waves = 4096, 100, 4
P = waves * B
sc = scenarios.two_dof_vsa_boxddp(B=P, T=T, seed=0)
sp = scenarios.solver_params(sc)
drawn = pp.draw(sc, 31)
params = {k: v for k, v in drawn.items() if v is not None}
slot_sc = dict(sc, x0=sc["x0"][:B], frame_refs=sc["frame_refs"][:B])
e = Engine(scenarios.lower(slot_sc))
e.set_subshards(nsub)


def batches():
    """(a): per wave -- set the table, cold start, solve to the last straggler, read iterations and status"""
    iters, conv, lock = 0, 0, 0
    for w in range(waves):
        lo = w * B
        e.set_trajectory_params(**{k: v[lo:lo + B] for k, v in params.items()})
        e.region(_abi.R_X0).copy_(torch.as_tensor(sc["x0"][lo:lo + B], device=e.device))
        e.region(_abi.R_FRAME_REF).copy_(torch.as_tensor(sc["frame_refs"][lo:lo + B], device=e.device))
        e.set_candidate(None, None)
        lock += e.solve(sp, poll_every=4)
        torch.cuda.synchronize()
        iters += int(e.traj_i(_abi.TI_ITER).sum().item())
        conv += int(((e.traj_i(_abi.TI_STATUS) & _abi.ST_CONVERGED) != 0).sum().item())
    e.set_trajectory_params()
    return iters, conv, lock


def pool(with_params, n=P):
    r = e.solve_pool(sc["x0"][:n], sc["frame_refs"][:n], sp, refill_every=4, poll_every=16,
                     **({k: v[:n] for k, v in params.items()} if with_params else {}))
    return int(r["iters"].sum().item()), int(((r["status"] & _abi.ST_CONVERGED) != 0).sum().item()), r["batch_iters"]


def timed(what, fn):
    rows = []
    for rep in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        iters, conv, lock = fn()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        rows.append((wall, iters * T / wall))
        print("%s rep %d: wall %.3f s, %d lock-step iterations, %d trajectory iterations, %d of %d converged, %.3e useful knot-steps/s"
              % (what, rep, wall, lock, iters, conv, P, iters * T / wall), flush=True)
    best = min(rows)
    print("%s best of %d: wall %.3f s, %.3e useful knot-steps/s" % (what, reps, best[0], best[1]), flush=True)
    return best


print("device %s, P = %d, slots = %d, T = %d, %d sub-shards" % (torch.cuda.get_device_name(0), P, B, T, nsub), flush=True)
pool(True, B)   # warm-up: every kernel of the three paths has run once
pool(False, B)
a = timed("(a) 4 batches with a table", batches)
b = timed("(b) pool with parameters ", lambda: pool(True))
c = timed("(c) pool, constants only  ", lambda: pool(False))
print("(b) / (a): %.2fx the useful knot-steps/s, %.2fx the wall time" % (b[1] / a[1], b[0] / a[0]))
