"""Milliseconds per control step of a receding-horizon run of SolverBoxDDP on the 2-DoF VSA arm (B = 4096, T = 100,
n_steps = 50, iters_per_step = 2, first solve 2 iterations, disturbance U(-1e-3, 1e-3)):
  (a) device: one aslr_mpc_run call (Engine.mpc_run);
  (b) host:   the same closed loop driven from Python through solve, calc and torch shifts of the region views
              (tests/_mpc_loop.py), which is what the library offered before aslr_mpc_run.
Both start from the empty candidate on a fresh handle each repetition (a run moves X0), are warmed up once and then
timed REPS times, alternating (a) and (b), wall clock around a device synchronisation; the medians and the spread are
reported in one JSON line.
usage: python tools/time_mpc.py [B] [T] [n_steps] [iters_per_step] [reps]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from aslr_to_amd import scenarios  # noqa: E402
from aslr_to_amd.engine import Engine  # noqa: E402
import _mpc_loop  # noqa: E402

arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
B, T, N, PER, REPS = arg(1, 4096), arg(2, 100), arg(3, 50), arg(4, 2), arg(5, 5)
sc = scenarios.two_dof_vsa_boxddp(B=B, T=T)
low = scenarios.lower(sc)
sp = scenarios.solver_params(sc)
dist_tm = torch.as_tensor(np.random.default_rng(7).uniform(-1e-3, 1e-3, (N, B, low.nx)), device="cuda")
dist_bm = dist_tm.permute(1, 0, 2).contiguous()


def device(e):
    e.mpc_run(sp, N, PER, PER, dist_bm)   # (synchronises before it returns)


def host(e):
    _mpc_loop.host_driven_mpc(e, sp, N, PER, PER, dist_tm)
    torch.cuda.synchronize()


def timed(fn):
    e = Engine(low)
    e.set_candidate(None, None)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(e)
    ms = (time.perf_counter() - t0) * 1e3 / N
    e.close()
    return ms


for fn in (device, host):   # warm-up: code objects, torch's copy kernels, the allocator
    timed(fn)
a, b = [], []
for _ in range(REPS):
    a.append(timed(device))
    b.append(timed(host))
print(json.dumps(dict(B=B, T=T, n_steps=N, iters_per_step=PER, reps=REPS, device_ms_per_step=float(np.median(a)),
                      host_ms_per_step=float(np.median(b)), device_ms_min_max=[min(a), max(a)],
                      host_ms_min_max=[min(b), max(b)], gpu=torch.cuda.get_device_name(0))))
