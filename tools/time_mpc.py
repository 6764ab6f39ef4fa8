"""Milliseconds per control step of a receding-horizon run of SolverBoxDDP on the 2-DoF VSA arm (B = 4096, T = 100,
n_steps = 50, iters_per_step = 2, first solve 2 iterations, disturbance U(-1e-3, 1e-3)):
  (a) device: one aslr_mpc_run call (Engine.mpc_run);
  (b) host:   the same closed loop driven from Python through solve, calc and torch shifts of the region views
              (tests/_mpc_loop.py), which is what the library offered before aslr_mpc_run.
Both start from the empty candidate on a fresh handle each repetition (a run moves X0), are warmed up once and then
timed REPS times, alternating (a) and (b), wall clock around a device synchronisation; the medians and the spread are
reported in one JSON line.
usage: python tools/time_mpc.py [B] [T] [n_steps] [iters_per_step] [reps]

With a sixth argument `plant` the comparison is instead between aslr_mpc_run and aslr_mpc_run_plant on the same shape
(include/aslr_to_amd_mpc_plant.h), alternating per repetition:
  (a) mpc:          Engine.mpc_run, n_steps control steps (the one-knot calc launch + mpc_advance_kernel between solves);
  (c) plant hold=1: Engine.mpc_run_plant with the motor-inertia plant given (within +-20 % of the model's) and the closed cost
                    requested, n_steps control steps (mpc_plant_kernel + mpc_advance_kernel between solves);
  (d) plant hold=4: the same with hold = 4 and n_steps / 4 control steps, reported per control step and per APPLIED KNOT.
usage: python tools/time_mpc.py 4096 100 48 3 7 plant"""
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


def timed(fn, steps=N):
    e = Engine(low)
    e.set_candidate(None, None)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(e)
    ms = (time.perf_counter() - t0) * 1e3 / steps
    e.close()
    return ms


def plant_mode():
    nj = low.nj
    diag_b = np.array([low.desc.models[0].B[j * nj + j] for j in range(nj)])   # (the scenario has no table: the model's diagonal)
    pb = diag_b * np.random.default_rng(11).uniform(0.8, 1.2, (B, nj))
    assert N % 4 == 0, "n_steps must be a multiple of 4 for the hold = 4 run"
    runs = {"mpc": (N, lambda e: e.mpc_run(sp, N, PER, PER, dist_bm)),
            "plant_hold1": (N, lambda e: e.mpc_run_plant(sp, N, PER, PER, 1, None, pb, dist_bm, True, True)),
            "plant_hold4": (N // 4, lambda e: e.mpc_run_plant(sp, N // 4, PER, PER, 4, None, pb, dist_bm, True, True))}
    ms = {k: [] for k in runs}
    for rep in range(REPS + 1):   # (repetition 0 is the warm-up)
        for k, (steps, fn) in runs.items():
            t = timed(fn, steps)
            if rep:
                ms[k].append(t)
    out = dict(B=B, T=T, n_steps=N, iters_per_step=PER, reps=REPS, gpu=torch.cuda.get_device_name(0))
    for k, v in ms.items():
        out[k + "_ms_per_step"] = float(np.median(v))
        out[k + "_ms_min_max"] = [min(v), max(v)]
    out["plant_hold4_ms_per_applied_knot"] = out["plant_hold4_ms_per_step"] / 4
    out["plant_hold1_over_mpc"] = out["plant_hold1_ms_per_step"] / out["mpc_ms_per_step"]
    print(json.dumps(out))


if len(sys.argv) > 6 and sys.argv[6] == "plant":
    plant_mode()
    sys.exit(0)
for fn in (device, host):   # warm-up: code objects, torch's copy kernels, the allocator
    timed(fn)
a, b = [], []
for _ in range(REPS):
    a.append(timed(device))
    b.append(timed(host))
print(json.dumps(dict(B=B, T=T, n_steps=N, iters_per_step=PER, reps=REPS, device_ms_per_step=float(np.median(a)),
                      host_ms_per_step=float(np.median(b)), device_ms_min_max=[min(a), max(a)],
                      host_ms_min_max=[min(b), max(b)], gpu=torch.cuda.get_device_name(0))))
