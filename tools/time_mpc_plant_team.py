"""Times of receding-horizon runs on a mismatched plant on the 7-joint arms (aslr_mpc_run_plant_all, mpc_plant_team_kernel)
beside aslr_mpc_run on the same handle shape: tools/time_mpc_plant_team.py [reps] [n_steps] [iters_per_step] [B] [T]

Shapes: talos_arm_sea with SolverFDDP and talos_arm_vsa with SolverBoxDDP, B = 512, T = 150 (nx = 28, nu = 7 and 14),
n_steps = 12 control steps of 3 iterations each (the first solve as well), disturbance U(-1e-3, 1e-3).  Per shape, alternating
per repetition on a fresh handle each (a run moves X0), after one warm-up repetition, wall clock around a device
synchronisation, median and spread of `reps` (default 7):
  (a) mpc:          Engine.mpc_run, n_steps control steps (the one-knot calc launch + mpc_advance_kernel between solves).
                    This is existing code; with the argument `mpc-only` the tool times nothing else, which is how the
                    baseline on an earlier commit is taken (the tool needs nothing newer than Engine.mpc_run then);
  (b) plant hold=1: Engine.mpc_run_plant with the motor-inertia plant given (within +-20 % of the model's) and the closed
                    cost requested (mpc_plant_team_kernel + mpc_advance_kernel between solves);
  (b0) the same with the model's own inertia as the plant: the closed loop and the solver's work of (a), so the difference
                    to (a) is the plant phase alone;
  (c) plant hold=4: the same with hold = 4 and n_steps / 4 control steps, per control step and per APPLIED KNOT.
The plant kernel alone, with HIP events on the launch stream: one control step at hold = 1, 4 and T takes one solve plus one
plant phase, so (step at hold h) - (step at hold 1) is h - 1 further knots of the kernel; the figure is printed per knot.
One JSON line per shape."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from aslr_to_amd import scenarios  # noqa: E402
from aslr_to_amd.engine import Engine  # noqa: E402

args = [a for a in sys.argv[1:] if a != "mpc-only"]
MPC_ONLY = "mpc-only" in sys.argv[1:]
arg = lambda i, d: int(args[i]) if len(args) > i else d
REPS, N, PER, B, T = arg(0, 7), arg(1, 12), arg(2, 3), arg(3, 512), arg(4, 150)
SHAPES = {"talos_arm_sea": ("SolverFDDP", lambda: scenarios.talos_arm_sea(B=B, T=T, seed=0)),
          "talos_arm_vsa": ("SolverBoxDDP", lambda: scenarios.talos_arm_vsa(B=B, T=T, seed=0))}


def main():
    assert N % 4 == 0, "n_steps must be a multiple of 4 for the hold = 4 run"
    for name, (solver, make) in SHAPES.items():
        sc = make()
        low = scenarios.lower(sc)
        sp = scenarios.solver_params(sc, solver=solver)
        nj = low.nj
        dist = torch.as_tensor(np.random.default_rng(7).uniform(-1e-3, 1e-3, (B, N, low.nx)), device="cuda")
        diag_b = np.array([low.desc.models[0].B[j * nj + j] for j in range(nj)])   # (no table: the model's diagonal)
        pb = diag_b * np.random.default_rng(11).uniform(0.8, 1.2, (B, nj))

        def timed(fn, steps):
            e = Engine(low)
            e.set_candidate(None, None)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(e)   # (synchronises before it returns)
            ms = (time.perf_counter() - t0) * 1e3 / steps
            e.close()
            return ms

        runs = {"mpc": (N, lambda e: e.mpc_run(sp, N, PER, PER, dist))}
        if not MPC_ONLY:
            runs["plant_hold1"] = (N, lambda e: e.mpc_run_plant(sp, N, PER, PER, 1, None, pb, dist, False, True))
            # the same call with the model's own inertia given as the plant: the closed loop, and with it the work of every
            # solve, is that of (a), so what (b0) - (a) shows is the plant phase and its shift alone
            pb0 = np.tile(diag_b, (B, 1))
            runs["plant_hold1_nominal"] = (N, lambda e: e.mpc_run_plant(sp, N, PER, PER, 1, None, pb0, dist, False, True))
            runs["plant_hold4"] = (N // 4, lambda e: e.mpc_run_plant(sp, N // 4, PER, PER, 4, None, pb, dist, False, True))
        ms = {k: [] for k in runs}
        for rep in range(REPS + 1):   # (repetition 0 is the warm-up)
            for k, (steps, fn) in runs.items():
                t = timed(fn, steps)
                if rep:
                    ms[k].append(t)
        out = dict(shape=name, solver=solver, B=B, T=T, n_steps=N, iters_per_step=PER, reps=REPS, gpu=torch.cuda.get_device_name(0))
        for k, v in ms.items():
            out[k + "_ms_per_step"] = statistics.median(v)
            out[k + "_ms_min_max"] = [min(v), max(v)]
        if not MPC_ONLY:
            out["plant_hold4_ms_per_applied_knot"] = out["plant_hold4_ms_per_step"] / 4
            out["plant_hold1_over_mpc"] = out["plant_hold1_ms_per_step"] / out["mpc_ms_per_step"]
            out["plant_hold1_nominal_over_mpc"] = out["plant_hold1_nominal_ms_per_step"] / out["mpc_ms_per_step"]
            # the plant kernel by difference: one control step (solve + plant phase + shift) at hold = 1, 4, T
            step = {}
            dist_h = torch.as_tensor(np.random.default_rng(8).uniform(-1e-3, 1e-3, (B, T, low.nx)), device="cuda")
            for h in (1, 4, T):
                v = []
                for rep in range(REPS + 1):
                    e = Engine(low)
                    e.set_candidate(None, None)
                    torch.cuda.synchronize()
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    e.mpc_run_plant(sp, 1, PER, PER, h, None, pb, dist_h[:, :h].contiguous(), False, True)
                    t1.record()
                    t1.synchronize()
                    if rep:
                        v.append(t0.elapsed_time(t1))
                    e.close()
                step[h] = statistics.median(v)
            out["one_step_ms_hold_1_4_T"] = [step[1], step[4], step[T]]
            out["plant_kernel_us_per_knot_from_hold4"] = 1e3 * (step[4] - step[1]) / 3
            out["plant_kernel_us_per_knot_from_holdT"] = 1e3 * (step[T] - step[1]) / (T - 1)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
