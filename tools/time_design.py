"""Milliseconds per outer step of a design descent (aslr_design_descent, include/aslr_to_amd_design.h) on one MI355X:
  (a) device: one Engine.design_descent call, n_steps outer steps (stiffness and motor inertia where the model has both);
  (b) host:   the same loop driven from Python through the entry points that existed before -- solve (4-byte polls every 4
              iterations), cost_sensitivity, a D2H of the gradients, the numpy step of tests/_design.py and
              set_trajectory_params (row builder on the host, H2D of the table) -- which is what a user could write;
  (c) parts:  iters_per_step lock-step iterations (iterate_n) and the two sweeps of cost_sensitivity on the same handle,
              each timed alone, so that (a) minus their sum is the call's own overhead (finalize, the step kernel, launches).
Fresh handles per repetition, one warm-up, REPS timed repetitions alternating (a) and (b), wall clock around a device
synchronisation; medians and spread in one JSON line.
The numpy step and the case set-up come from tests/_design.py (tests/ is put on sys.path, as tools/time_mpc.py does for
tests/_mpc_loop.py): run it from a checkout.  "parts" run their first sweep with kModeSkipConst once the record chunks are in
place; the call's outer steps do not (IterOpts::fresh_first), so some of the "own overhead" is iteration cost.
usage: python tools/time_design.py [scenario] [B] [T] [n_steps] [iters_per_step] [reps]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from aslr_to_amd import _abi, scenarios  # noqa: E402
from aslr_to_amd.engine import Engine  # noqa: E402
import _design as D  # noqa: E402

arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
NAME = sys.argv[1] if len(sys.argv) > 1 else "two_dof_sea"
B, T, N, PER, REPS = arg(2, 4096), arg(3, 100), arg(4, 10), arg(5, 4), arg(6, 5)
sc = scenarios.with_traj_params(scenarios.SCENARIOS[NAME](B=B, T=T), seed=5)
low = scenarios.lower(sc)
sp = scenarios.solver_params(sc)
nj, vsa = low.nj, low.dam == _abi.DAM_VSA
tp = sc["traj_params"]
th0 = np.concatenate([np.zeros((nj, B)) if vsa else tp["stiffness"].T, tp["motor_inertia"].T])
lo, hi = np.where(th0 > 0, th0 / 3.0, 1.0), np.where(th0 > 0, th0 * 3.0, 1.0)
active = np.array([not vsa] * nj + [True] * nj)
kb = None if vsa else (lo[:nj].T, hi[:nj].T)
bb = (lo[nj:].T, hi[nj:].T)


def device(e):
    e.design_descent(sp, N, PER, PER, kb, bb)   # (synchronises before it returns)


def host(e):
    st = D.new_state(th0, T, low.nx, low.nu)
    X, U = e.region(_abi.R_XS), e.region(_abi.R_US)
    zeroed = [e.region(r) for r in (_abi.R_KFF, _abi.R_GAPS, _abi.R_VXXF)]
    cand = th0.copy()
    keep = sp.maxiter, sp.is_feasible
    sp.maxiter = PER
    for s in range(N):
        sp.is_feasible = keep[1] if s == 0 else 0
        e.solve(sp, poll_every=4)
        g = e.cost_sensitivity()
        grad = np.concatenate([np.zeros((nj, B)) if vsa else g.stiffness.t().cpu().numpy(), g.motor_inertia.t().cpu().numpy()])
        J = e.traj_f(_abi.TF_COST).cpu().numpy()
        r = D.step(st, s, s == N - 1, J, grad, X.cpu().numpy(), U.cpu().numpy(), active, lo, hi, **D.DEFAULTS)
        X.copy_(torch.as_tensor(r["xs"]))
        U.copy_(torch.as_tensor(r["us"]))
        for z in zeroed:
            z.zero_()
        frozen = st["eta"] < 0.0
        for row in np.nonzero(active)[0]:
            cand[row] = st["theta"][row] if s == N - 1 else np.where(frozen, st["theta"][row], D.candidate(
                st["theta"][row], st["g_acc"][row], st["eta"], D.DEFAULTS["max_rel"], lo[row], hi[row]))
        e.set_trajectory_params(stiffness=None if vsa else np.ascontiguousarray(cand[:nj].T),
                                motor_inertia=np.ascontiguousarray(cand[nj:].T))
    sp.maxiter, sp.is_feasible = keep
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


def parts():
    e = Engine(low)
    e.set_candidate(None, None)
    e.iterate_n(sp, True, PER)
    e.cost_sensitivity()
    torch.cuda.synchronize()
    it, sw = [], []
    for _ in range(REPS):
        t0 = time.perf_counter()
        e.iterate_n(sp, True, PER)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        e.cost_sensitivity()
        torch.cuda.synchronize()
        it.append((t1 - t0) * 1e3)
        sw.append((time.perf_counter() - t1) * 1e3)
    e.close()
    return float(np.median(it)), float(np.median(sw))


for fn in (device, host):   # warm-up: code objects, torch's copy kernels, the allocator
    timed(fn)
a, b = [], []
for _ in range(REPS):
    a.append(timed(device))
    b.append(timed(host))
it_ms, sweep_ms = parts()
print(json.dumps(dict(scenario=NAME, B=B, T=T, n_steps=N, iters_per_step=PER, reps=REPS, device_ms_per_step=float(np.median(a)),
                      host_ms_per_step=float(np.median(b)), device_ms_min_max=[min(a), max(a)], host_ms_min_max=[min(b), max(b)],
                      iterations_ms=it_ms, sensitivity_sweeps_ms=sweep_ms,
                      own_overhead_ms=float(np.median(a)) - it_ms - sweep_ms, gpu=torch.cuda.get_device_name(0))))
