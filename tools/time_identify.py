"""Milliseconds of a plant identification (aslr_plant_identify, include/aslr_to_amd_identify.h) on one MI355X:
  (a) kernel: identify_normal_kernel alone (the debug export, no sweep) beside the calcDiff sweep of the same handle;
  (b) device: one Engine.plant_identify call, per outer step;
  (c) host:   the same step driven from Python through the entry points that existed before plus numpy -- set_trajectory_params,
              calc_diff, a D2H of XNEXT and of the Fx columns, residuals, Jacobian and normal equations with einsum, a damped
              solve per trajectory with numpy.linalg -- which is what a user could write.
The recorded run is a short solve under the problem's table; the fit starts 10 % off it.  One warm-up, REPS timed repetitions,
wall clock around a device synchronisation; medians in one JSON line.
usage: python tools/time_identify.py [scenario] [B] [T] [n_steps] [reps]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from aslr_to_amd import _abi, scenarios  # noqa: E402
from aslr_to_amd.engine import Engine  # noqa: E402

arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
NAME = sys.argv[1] if len(sys.argv) > 1 else "two_dof_sea"
B, T, N, REPS = arg(2, 4096), arg(3, 100), arg(4, 10), arg(5, 5)
sc = scenarios.with_traj_params(scenarios.SCENARIOS[NAME](B=B, T=T), seed=5)
low = scenarios.lower(sc)
sp = scenarios.solver_params(sc, maxiter=5)
nj, nx, vsa = low.nj, low.nx, low.dam == _abi.DAM_VSA
tp = sc["traj_params"]
k0 = None if vsa else tp["stiffness"] * 1.1
b0 = tp["motor_inertia"] * 1.1
kb = None if vsa else (k0 / 3, k0 * 3)
bb = (b0 / 3, b0 * 3)
o = _abi.record_offsets(nx, low.nu)

e = Engine(low)
e.set_candidate(None, None)
e.solve(sp, poll_every=0)
torch.cuda.synchronize()
e.lib.aslr_debug_identify_normal.restype = C.c_int
e.lib.aslr_debug_identify_normal.argtypes = [C.c_void_p, C.POINTER(_abi.Identify), C.c_void_p]


def start():
    e.set_trajectory_params(stiffness=k0, motor_inertia=b0)


def sync_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def kernel_alone():
    npar = nj if vsa else 2 * nj
    work = torch.zeros((2 * npar + 1 + npar * (npar + 1) // 2, B), dtype=torch.float64, device=e.device)
    d = _abi.Identify(n_steps=1, fit_stiffness=int(not vsa), fit_motor_inertia=1)
    d.work = work.data_ptr()
    return lambda: _abi.check(e.lib.aslr_debug_identify_normal(e.handle, C.byref(d), e._stream()), "aslr_debug_identify_normal")


def host_step(k, bm, mu):
    """one step as a user writes it: the table, the sweep, the records to the host, numpy"""
    e.set_trajectory_params(stiffness=None if vsa else k, motor_inertia=bm)
    e.calc_diff()
    X, XN = e.region(_abi.R_XS).cpu().numpy(), e.region(_abi.R_XNEXT).cpu().numpy()
    Fx = e.region(_abi.R_DERIV)[:T, :, o["Fx"]:o["Fx"] + nx * nx].reshape(T, B, nx, nx)[..., nj:2 * nj].cpu().numpy()
    dt = low.desc.models[0].dt
    r = X[1:] - XN[:T]
    cols = []
    eye = np.eye(nx)
    if not vsa:
        delta = X[:T, :, :nj] - X[:T, :, nj:2 * nj]
        cols.append(-delta[:, :, None, :] * (Fx - eye[:, nj:2 * nj]))
    D = XN[:T, :, 3 * nj:] - X[:T, :, 3 * nj:]
    cols.append(-D[:, :, None, :] * (dt * eye[:, nj:2 * nj] + eye[:, 3 * nj:]))
    J = np.concatenate(cols, axis=-1)
    H = np.einsum("tbip,tbiq->bpq", J, J)
    g = -np.einsum("tbip,tbi->bp", J, r)
    A = H + mu * H * np.eye(H.shape[-1])
    dz = np.clip(-np.linalg.solve(A, g[..., None])[..., 0], -0.5, 0.5)
    th = np.concatenate(([k] if not vsa else []) + [bm], axis=1) * (1.0 + dz)
    return (None if vsa else th[:, :nj]), th[:, -nj:], float((r * r).sum())


def host_loop():
    k, bm = k0, b0
    for _ in range(N):
        k, bm, _sse = host_step(k, bm, 1e-3)


def device_loop():
    start()
    e.plant_identify(N, None, kb, bb)


start()
normal = kernel_alone()
e.calc_diff()
normal()
device_loop()
host_loop()
t_calc, t_norm, t_dev, t_host = [], [], [], []
for _ in range(REPS):
    start()
    t_calc.append(sync_ms(e.calc_diff))
    t_norm.append(sync_ms(normal))
    t_dev.append(sync_ms(device_loop) / N)
    t_host.append(sync_ms(host_loop) / N)
med = lambda v: float(np.median(v))
print(json.dumps(dict(scenario=NAME, B=B, T=T, n_steps=N, reps=REPS, calc_diff_ms=med(t_calc), normal_kernel_ms=med(t_norm),
                      device_ms_per_step=med(t_dev), host_ms_per_step=med(t_host), gpu=torch.cuda.get_device_name(0))))
