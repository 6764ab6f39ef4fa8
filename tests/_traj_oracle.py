"""The per-trajectory oracle loop of the parameter-table tests: the expected result for trajectory b of a batch with a
per-trajectory parameter table is the CPU oracle on a B = 1 problem whose models carry that trajectory's K, B and control
box -- the loop a user writes without the table (one problem per design)."""
import ctypes as C

import numpy as np

from aslr_to_amd import _abi
from aslr_to_amd.lowering import LoweredProblem


def single(low, b):
    """B = 1 lowered problem of trajectory b; its models hold row b of low.traj_params where a field is given."""
    desc = _abi.ProblemDesc()
    C.memmove(C.byref(desc), C.byref(low.desc), C.sizeof(desc))
    desc.B = 1
    x0 = np.ascontiguousarray(low.x0[b:b + 1])
    fr = None if low.frame_ref is None else np.ascontiguousarray(low.frame_ref[b:b + 1])
    desc.x0 = x0.ctypes.data_as(C.POINTER(C.c_double))
    desc.frame_ref = None if fr is None else fr.ctypes.data_as(C.POINTER(C.c_double))
    tp, nj, nu = low.traj_params or {}, low.nj, low.nu
    for i in range(desc.nmodels):
        m = desc.models[i]
        for j in range(nj):
            if "stiffness" in tp:
                m.K[j * nj + j] = tp["stiffness"][b, j]
            if "motor_inertia" in tp:
                m.B[j * nj + j] = tp["motor_inertia"][b, j]
        if m.has_u_limits:
            for c in range(nu):
                if "u_lb" in tp:
                    m.u_lb[c] = tp["u_lb"][b, c]
                if "u_ub" in tp:
                    m.u_ub[c] = tp["u_ub"][b, c]
    return LoweredProblem(desc, low.node_model, x0, fr, low.nj, low.nx, low.nu, low.dam, low.nu_user)


def calc_diff(oracle, low, xs, us):
    outs = [oracle.calc_diff(single(low, b), xs[:, b:b + 1], us[:, b:b + 1]) for b in range(low.B)]
    return tuple(np.concatenate([o[k] for o in outs], axis=1) for k in range(3))


def backward_pass(oracle, low, sp, deriv, gaps, us, xreg, feasible, kff0):
    outs = [oracle.backward_pass(single(low, b), sp, deriv[:, b:b + 1], gaps[:, b:b + 1], us[:, b:b + 1], xreg, feasible,
                                 kff0=kff0[:, b:b + 1]) for b in range(low.B)]
    out = {}
    for k in outs[0]:
        out[k] = np.concatenate([o[k] for o in outs], axis=1 if outs[0][k].ndim > 1 else 0)
    return out


def forward_pass(oracle, low, sp, alpha, xs, us, K, k):
    outs = [oracle.forward_pass(single(low, b), sp, alpha, xs[:, b:b + 1], us[:, b:b + 1], K[:, b:b + 1], k[:, b:b + 1])
            for b in range(low.B)]
    return (np.concatenate([o[0] for o in outs], axis=1), np.concatenate([o[1] for o in outs], axis=1),
            np.concatenate([o[2] for o in outs]), np.concatenate([o[3] for o in outs]))


def solve(oracle, low, sp, log_cap=0):
    outs = [oracle.solve(single(low, b), sp, log_cap=log_cap) for b in range(low.B)]
    out = dict(xs=np.concatenate([o["xs"] for o in outs], axis=1), us=np.concatenate([o["us"] for o in outs], axis=1),
               traj_f=np.concatenate([o["traj_f"] for o in outs], axis=1),
               traj_i=np.concatenate([o["traj_i"] for o in outs], axis=1))
    if log_cap:
        out["log"] = np.concatenate([o["log"] for o in outs], axis=2)
    return out
