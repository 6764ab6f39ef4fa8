"""Shared by tests/test_sensitivity_host.py and tests/test_gpu_sensitivity.py: what the CPU oracle says about the cost
sensitivities of aslr_cost_sensitivity (include/aslr_to_amd_sens.h), without changing the oracle.

 - expected(): the costates and the three gradients from the DEFINITION -- lambda_T = Lx_T, lambda_t = Lx_t + Fx_t^T
   lambda_{t+1}, dJ/dtheta_j = sum_t lambda_{t+1}^T dxnext_t/dtheta_j -- on the oracle's records, with dxnext/dK_j and
   dxnext/d(1/B_j) as central differences of the oracle's own knot evaluation on tests/_traj_oracle.single(low, b) with the
   parameter moved.  xnext is linear in K_j and in 1 / B_j, so these differences are exact up to rounding whatever the
   step; dJ/dB_j = -(1 / B_j^2) dJ/d(1/B_j).  The two closed-form identities the kernel uses appear nowhere here.
 - rollout(): the oracle's open-loop rollout (forward_pass with zero gains: u = us exactly), whose total cost _open_loop
   returns; fd_rollout(): central differences of that cost in every K_j, B_j and x0_i -- the independent second check.
 - fd_optimum(): central differences of the CONVERGED cost of re-solved, perturbed problems.

Everything is time-major going in ([T+1, B, nx], [T, B, nu], the oracle's layout) and batch-major coming out, like the
public getters: stiffness [B, nj] (None for VSA), motor_inertia [B, nj], x0 [B, nx], costate [B, T+1, nx]."""
import numpy as np

import _traj_oracle
from _gpu_case import relerr  # noqa: F401 (sens.relerr of the host suites)
from aslr_to_amd import _abi


def diag(low, b, field, mi=0):
    """diagonal of K or B of model mi as trajectory b has it (its row of the table, else the model's constant)"""
    nj = low.nj
    m = _traj_oracle.single(low, b).desc.models[mi]
    return np.array([getattr(m, field)[j * nj + j] for j in range(nj)])


def moved(low, b, field, j, value, x0=None):
    """B = 1 problem of trajectory b with entry j of the diagonal of `field` (K or B) set to `value` in EVERY model, and
    optionally another x0.  field None: only x0 moves."""
    lb = _traj_oracle.single(low, b)
    if field is not None:
        for i in range(lb.desc.nmodels):
            getattr(lb.desc.models[i], field)[j * low.nj + j] = value
    if x0 is not None:
        import ctypes as C
        lb.x0 = np.array(x0, dtype=np.float64).reshape(1, low.nx)  # (an array of its own: single() may hand out a view)
        lb.desc.x0 = lb.x0.ctypes.data_as(C.POINTER(C.c_double))
    return lb


def records(oracle, low, xs, us, path=None):
    """(xnext, cost, deriv) of the candidate; path = (path_tm, row0): against a reference path (tests/_ref_path.sweep)"""
    if path is not None:
        import _ref_path
        return _ref_path.sweep(oracle, low, xs, us, path[0], path[1])
    return _traj_oracle.calc_diff(oracle, low, xs, us)


def expected(oracle, low, xs, us, path=None):
    T, B, nx, nu, nj = low.T, low.B, low.nx, low.nu, low.nj
    sea = low.dam == _abi.DAM_SEA
    o = _abi.record_offsets(nx, nu)
    deriv = records(oracle, low, xs, us, path)[2]
    Fx = deriv[:, :, o["Fx"]:o["Fx"] + nx * nx].reshape(T + 1, B, nx, nx)
    Lx = deriv[:, :, o["Lx"]:o["Lx"] + nx]
    lam = np.zeros((T + 1, B, nx))
    lam[T] = Lx[T]
    for t in range(T - 1, -1, -1):
        lam[t] = Lx[t] + np.einsum("bij,bi->bj", Fx[t], lam[t + 1])
    dK, dB = np.zeros((B, nj)), np.zeros((B, nj))
    for b in range(B):
        for j in range(nj):
            for t in range(T):
                mi = int(low.node_model[t])
                xn = lambda lb: oracle.knot(lb, mi, xs[t, b], us[t, b], diff=False)["xnext"]
                if sea:
                    k = diag(low, b, "K", mi)[j]
                    h = 0.25 * abs(k) if k != 0.0 else 0.25
                    dK[b, j] += lam[t + 1, b] @ ((xn(moved(low, b, "K", j, k + h)) - xn(moved(low, b, "K", j, k - h))) / (2 * h))
                r = 1.0 / diag(low, b, "B", mi)[j]
                h = 0.25 * r
                d = (xn(moved(low, b, "B", j, 1.0 / (r + h))) - xn(moved(low, b, "B", j, 1.0 / (r - h)))) / (2 * h)
                dB[b, j] += -(r * r) * (lam[t + 1, b] @ d)
    return dict(stiffness=dK if sea else None, motor_inertia=dB, x0=lam[0].copy(), costate=lam.transpose(1, 0, 2).copy())


def _open_loop(oracle, lb, us_b):
    sp = _abi.default_solver_params(_abi.SOLVER_DDP)
    T, nx, nu = lb.T, lb.nx, lb.nu
    xs0 = np.zeros((T + 1, 1, nx))
    xs0[0, 0] = lb.x0[0]
    xs_try, us_try, cost_try, fail = oracle.forward_pass(lb, sp, 1.0, xs0, us_b, np.zeros((T, 1, nu, nx)), np.zeros((T, 1, nu)))
    assert not fail.any()
    np.testing.assert_array_equal(us_try, us_b)
    return xs_try, float(cost_try[0])


def rollout(oracle, low, us):
    """xs [T+1, B, nx] of the open-loop rollout of us from x0, trajectory by trajectory with its own parameters"""
    return np.concatenate([_open_loop(oracle, _traj_oracle.single(low, b), us[:, b:b + 1])[0] for b in range(low.B)], axis=1)


def fd_rollout(oracle, low, us, rel):
    """central differences of the open-loop rollout cost with steps rel * |value| (x0: rel * max(1, |x0_i|))"""
    B, nj, nx = low.B, low.nj, low.nx
    sea = low.dam == _abi.DAM_SEA
    dK, dB, dx0 = np.zeros((B, nj)), np.zeros((B, nj)), np.zeros((B, nx))
    for b in range(B):
        J = lambda lb: _open_loop(oracle, lb, us[:, b:b + 1])[1]
        for field, out in (("K", dK), ("B", dB)):
            if field == "K" and not sea:
                continue
            v = diag(low, b, field)
            for j in range(nj):
                h = rel * abs(v[j])
                out[b, j] = (J(moved(low, b, field, j, v[j] + h)) - J(moved(low, b, field, j, v[j] - h))) / (2 * h)
        for i in range(nx):
            h = rel * max(1.0, abs(low.x0[b, i]))
            xp, xm = low.x0[b].copy(), low.x0[b].copy()
            xp[i] += h
            xm[i] -= h
            dx0[b, i] = (J(moved(low, b, None, 0, 0.0, x0=xp)) - J(moved(low, b, None, 0, 0.0, x0=xm))) / (2 * h)
    return dict(stiffness=dK if sea else None, motor_inertia=dB, x0=dx0)


def fd_optimum(oracle, low, sp, rel):
    """central differences of the converged cost of re-solved problems with K_j / B_j moved by rel * value -> dict(stiffness,
    motor_inertia) [B, nj]; every re-solve must converge"""
    B, nj = low.B, low.nj
    out = dict(stiffness=np.zeros((B, nj)), motor_inertia=np.zeros((B, nj)))

    def J(lb):
        r = oracle.solve(lb, sp)
        assert (r["traj_i"][_abi.TI_STATUS] & _abi.ST_CONVERGED).all(), "a perturbed re-solve did not converge"
        return float(r["traj_f"][_abi.TF_COST][0])

    for b in range(B):
        for field, name in (("K", "stiffness"), ("B", "motor_inertia")):
            v = diag(low, b, field)
            for j in range(nj):
                h = rel * abs(v[j])
                out[name][b, j] = (J(moved(low, b, field, j, v[j] + h)) - J(moved(low, b, field, j, v[j] - h))) / (2 * h)
    return out


# the case of the optimum tests (test_sensitivity_host.py on the oracle, test_gpu_sensitivity.py through the Python facade):
# two_dof_sea, B = 4, T = 20, SolverDDP run to th_stop = 1e-16 (why: test_sensitivity_host.py)
OPT_B, OPT_T, OPT_SEED, OPT_TH_STOP, OPT_MAXITER = 4, 20, 4, 1e-16, 200
OPT_FD = (1e-3, 2.2e-6)   # (relative step, disagreement measured at it on the oracle alone); the bound is ten times that


def optimum_case():
    from aslr_to_amd import scenarios
    sc = scenarios.two_dof_sea(B=OPT_B, T=OPT_T, seed=OPT_SEED)
    return sc, scenarios.solver_params(sc, solver="SolverDDP", th_stop=OPT_TH_STOP, maxiter=OPT_MAXITER)


def optimum_fd(oracle):
    from aslr_to_amd import scenarios
    sc, sp = optimum_case()
    return fd_optimum(oracle, scenarios.lower(sc), sp, OPT_FD[0])
