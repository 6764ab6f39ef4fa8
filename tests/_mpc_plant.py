"""Shared by tests/test_mpc_plant_host.py and tests/test_gpu_mpc_plant.py: what the CPU oracle says about
aslr_mpc_run_plant (include/aslr_to_amd_mpc_plant.h), without changing the oracle.

The oracle's solve returns no gains, so the device is held to the definition by induction: one control step against
plant_phase() fed the DEVICE's own plan and gains, then the loop against itself (tests/test_gpu_mpc_plant.py).  Only at
hold = 1, where no gain is read, is there a whole oracle loop: oracle_loop().

 - plant_phase(): the plant phase of one control step as a numpy loop over oracle.knot on the B = 1 problem of trajectory b
   whose models carry the plant's K and B (tests/_policy.plant_problem);
 - shifted(): the shift by hold;
 - oracle_loop(): oracle.solve + one plant knot + shift, per-trajectory plants (hold = 1).

The oracle-loop rows (ROWS, PLANT_RANGE) were chosen by test_oracle_loop_rows_are_stable in tests/test_mpc_plant_host.py, the
criterion of tests/test_mpc_host.py's rows.  Range tried first: +-20 % of the nominal K and B, default_rng(11); both rows hold
the criterion at it, so nothing was halved and no row was rejected."""
import numpy as np

import _policy as pol
import _ref_path
from aslr_to_amd import _abi

# (scenario, solver, B, T, scenario seed), with N_STEPS, FIRST_MAXITER, ITERS_PER_STEP of tests/test_mpc_host.py
ROWS = [("two_dof_sea", "SolverDDP", 16, 40, 0),
        ("two_dof_sea", "SolverFDDP", 16, 40, 0)]
ROW_IDS = ["%s-%s" % r[:2] for r in ROWS]
PLANT_RANGE = 0.2   # plants within +-20 % of the trajectory's nominal K and B
PLANT_SEED = 11


def plant_phase(oracle, low, b, xs, us, K, hold, k=None, bm=None, w=None, clamp=False, row0=0):
    """The plant phase of one control step of trajectory b.  xs [T+1, nx], us [T, nu], K [T, nu, nx]: the plan and gains the
    solve left; k, bm: diagonals of the plant's K and B (None: the trajectory's own); w [hold, nx]: the disturbance of the
    applied knots or None; row0: how many rows the window has advanced beyond the path's own first row (the step's first
    applied knot).  -> dict(x [hold+1, nx], u [hold, nu], cost: sum of the running costs in knot order, failed: the first j
    whose xnext is bad or -1, bound: the clamp moved some control)"""
    lb = pol.plant_problem(low, b, k, bm)
    mi = int(low.node_model[0])
    m = lb.desc.models[mi]
    path = getattr(low, "ref_path", None)
    ref = lambda j: (path[0][_ref_path.row_of(row0 + j, path[1], path[0].shape[0]), b] if path is not None
                     else None if low.frame_ref is None else low.frame_ref[b])
    x = np.array(xs[0], dtype=np.float64)
    X, U = np.zeros((hold + 1, low.nx)), np.zeros((hold, low.nu))
    cost, failed, bound = 0.0, -1, False
    for j in range(hold):
        u = np.array(us[0]) if j == 0 else us[j] - K[j] @ (x - xs[j])
        if clamp and m.has_u_limits:
            uc = np.clip(u, np.array(m.u_lb[:low.nu]), np.array(m.u_ub[:low.nu]))
            bound = bound or bool((uc != u).any())
            u = uc
        X[j], U[j] = x, u
        kn = oracle.knot(lb, mi, x, u, frame_ref=ref(j), diff=False)
        cost = cost + kn["cost"]
        if failed < 0 and pol.bad(kn["xnext"]):
            failed = j
        x = kn["xnext"] if w is None else kn["xnext"] + w[j]
    X[hold] = x
    return dict(x=X, u=U, cost=cost, failed=failed, bound=bound)


def shifted(xs, us, hold, xplus):
    """xs [T+1, ...], us [T, ...] -> the plan moved down by hold rows, the last row repeated, xs[0] = xplus"""
    T = us.shape[0]
    xs2 = np.array(xs[np.minimum(np.arange(T + 1) + hold, T)])
    us2 = np.array(us[np.minimum(np.arange(T) + hold, T - 1)])
    xs2[0] = xplus
    return xs2, us2


def plants(low, seed=PLANT_SEED, rng_range=PLANT_RANGE, stiffness=True):
    """-> batch-major (K [B, nj] or None, B [B, nj]): the trajectories' nominal diagonals times U(1 - r, 1 + r)"""
    rng = np.random.default_rng(seed)
    kn = np.array([pol.nominal_diag(low, b, "K") for b in range(low.B)])
    bn = np.array([pol.nominal_diag(low, b, "B") for b in range(low.B)])
    pk = kn * rng.uniform(1.0 - rng_range, 1.0 + rng_range, kn.shape)
    pb = bn * rng.uniform(1.0 - rng_range, 1.0 + rng_range, bn.shape)
    return (pk if stiffness and low.dam == _abi.DAM_SEA else None), pb


def oracle_loop(oracle, low, sp, n_steps, first_maxiter, iters_per_step, pk=None, pb=None, disturbance=None, nthreads=8):
    """tests/test_mpc_host.oracle_mpc with the plant knot evaluated on trajectory b's own plant (pk[b], pb[b]; None: the
    model), hold = 1.  disturbance [n_steps, B, nx] or None -> the dict oracle_mpc returns, plus closed_cost [B]"""
    assert low.traj_params is None
    B, nx, nu = low.B, low.nx, low.nu
    x_closed, u_closed = np.zeros((n_steps + 1, B, nx)), np.zeros((n_steps, B, nu))
    iters, status = np.zeros((n_steps, B), dtype=np.int32), np.zeros((n_steps, B), dtype=np.int32)
    cost, stop, closed = np.zeros((n_steps, B)), np.zeros((n_steps, B)), np.zeros(B)
    x0_keep, maxiter_keep = low.x0.copy(), sp.maxiter
    xs = us = None
    zk = np.zeros((low.T, nu, nx))
    try:
        for s in range(n_steps):
            sp.maxiter = first_maxiter if s == 0 else iters_per_step
            r = oracle.solve(low, sp, xs=xs, us=us, nthreads=nthreads)
            xs, us = r["xs"], r["us"]
            x_closed[s], u_closed[s] = xs[0], us[0]
            iters[s], status[s] = r["traj_i"][_abi.TI_ITER], r["traj_i"][_abi.TI_STATUS]
            cost[s], stop[s] = r["traj_f"][_abi.TF_COST], r["traj_f"][_abi.TF_STOP]
            ph = [plant_phase(oracle, low, b, xs[:, b], us[:, b], zk, 1, None if pk is None else pk[b],
                              None if pb is None else pb[b], None if disturbance is None else disturbance[s:s + 1, b])
                  for b in range(B)]
            xp = np.stack([p["x"][1] for p in ph])
            closed = closed + np.array([p["cost"] for p in ph])
            xs, us = shifted(xs, us, 1, xp)
            low.x0[...] = xp
        x_closed[n_steps] = xp
    finally:
        low.x0[...] = x0_keep
        sp.maxiter = maxiter_keep
    return dict(x_closed=x_closed, u_closed=u_closed, iters=iters, status=status, cost=cost, stop=stop, xs=xs, us=us,
                closed_cost=closed)


_REFS = {}


def loop_reference(oracle, row, host):
    """the oracle loop of a row on its mismatched plants, computed once per session and shared (callers do not write to it);
    host: tests/test_mpc_host (its parity_case gives the scenario, the solver parameters and the disturbance)
    -> (reference dict, pk, pb)"""
    if row not in _REFS:
        from aslr_to_amd import scenarios
        sc, sp, dist = host.parity_case(*row)
        low = scenarios.lower(sc)
        pk, pb = plants(low)
        _REFS[row] = (oracle_loop(oracle, low, sp, host.N_STEPS, host.FIRST_MAXITER, host.ITERS_PER_STEP, pk, pb, dist), pk, pb)
    return _REFS[row]
