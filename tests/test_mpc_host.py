"""Receding-horizon runs (aslr_mpc_run), host side: the ABI's self-description, and the reference loop the GPU tests compare
against -- composed from the unchanged oracle -- with the criterion by which its cases were chosen."""
import ctypes as C

import numpy as np
import pytest

from aslr_to_amd import _abi, scenarios


def oracle_mpc(oracle, low, sp, n_steps, first_maxiter, iters_per_step, disturbance=None, xs=None, us=None, nthreads=8):
    """The closed loop, step by step on the CPU: oracle.solve with the step's maxiter (step 0 from xs / us, None: the empty
    candidate), the first running model's oracle.knot on (xs[0], us[0]) plus disturbance[s], a numpy shift, low.x0
    written in place (put back on return; sp.maxiter likewise).  disturbance: [n_steps, B, nx] or None.
    -> dict of time-major arrays: x_closed [n+1, B, nx], u_closed [n, B, nu], iters / status [n, B] (int32), cost, stop
    [n, B], and the last shifted plan xs [T+1, B, nx], us [T, B, nu]."""
    assert low.traj_params is None  # (the oracle knows the models' constants only)
    B, nx, nu = low.B, low.nx, low.nu
    mi = int(low.node_model[0])
    x_closed, u_closed = np.zeros((n_steps + 1, B, nx)), np.zeros((n_steps, B, nu))
    iters, status = np.zeros((n_steps, B), dtype=np.int32), np.zeros((n_steps, B), dtype=np.int32)
    cost, stop = np.zeros((n_steps, B)), np.zeros((n_steps, B))
    x0_keep, maxiter_keep = low.x0.copy(), sp.maxiter
    try:
        for s in range(n_steps):
            sp.maxiter = first_maxiter if s == 0 else iters_per_step
            r = oracle.solve(low, sp, xs=xs, us=us, nthreads=nthreads)
            xs, us = r["xs"], r["us"]
            x_closed[s], u_closed[s] = xs[0], us[0]
            iters[s], status[s] = r["traj_i"][_abi.TI_ITER], r["traj_i"][_abi.TI_STATUS]
            cost[s], stop[s] = r["traj_f"][_abi.TF_COST], r["traj_f"][_abi.TF_STOP]
            xp = np.stack([oracle.knot(low, mi, xs[0, b], us[0, b], None if low.frame_ref is None else low.frame_ref[b],
                                       diff=False)["xnext"] for b in range(B)])
            if disturbance is not None:
                xp = xp + disturbance[s]
            xs, us = np.concatenate([xs[1:], xs[-1:]]), np.concatenate([us[1:], us[-1:]])
            xs[0] = xp
            low.x0[...] = xp
        x_closed[n_steps] = xp
    finally:
        low.x0[...] = x0_keep
        sp.maxiter = maxiter_keep
    return dict(x_closed=x_closed, u_closed=u_closed, iters=iters, status=status, cost=cost, stop=stop, xs=xs, us=us)


# The oracle-parity rows of tests/test_gpu_mpc.py: (scenario, solver, B, T, scenario seed).  n_steps = 5, first_maxiter =
# 100, iters_per_step = 3, disturbance U(-1e-3, 1e-3) on every state entry from default_rng(7).  Chosen by
# test_oracle_loop_is_stable_on_the_parity_rows below, on the oracle alone.
# Rejected there: two_dof_vsa_boxddp with SolverBoxDDP at B = 16, T = 40, seed 0.  (1) Step 0 converges on 10 of 16
# trajectories within 100 iterations; no seed in 0..11 at T = 40, 30 or 20 and none in 0..79 at T = 20 brings all 16 there
# (3 - 15 of 16: this cost stack needs up to 400 BoxDDP iterations).  (2) Where step 0 does converge on all 16 -- T = 6 ..
# 15, ten seeds out of 80 each -- the closed loop itself is not reproducible on the oracle: three iterations per step do not
# hold this plant (motor inertia 1e-3 under explicit Euler steps of 1e-2 with stiffness commands up to 100), |x| reaches
# 1e2 .. 1e3 within five steps and the 1e-14 perturbation of x0 moves the closed-loop states by 1e0 .. 1e3 from step 3 on,
# whatever the disturbance scale (1e-3 .. 1e-8 tried).  The loop stays reproducible for five steps only at very short
# horizons: of the seeds 16..399 one passes at T = 3 (217, used below) and five at T = 2.
N_STEPS, FIRST_MAXITER, ITERS_PER_STEP = 5, 100, 3
ROWS = [("two_dof_sea", "SolverDDP", 16, 40, 0),
        ("two_dof_sea", "SolverFDDP", 16, 40, 0),
        ("two_dof_vsa_boxddp", "SolverBoxDDP", 16, 3, 217),
        ("talos_arm_sea", "SolverFDDP", 4, 20, 0),
        ("talos_arm_vsa", "SolverBoxDDP", 4, 20, 0)]
ROW_IDS = ["%s-%s" % r[:2] for r in ROWS]


def parity_case(name, solver, B, T, seed):
    """-> scenario, solver parameters, disturbance [N_STEPS, B, nx]"""
    sc = scenarios.SCENARIOS[name](B=B, T=T, seed=seed)
    sp = scenarios.solver_params(sc, solver=solver)
    nx = np.atleast_2d(sc["x0"]).shape[1]
    return sc, sp, np.random.default_rng(7).uniform(-1e-3, 1e-3, (N_STEPS, B, nx))


_REFS = {}


def parity_reference(oracle, row):
    """the oracle loop of a row, computed once per session and shared (callers do not write to it)"""
    if row not in _REFS:
        sc, sp, dist = parity_case(*row)
        _REFS[row] = oracle_mpc(oracle, scenarios.lower(sc), sp, N_STEPS, FIRST_MAXITER, ITERS_PER_STEP, dist)
    return _REFS[row]


@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_oracle_loop_is_stable_on_the_parity_rows(oracle, row):
    """The project's rule for full-solve parity cases, on the oracle alone: step 0 converges on every
    trajectory, and a 1e-14 relative perturbation of x0 moves none of the iteration counts of any step and the closed-loop
    states by less than 1e-8, 100 times below the bound the GPU is held to."""
    ref = parity_reference(oracle, row)
    assert ((ref["status"][0] & _abi.ST_CONVERGED) != 0).all(), ref["status"][0]
    sc, sp, dist = parity_case(*row)
    sc["x0"] = sc["x0"] * (1.0 + 1e-14)
    per = oracle_mpc(oracle, scenarios.lower(sc), sp, N_STEPS, FIRST_MAXITER, ITERS_PER_STEP, dist)
    np.testing.assert_array_equal(per["iters"], ref["iters"])
    dx = np.abs(per["x_closed"] - ref["x_closed"]).max()
    print("%s %s: iterations per step %s, closed-loop states move by %.1e"
          % (row[0], row[1], [(int(a), int(b)) for a, b in zip(ref["iters"].min(axis=1), ref["iters"].max(axis=1))], dx))
    assert dx < 1e-8


def test_oracle_loop_is_the_composition_it_claims(oracle):
    """Pins the helper: one step of it is oracle.solve, the knot of the first node and a shift; low.x0 and sp.maxiter
    are left as they were."""
    sc = scenarios.two_dof_sea(B=3, T=4)
    low, sp = scenarios.lower(sc), scenarios.solver_params(sc, solver="SolverFDDP", maxiter=77)
    x0 = low.x0.copy()
    dist = np.random.default_rng(0).uniform(-1e-3, 1e-3, (2, 3, 8))
    got = oracle_mpc(oracle, low, sp, 2, 5, 2, dist)
    np.testing.assert_array_equal(low.x0, x0)
    assert sp.maxiter == 77
    first = oracle.solve(low, scenarios.solver_params(sc, solver="SolverFDDP", maxiter=5))
    np.testing.assert_array_equal(got["x_closed"][0], first["xs"][0])
    np.testing.assert_array_equal(got["u_closed"][0], first["us"][0])
    np.testing.assert_array_equal(got["iters"][0], first["traj_i"][_abi.TI_ITER])
    xp = np.stack([oracle.knot(low, 0, first["xs"][0, b], first["us"][0, b], low.frame_ref[b], diff=False)["xnext"]
                   for b in range(3)]) + dist[0]
    np.testing.assert_array_equal(got["x_closed"][1], xp)
    assert (got["iters"][1] <= 2).all()
    np.testing.assert_array_equal(got["xs"][-1], got["xs"][-2])   # the terminal state is repeated by every shift
    np.testing.assert_array_equal(got["x_closed"][2], got["xs"][0])


def test_symbol_struct_and_version_are_declared():
    assert "aslr_mpc_run" in _abi.EXPORTED_SYMBOLS
    assert C.sizeof(_abi.Mpc) == 4 * 4 + 5 * C.sizeof(C.c_void_p)
    header = open(__file__.rsplit("/tests/", 1)[0] + "/include/aslr_to_amd.h").read()
    for word in ("aslr_mpc_run", "aslr_mpc_t", "8 mpc"):
        assert word in header, word
    assert "#define ASLR_ABI_VERSION %d" % _abi.ABI_VERSION in header
    assert _abi.R_TRAJ_PARAMS == _abi.R_COUNT - 1   # no workspace region was added for it


def test_library_exports_the_entry_point_and_declines_null():
    """aslr_sizeof(8), the ABI version, and the decline that needs no handle (and so no GPU)."""
    lib = _abi.load_library()
    assert hasattr(lib, "aslr_mpc_run")
    assert lib.aslr_sizeof(8) == C.sizeof(_abi.Mpc)
    assert lib.aslr_abi_version() == _abi.ABI_VERSION
    assert lib.aslr_mpc_run(None, None, None, None) == _abi.E_INVALID
    assert b"aslr_mpc_run: NULL argument" in lib.aslr_last_error()
