"""Receding-horizon runs on a mismatched plant (aslr_mpc_run_plant, include/aslr_to_amd_mpc_plant.h) on a CPU: the contract
of the extension header, the helpers of tests/_mpc_plant.py pinned on the oracle alone, and the conditioning of the rows the
GPU test of the whole loop uses (tests/test_gpu_mpc_plant.py)."""
import ctypes as C

import numpy as np
import pytest

import _mpc_plant as mp
import _policy as pol
import test_mpc_host as H
from aslr_to_amd import _abi, scenarios


def test_a_null_handle_is_refused_by_name():
    lib = _abi.load_library()
    assert lib.aslr_workspace_bytes(None) < 0     # some other message is in the buffer first
    assert lib.aslr_mpc_run_plant(None, None, None, 1, None, None, 0, None, None, None) == _abi.E_INVALID
    msg = lib.aslr_last_error().decode()
    assert msg.startswith("aslr_mpc_run_plant:") and "handle" in msg, msg


def _plan(low, seed):
    """a seeded plan of one trajectory set: xs [T+1, B, nx], us [T, B, nu], K [T, B, nu, nx] (mild gains)"""
    rng = np.random.default_rng(seed)
    xs = rng.uniform(-0.5, 0.5, (low.T + 1, low.B, low.nx))
    us = rng.uniform(-1.0, 1.0, (low.T, low.B, low.nu))
    if low.dam == _abi.DAM_VSA:
        us[..., low.nu // 2:] = rng.uniform(0.5, 4.0, (low.T, low.B, low.nu // 2))
    K = rng.uniform(-0.1, 0.1, (low.T, low.B, low.nu, low.nx))
    return xs, us, K


def test_plant_phase_with_hold_one_is_the_knot_of_node_zero(oracle):
    """hold = 1, no plant, no disturbance: x[1] and the cost are oracle.knot of node 0 on (xs[0], us[0]), exactly, whatever
    the gains hold"""
    low = scenarios.lower(scenarios.two_dof_sea(B=3, T=4, seed=4))
    xs, us, K = _plan(low, 1)
    for b in range(low.B):
        got = mp.plant_phase(oracle, low, b, xs[:, b], us[:, b], np.full_like(K[:, b], np.nan), 1)
        kn = oracle.knot(low, int(low.node_model[0]), xs[0, b], us[0, b], low.frame_ref[b], diff=False)
        np.testing.assert_array_equal(got["x"][0], xs[0, b])
        np.testing.assert_array_equal(got["u"][0], us[0, b])
        np.testing.assert_array_equal(got["x"][1], kn["xnext"])
        assert got["cost"] == kn["cost"] and got["failed"] == -1


@pytest.mark.parametrize("name, clamp", [("two_dof_sea", False), ("two_dof_vsa_boxddp", True)])
def test_plant_phase_without_gains_is_the_open_loop_rollout(oracle, name, clamp):
    """K = 0: the states and controls of the first `hold` knots are those of tests/_policy.rollout_one from xs[0] -- on a
    plant, with a disturbance, with the (narrowed) box -- exactly"""
    sc = pol.scenario(name, 3, 5, name == "two_dof_vsa_boxddp", False)
    low = scenarios.lower(sc)
    xs, us, _ = _plan(low, 2)
    zk = np.zeros((low.T, low.nu, low.nx))
    pk, pb = mp.plants(low, rng_range=0.3)
    w = np.random.default_rng(3).uniform(-1e-3, 1e-3, (low.T, low.B, low.nx))
    hold = 3
    for b in range(low.B):
        k = None if pk is None else pk[b]
        got = mp.plant_phase(oracle, low, b, xs[:, b], us[:, b], zk, hold, k, pb[b], w[:hold, b], clamp)
        want = pol.rollout_one(oracle, low, b, xs[:, b], us[:, b], zk, k, pb[b], None, w[:, b], clamp, x0=xs[0, b])
        np.testing.assert_array_equal(got["x"], want["xs"][:hold + 1])
        np.testing.assert_array_equal(got["u"], want["us"][:hold])
        assert got["failed"] == -1 and np.isfinite(got["cost"])
    if clamp:
        assert (np.abs(us[:3, :, :2]) > pol.BOX_UB[0]).any()   # (seeded torques leave the narrowed box: the clamp was at work)


def test_shifted_with_hold_one_is_the_concatenation_of_the_oracle_loop():
    rng = np.random.default_rng(0)
    xs, us, xp = rng.uniform(-1, 1, (6, 3, 8)), rng.uniform(-1, 1, (5, 3, 2)), rng.uniform(-1, 1, (3, 8))
    xs1, us1 = np.concatenate([xs[1:], xs[-1:]]), np.concatenate([us[1:], us[-1:]])
    xs1[0] = xp
    got = mp.shifted(xs, us, 1, xp)
    np.testing.assert_array_equal(got[0], xs1)
    np.testing.assert_array_equal(got[1], us1)
    # ... and by the whole horizon: every row but xs[0] is the last one
    gx, gu = mp.shifted(xs, us, 5, xp)
    np.testing.assert_array_equal(gx[1:], np.repeat(xs[-1:], 5, axis=0))
    np.testing.assert_array_equal(gu, np.repeat(us[-1:], 5, axis=0))
    np.testing.assert_array_equal(gx[0], xp)


@pytest.mark.parametrize("row", mp.ROWS, ids=mp.ROW_IDS)
def test_oracle_loop_rows_are_stable(oracle, row):
    """The criterion of test_mpc_host.test_oracle_loop_is_stable_on_the_parity_rows for the loop on a mismatched plant
    (oracle.solve + the plant's knot + shift; hold = 1 reads no gains): step 0 converges on every trajectory, a 1e-14
    relative perturbation of x0 moves no iteration count and the closed-loop states by less than 1e-8 -- and the plant is
    not the model: it moves x_closed by more than 1e-6 against the nominal loop.

    Plants: mp.PLANT_RANGE = +-20 % of the nominal K and B from default_rng(11), the range tried first; both rows hold the
    criterion at it, so nothing was halved and no row rejected (the figures are printed)."""
    ref, pk, pb = mp.loop_reference(oracle, row, H)
    assert ((ref["status"][0] & _abi.ST_CONVERGED) != 0).all(), ref["status"][0]
    sc, sp, dist = H.parity_case(*row)
    sc["x0"] = sc["x0"] * (1.0 + 1e-14)
    per = mp.oracle_loop(oracle, scenarios.lower(sc), sp, H.N_STEPS, H.FIRST_MAXITER, H.ITERS_PER_STEP, pk, pb, dist)
    np.testing.assert_array_equal(per["iters"], ref["iters"])
    dx = np.abs(per["x_closed"] - ref["x_closed"]).max()
    nominal = H.parity_reference(oracle, row)
    moved = np.abs(nominal["x_closed"] - ref["x_closed"]).max()
    print("%s %s: iterations per step %s, closed-loop states move by %.1e under the perturbation, by %.1e under the plant"
          % (row[0], row[1], [(int(a), int(b)) for a, b in zip(ref["iters"].min(axis=1), ref["iters"].max(axis=1))], dx, moved))
    assert dx < 1e-8
    assert moved > 1e-6


def test_oracle_loop_on_the_model_is_the_oracle_loop_of_the_mpc_suite(oracle):
    """pins the helper: without plants it is tests/test_mpc_host.oracle_mpc, exactly; its closed cost is the sum of the
    knot costs of the applied controls"""
    sc = scenarios.two_dof_sea(B=3, T=4)
    low, sp = scenarios.lower(sc), scenarios.solver_params(sc, solver="SolverFDDP", maxiter=77)
    dist = np.random.default_rng(0).uniform(-1e-3, 1e-3, (2, 3, 8))
    got = mp.oracle_loop(oracle, low, sp, 2, 5, 2, None, None, dist)
    want = H.oracle_mpc(oracle, low, sp, 2, 5, 2, dist)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert sp.maxiter == 77
    c = sum(np.array([oracle.knot(low, 0, want["x_closed"][s, b], want["u_closed"][s, b], low.frame_ref[b], diff=False)["cost"]
                      for b in range(3)]) for s in range(2))
    np.testing.assert_allclose(got["closed_cost"], c, rtol=1e-15)
