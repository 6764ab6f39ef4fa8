"""Receding-horizon runs on a mismatched plant for every model size (aslr_mpc_run_plant_all,
include/aslr_to_amd_mpc_plant_all.h) on a CPU: the contract of the extension header, and the conditioning of the 7-joint
rows and one-step cases the GPU tests use (tests/_mpc_plant_team.py, tests/test_gpu_mpc_plant_team.py) on the oracle alone,
with the reference of tests/_mpc_plant.py as it stands."""
import ctypes as C

import numpy as np
import pytest

import _mpc_plant as mp
import _mpc_plant_team as mt
import _policy as pol
import test_mpc_host as H
from aslr_to_amd import _abi, scenarios


def test_a_null_handle_is_refused_by_name():
    lib = _abi.load_library()
    assert lib.aslr_workspace_bytes(None) < 0     # some other message is in the buffer first
    assert lib.aslr_mpc_run_plant_all(None, None, None, 1, None, None, 0, None, None, None) == _abi.E_INVALID
    msg = lib.aslr_last_error().decode()
    assert msg.startswith("aslr_mpc_run_plant_all:") and "handle" in msg, msg


@pytest.mark.parametrize("row", mt.ROWS, ids=mt.ROW_IDS)
def test_oracle_loop_rows_are_stable(oracle, row):
    """The criterion of test_mpc_plant_host.test_oracle_loop_rows_are_stable on the two arm rows of test_mpc_host.ROWS: step
    0 converges on every trajectory, a 1e-14 relative perturbation of x0 moves no iteration count and the closed-loop states
    by less than 1e-8 -- and the plant is not the model: it moves x_closed by more than 1e-6 against the nominal loop.

    Plants: mp.plants(low), +-20 % of the nominal K and B from default_rng(11), the range tried first; both rows hold the
    criterion at it, so nothing was halved and no row rejected (the figures are printed)."""
    assert row in H.ROWS
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


@pytest.mark.parametrize("key", sorted(mt.ONE_STEP))
def test_the_one_step_cases_are_well_conditioned(oracle, key):
    """On the oracle alone, with the plan of oracle.solve after three iterations and the gains of pol.oracle_gains at that
    plan: no knot fails; over the `hold` applied knots the closed loop leaves the plan by more than 1e-3; the gains moved by
    1e-13 relative (seeded signs) move every output of mp.plant_phase by less than 1e-10 in the measure of the GPU tests,
    max |a - b| / (1 + |b|) -- an amplification below 1e3, which is what makes 1e-9 there a statement about the kernel and
    not about the inputs.  vsa_box: the narrowed box of _policy_team.box(7) binds on some trajectory and not on all, and
    the clamped controls differ from the free ones by more than 1e-3.

    Every case holds its conditions at the ranges tried first (plants +-30 %, disturbance 1e-3, scenario seed 4): nothing
    was halved; the figures are printed.  vsa_box runs T = 6, hold = 6, where the box also binds under the DEVICE's
    BoxDDP gains (tests/_mpc_plant_team.py records that search)."""
    c = mt.one_step(key)
    low, sp, hold = c["low"], c["sp"], c["hold"]
    r = oracle.solve(low, sp)
    X, U = r["xs"], r["us"]
    K = pol.oracle_gains(oracle, low, sp, X, U)
    base = mt.reference(oracle, c, X, U, K)
    assert (base["failed"] == -1).all() and np.isfinite(base["cost"]).all()
    left = np.abs(base["x"][1:] - X[1:hold + 1]).max()
    print("%s: the closed loop leaves the plan by %.2e" % (key, left))
    assert left > 1e-3
    rng = np.random.default_rng(23)
    K2 = K * (1.0 + 1e-13 * rng.choice([-1.0, 1.0], K.shape))
    moved = mt.reference(oracle, c, X, U, K2)
    worst = max(pol.relerr(moved[k], base[k]) for k in ("x", "u", "cost"))
    print("%s: worst movement %.2e" % (key, worst))
    assert worst < 1e-10, worst
    np.testing.assert_array_equal(moved["failed"], base["failed"])
    if c["clamp"]:
        print("%s: the box binds on %d of %d trajectories" % (key, base["bound"].sum(), base["bound"].size))
        assert base["bound"].any() and not base["bound"].all()
        free = mt.reference(oracle, c, X, U, K, clamp=False)
        diff = pol.relerr(free["u"], base["u"])
        print("%s: clamped against free controls %.2e" % (key, diff))
        assert diff > 1e-3
