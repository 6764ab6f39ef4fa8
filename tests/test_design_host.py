"""aslr_design_descent (include/aslr_to_amd_design.h) on a CPU: the contract of the extension header, and the step rule of
tests/_design.py in a loop on the CPU oracle alone -- the properties a descent must have, and the conditioning of the cases
the GPU tests reuse (tests/test_gpu_design.py): every case accepts and rejects, no Armijo decision within rounding."""
import ctypes as C

import numpy as np
import pytest

import _design as D
from aslr_to_amd import _abi


def test_a_null_handle_is_refused_by_name():
    lib = _abi.load_library()
    assert lib.aslr_workspace_bytes(None) < 0     # some other message is in the buffer first
    sp, d = _abi.default_solver_params(), _abi.Design()
    assert lib.aslr_design_descent(None, C.byref(sp), C.byref(d), None) == _abi.E_INVALID
    msg = lib.aslr_last_error().decode()
    assert msg.startswith("aslr_design_descent:") and "handle" in msg, msg


def test_the_step_rule_restates_the_formulas():
    """candidate() on hand-made numbers: the relative clamp, the bounds, and a NaN passing through"""
    th, lo, hi = np.array([2.0, 2.0, 2.0, 2.0, 2.0]), np.full(5, 0.5), np.full(5, 2.5)
    g = np.array([0.1, -0.1, 10.0, -10.0, np.nan])
    got = D.candidate(th, g, 0.5, 0.25, lo, hi)
    np.testing.assert_array_equal(got[:4], [2.0 * (1.0 - 0.1), 2.0 * (1.0 + 0.1), 1.5, 2.5])
    assert np.isnan(got[4])


@pytest.fixture(scope="module")
def runs(oracle):
    """name -> (case, the oracle loop on it); built on first use, shared, never changed"""
    made = {}

    def get(name):
        if name not in made:
            c = D.case(name)
            low = c["low"]
            made[name] = (c, D.run(D.OracleBackend(oracle, c["sc"], c["sp"]), c["theta0"], np.zeros((low.T + 1, low.B, low.nx)),
                                   np.zeros((low.T, low.B, low.nu)), c["active"], c["lo"], c["hi"], c["n_steps"],
                                   c["first_maxiter"], c["iters_per_step"], eta0=c["eta0"], max_rel=c["max_rel"]))
        return made[name]
    return get


@pytest.mark.parametrize("name", D.ORACLE_CASES)
def test_the_oracle_loop_descends_inside_the_bounds(runs, name):
    c, r = runs(name)
    flag, J = r["flag"], r["hist_f"][:, 0]
    print("%s: flags %s" % (name, flag.T.tolist()))
    assert (flag[0] == 1).all()
    assert (flag[1:] == 1).any(), "no step after s = 0 is accepted"
    assert (flag == 0).any(), "no step is rejected: eta0 does not overshoot"
    act = c["active"]
    for s in range(c["n_steps"]):
        th_before, J_before, xs_before = r["log"][s]
        th_after, J_after, xs_after = r["log"][s + 1] if s + 1 < c["n_steps"] else (r["state"]["theta"], r["state"]["cost"], r["state"]["xs_best"])
        acc = flag[s] == 1
        if s > 0:   # accepted costs never increase; a rejected step leaves theta_acc, J_acc and xs_best untouched
            assert (J_after[acc] <= J_before[acc]).all()
            np.testing.assert_array_equal(J_after[acc], J[s][acc])
            np.testing.assert_array_equal(th_after[:, ~acc], th_before[:, ~acc])
            np.testing.assert_array_equal(J_after[~acc], J_before[~acc])
            np.testing.assert_array_equal(xs_after[:, ~acc], xs_before[:, ~acc])
        cand = r["theta_hist"][s]
        assert (cand[act] >= c["lo"][act]).all() and (cand[act] <= c["hi"][act]).all()
        np.testing.assert_array_equal(cand[~act], c["theta0"][~act])
        np.testing.assert_array_equal(th_after[:, acc], cand[:, acc])
    # after the last step XS holds the best plan and the table the accepted design
    np.testing.assert_array_equal(r["xs"], r["state"]["xs_best"])
    nj = c["low"].nj
    want = np.concatenate([r["state"]["theta"][:nj], 1.0 / r["state"]["theta"][nj:]])
    np.testing.assert_array_equal(r["table"][act], want[act])
    assert (r["state"]["cost"] < J[0]).any()


@pytest.mark.parametrize("name", D.ORACLE_CASES)
def test_no_armijo_decision_is_within_rounding(runs, name):
    c, r = runs(name)
    J_acc = np.stack([l[1] for l in r["log"]])
    rel = r["margin"][1:] / np.abs(J_acc[1:])
    print("%s: smallest Armijo margin %.2e |J_acc|" % (name, np.nanmin(rel)))
    assert not np.isnan(rel).any()
    assert np.nanmin(rel) > D.MARGIN
