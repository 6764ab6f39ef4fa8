"""Output-feedback covariance (aslr_policy_lqg, include/aslr_to_amd_lqg.h) on a CPU: the reference of tests/_lqg.py pinned on
the oracle alone -- against the directly propagated covariance of [error; estimate], against the optimality of its gains, in
its two limits (tests/_covariance.propagate with the gains and with K = 0) -- and the conditioning of the inputs the GPU
cases use (tests/test_gpu_lqg.py)."""
import ctypes as C

import numpy as np
import pytest

import _covariance as cv
import _lqg as lq
import _policy as pol
from aslr_to_amd import _abi

_made = {}


def _case(oracle, key):
    """the case of tests/_covariance.case with its records and the oracle's gains of one backward sweep, built once"""
    if key not in _made:
        c = cv.case(oracle, key)
        c["deriv"] = cv.records(oracle, c["low"], c["xs"], c["us"])
        c["K"] = pol.oracle_gains(oracle, c["low"], c["sp"], c["xs"], c["us"])
        _made[key] = c
    return _made[key]


def test_a_null_handle_is_refused_by_name():
    lib = _abi.load_library()
    assert lib.aslr_workspace_bytes(None) < 0     # some other message is in the buffer first
    buf = C.cast((C.c_double * 64)(), C.c_void_p)   # stands where a device pointer goes; never dereferenced
    assert lib.aslr_policy_lqg(None, 4, None, buf, buf, buf, buf, buf, buf, buf, buf, buf, buf, None) == _abi.E_INVALID
    msg = lib.aslr_last_error().decode()
    assert msg.startswith("aslr_policy_lqg:") and "handle" in msg, msg


@pytest.mark.parametrize("which", lq.SETS)
@pytest.mark.parametrize("key", ["sea", "vsa_box", "arm_sea"])
def test_separation_the_recursion_is_the_covariance_of_error_and_estimate(oracle, key, which):
    """Sigma_t, U_t and cost_increase of the helper against the 2 nx x 2 nx covariance of [e; eh] propagated with the helper's
    L_t (tests/_lqg.augmented: (I - L C) and L R L^T written out, E[eh e^T] read off the big matrix, no orthogonality used).

    Bound 1e-10 in traj_relerr: the two sides are equal in exact arithmetic and are float64 evaluations in different orders;
    the conditioning test below bounds the amplification of a relative 1e-13 by 100, and the thousand or so roundings of
    1.1e-16 behind an entry (T nx^2 products), amplified alike, stay near 1e-11.  Measured: 3.2e-12 at the worst."""
    c = _case(oracle, key)
    low = c["low"]
    m = lq.measured(low.nx, which)
    r = lq.meas_var(low.B, len(m), key)
    for combo in cv.COMBOS:
        s0, w = cv.combo(c, combo)
        got = lq.propagate(low, c["deriv"], c["K"], m, r, s0, w)
        want = lq.augmented(low, c["deriv"], c["K"], m, r, got["kalman_gain"], s0, w)
        for k in ("Sigma", "U", "cost_increase"):
            err = cv.traj_relerr(got[k], want[k])
            print("%s %s %s %s: %.2e" % (key, which, combo, k, err))
            assert err < 1e-10, (k, err)
        # ... and P is the covariance of e - eh, which the big matrix gives as a difference of blocks the size of Sigma
        assert cv.traj_relerr(got["Sigma"] + got["P"] - want["err"], got["Sigma"]) < 1e-10
        assert np.abs(want["U"]).max() > 1e-6 and np.abs(want["cost_increase"]).min() > 1e-6


@pytest.mark.parametrize("key", ["sea", "arm_sea"])
def test_optimality_no_other_gain_estimates_better(oracle, key):
    """one entry of one L_t (the largest of the knot) moved by +-1e-3 of its size, in the augmented recursion: tr P_t of that
    knot does not go down.  (It goes up by delta^2 S[a][a], about 1e-6 L^2 S: far above the rounding of a trace of order 1.)"""
    c = _case(oracle, key)
    low = c["low"]
    for which in lq.SETS:
        m = lq.measured(low.nx, which)
        r = lq.meas_var(low.B, len(m), key)
        base = lq.propagate(low, c["deriv"], c["K"], m, r, c["sigma0"], c["noise_var"])
        L = base["kalman_gain"]
        ref = lq.augmented(low, c["deriv"], c["K"], m, r, L, c["sigma0"], c["noise_var"])["err"]
        for t in (0, low.T // 2, low.T):
            j, a = np.unravel_index(np.abs(L[:, t]).reshape(low.B, -1).argmax(axis=1), L.shape[2:])
            for sign in (-1.0, 1.0):
                moved = np.array(L)
                moved[np.arange(low.B), t, j, a] *= 1.0 + sign * 1e-3
                err = lq.augmented(low, c["deriv"], c["K"], m, r, moved, c["sigma0"], c["noise_var"])["err"]
                for b in range(low.B):
                    assert np.trace(err[b, t]) > np.trace(ref[b, t]), (which, t, b, sign)


@pytest.mark.parametrize("key", ["sea", "nu1", "arm_sea"])
def test_full_information_limit_is_the_state_feedback_covariance(oracle, key):
    """every entry measured (a permutation) with meas_var = 1e-12: x_var, u_var, cov_final and cost_increase of
    tests/_covariance.propagate within 1e-9.  The gap is O(meas_var / lambda_min(Pm)), and lambda_min >= 0.1 with cv.inputs.
    One case per record size with nx = 8, nu = 2, a padded control, and nx = 28.  The VSA cases are left to the other limit:
    their Pm reaches 1e5, where the rounding of P = Pm - D (1e-11 absolute) is above this meas_var and S loses definiteness."""
    c = _case(oracle, key)
    low = c["low"]
    m = lq.measured(low.nx, "all")
    r = np.full((low.B, low.nx), 1e-12)
    for combo in cv.COMBOS:
        s0, w = cv.combo(c, combo)
        got = lq.propagate(low, c["deriv"], c["K"], m, r, s0, w)
        want = cv.propagate(low, c["deriv"], c["K"], s0, w)
        for k in ("x_var", "u_var", "cov_final", "cost_increase"):
            err = cv.traj_relerr(got[k], want[k])
            print("%s %s %s: %.2e" % (key, combo, k, err))
            assert err < 1e-9, (k, err)


@pytest.mark.parametrize("key", ["sea", "vsa_box", "arm_vsa"])
def test_no_information_limit_is_the_open_loop_covariance(oracle, key):
    """meas_var = 1e14 lambda_max over the knots of the open-loop covariance, which dominates every Pm_t (so
    lambda_max(Pm_t) / meas_var <= 1e-14 < 1e-11 at every t): Sigma_t is tests/_covariance.propagate with K = 0 within 1e-9,
    and u_var is below 1e-9 of diag(K Sigma K^T)"""
    c = _case(oracle, key)
    low = c["low"]
    m = lq.measured(low.nx, "default")
    zero = np.zeros_like(c["K"])
    for combo in cv.COMBOS:
        s0, w = cv.combo(c, combo)
        open_loop = cv.propagate(low, c["deriv"], zero, s0, w)
        r = np.full((low.B, len(m)), 1e14 * np.linalg.eigvalsh(open_loop["cov"]).max())
        got = lq.propagate(low, c["deriv"], c["K"], m, r, s0, w)
        assert (np.linalg.eigvalsh(got["Pm"]).max(axis=(1, 2)) / r[:, 0] < 1e-11).all()
        assert cv.traj_relerr(got["Sigma"], open_loop["cov"]) < 1e-9
        ref = np.einsum("tbki,btij,tbkj->btk", c["K"], open_loop["cov"][:, :low.T], c["K"])
        assert ref.max() > 1e-6 and (got["u_var"] <= 1e-9 * ref).all()


@pytest.mark.parametrize("key", ["sea", "arm_vsa"])
def test_the_filter_does_not_depend_on_the_gains(oracle, key):
    c = _case(oracle, key)
    low = c["low"]
    for which in lq.SETS:
        m = lq.measured(low.nx, which)
        r = lq.meas_var(low.B, len(m), key)
        a = lq.propagate(low, c["deriv"], c["K"], m, r, c["sigma0"], c["noise_var"])
        z = lq.propagate(low, c["deriv"], np.zeros_like(c["K"]), m, r, c["sigma0"], c["noise_var"])
        for k in ("est_var", "est_cov_final", "kalman_gain"):
            np.testing.assert_array_equal(a[k], z[k], err_msg=k)
        assert cv.traj_relerr(a["x_var"], z["x_var"]) > 1e-3


@pytest.mark.parametrize("key", sorted(cv.CASES))
def test_the_gpu_cases_are_well_conditioned(oracle, key):
    """x0, K and meas_var moved by 1e-13 relative (seeded signs; the candidate is rolled out again from the moved x0): every
    output of the helper, for every measured set and each of the three input combinations, must move by less than 1e-11 in
    the measure of the GPU tests, so that 1e-9 there is a statement about the kernel; and every P_t of the helper is positive
    definite.  A condition on the choice of inputs.

    What was chosen: the cases, sigma0 and noise_var of tests/_covariance.py as they are and meas_var ~ U(0.1, 1)
    (tests/_lqg.meas_var).  Two cases failed with that and had their inputs changed, not the bound: vsa_box moved by 8.7e-11
    and arm_vsa by 1.1e-11 (est_cov_final, sets `odd` and `all`), because their states spread to variances of 1e5 and a
    measurement of variance 1 makes P = Pm - D a difference of five cancelled digits.  Their meas_var is scaled by 1e4
    (tests/_lqg.MEAS_SCALE).  Measured movement after that, worst output, set and combination: arm_sea 2.4e-12,
    arm_vsa 9.4e-13, nu1 5.7e-13, sea 2.7e-12, sea_one 6.0e-13, sea_path 2.7e-12, vsa_box 2.9e-12."""
    c = _case(oracle, key)
    low = c["low"]
    rng = np.random.default_rng(23)
    K2 = c["K"] * (1.0 + 1e-13 * rng.choice([-1.0, 1.0], c["K"].shape))
    x0 = np.array(low.x0)
    xs2, us2 = cv.candidate(oracle, low, x0=x0 * (1.0 + 1e-13 * rng.choice([-1.0, 1.0], x0.shape)))
    assert (us2 == c["us"]).all()
    deriv2 = cv.records(oracle, low, xs2, us2)
    worst, least = 0.0, np.inf
    for which in lq.SETS:
        m = lq.measured(low.nx, which)
        r = lq.meas_var(low.B, len(m), key)
        r2 = r * (1.0 + 1e-13 * rng.choice([-1.0, 1.0], r.shape))
        for combo in cv.COMBOS:
            s0, w = cv.combo(c, combo)
            base = lq.propagate(low, c["deriv"], c["K"], m, r, s0, w)
            moved = lq.propagate(low, deriv2, K2, m, r2, s0, w)
            assert all(np.isfinite(base[k]).all() for k in lq.OUTPUTS)
            worst = max([worst] + [cv.traj_relerr(moved[k], base[k]) for k in lq.OUTPUTS])
            # (without sigma0 Pm_0 = 0 and P_0 = 0 exactly: knot 0 is left out there)
            least = min(least, np.linalg.eigvalsh(base["P"][:, 0 if s0 is not None else 1:]).min())
    print("%s: worst movement %.2e; smallest eigenvalue of a P_t %.2e" % (key, worst, least))
    assert worst < 1e-11, worst
    assert least > 0.0, least
