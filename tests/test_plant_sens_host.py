"""Closed-loop plant sensitivity (aslr_policy_plant_sensitivity, include/aslr_to_amd_plant_sens.h) on a CPU: the contract of
the extension header, the reference of tests/_plant_sens.py pinned on the oracle alone -- against central differences of the
nonlinear closed loop of tests/_policy.py on perturbed plants, and against the adjoint reference of tests/_sensitivity.py
where the loop is open -- and the conditioning of the inputs the GPU cases use (tests/test_gpu_plant_sens.py)."""
import ctypes as C

import numpy as np
import pytest

import _covariance as cv
import _plant_sens as ps
import _policy as pol
import _sensitivity as sens
from aslr_to_amd import _abi


def test_a_null_handle_is_refused_by_name():
    lib = _abi.load_library()
    assert lib.aslr_workspace_bytes(None) < 0     # some other message is in the buffer first
    buf = C.cast((C.c_double * 64)(), C.c_void_p)   # stands where a device pointer goes; never dereferenced
    assert lib.aslr_policy_plant_sensitivity(None, *([buf] * 10), None) == _abi.E_INVALID
    msg = lib.aslr_last_error().decode()
    assert msg.startswith("aslr_policy_plant_sensitivity:") and "handle" in msg, msg


@pytest.fixture(scope="module")
def cases(oracle):
    """key -> the seeded case of tests/_covariance.case with the oracle's gains of one backward sweep on it; built on first
    use, shared, never changed"""
    made = {}

    def get(key):
        if key not in made:
            c = cv.case(oracle, key)
            c["K"] = pol.oracle_gains(oracle, c["low"], c["sp"], c["xs"], c["us"])
            made[key] = c
        return made[key]
    return get


@pytest.mark.parametrize("halve", [False, True])
@pytest.mark.parametrize("key", sorted(ps.FD))
def test_the_definition_is_the_derivative_of_the_nonlinear_closed_loop(oracle, cases, key, halve):
    """S_T, V and dJ_cl/dtheta of the definition (closed forms of G_t included) against central differences of
    _policy.rollout_one with the oracle's gains, no clamp, on plants whose theta_p is theta_p (1 +- h), one parameter at a
    time, in the measure cv.traj_relerr; at the step h and at h / 2.

    Finite-difference error is not rounding error and has no a-priori bound, so steps and bounds were fixed as in
    tests/test_sensitivity_host.py and test_covariance_host.py: the disagreement measured on the oracle alone over a scan of
    steps, recorded in tests/_plant_sens.FD, ten times that value as the bound (the margin covers libm differences between
    machines).  A measurement against the oracle, not against the code under test.  Measured, worst output, per relative
    step 1e-3 / 1e-4 / 5e-5 / 1e-5 / 1e-6 / 1e-7:
      sea      2.6e-5 / 2.6e-7 / 6.4e-8 / 3.8e-8 / 3.4e-7 / 2.7e-6     (max |K| 479)
      vsa_box  4.3e-5 / 4.3e-7 / 1.1e-7 / 5.1e-9 / 1.1e-8 / 3.5e-7     (max |K| 350)
      arm_sea  2.5e-6 / 2.5e-8 / 1.0e-8 / 6.3e-8 / 4.4e-7 / 4.1e-6     (max |K| 123)
      arm_vsa  2.7e-6 / 2.7e-8 / 6.7e-9 / 5.2e-10 / 7.1e-9 / 4.8e-8    (max |K| 130)
    Truncation falls with h^2 down to about 1e-5, where the rounding of the cost difference takes over (dJ/dtheta is the
    worst output there).  The steps chosen, 1e-4 and 5e-5, lie where truncation still rules, so the recorded values do not
    hang on the last bits of a libm."""
    h, at_h, at_half = ps.FD[key]
    c = cases(key)
    assert np.abs(c["K"]).max() > 1e-3
    step, measured = (0.5 * h, at_half) if halve else (h, at_h)
    err = ps.fd_disagreement(oracle, c["low"], c["xs"], c["us"], c["K"], step)
    print("%s: disagreement %.2e at step %.1e (bound %.1e)" % (key, err, step, 10 * measured))
    assert err < 10 * measured, err


@pytest.mark.parametrize("key", sorted(ps.CASES))
def test_open_loop_cost_derivatives_are_the_adjoint_ones(oracle, cases, key):
    """K = 0: dJ_cl/dtheta of the definition (tangent sweep) against the adjoint reference of tests/_sensitivity.expected,
    which sums lambda_{t+1}^T dxnext_t/dtheta with the oracle's own differences of the step: 1e-11 in cv.traj_relerr, the
    measure of every other check of this call (per trajectory, max |a - b| / max |b|).  The two sweeps are dual, and the
    closed forms of G_t are the step's parameter derivatives.

    Why that measure: both sweeps add T nx terms of size |lambda| |G| (|lambda| up to 6.9e3 on arm_sea) that cancel to results
    of size 0.1 .. 160, so the rounding of either side scales with the largest term of the trajectory, not with each entry.
    Measured: worst case arm_sea, 4.5e-13 (entry by entry as |a - b| / (1 + |b|) it is 1.6e-11, on an entry of size 0.5 next
    to one of 163)."""
    c = cases(key)
    low = c["low"]
    zero = np.zeros((low.T, low.B, low.nu, low.nx))
    got = ps.expected(oracle, low, c["xs"], c["us"], zero)
    want = sens.expected(oracle, low, c["xs"], c["us"], path=getattr(low, "ref_path", None))
    assert (got["V"] == 0.0).all()
    for kind in ps.KINDS:
        if want[kind] is None:
            assert got["dcost_d" + kind] is None
            continue
        err = cv.traj_relerr(got["dcost_d" + kind], want[kind])
        print("%s d/d%s: %.2e (max |reference| %.2e)" % (key, kind, err, np.abs(want[kind]).max()))
        assert err < 1e-11, (kind, err)
        if low.T > 1:   # (T = 1: the terminal cost's gradient has no motor entries, so dJ/dB is exactly 0)
            assert np.abs(want[kind]).max() > 1e-3


@pytest.mark.parametrize("key", sorted(ps.CASES))
def test_the_gpu_cases_are_well_conditioned(oracle, cases, key):
    """x0 and K moved by 1e-13 relative (seeded signs; the candidate is rolled out again from the moved x0): every output of
    the definition must move by less than 1e-11 in the measure of the GPU tests (cv.traj_relerr), so that 1e-9 there is a
    statement about the kernel.  A condition on the choice of inputs: the cases, candidates and gains are those of
    tests/_covariance.py as they are.  Measured movement, worst output: arm_sea 1.7e-12, arm_vsa 5.2e-13, nu1 6.6e-13, sea
    2.6e-12, sea_one 0, sea_path 2.6e-12, vsa_box 5.4e-12: no case had to be changed."""
    c = cases(key)
    low, K = c["low"], c["K"]
    rng = np.random.default_rng(23)
    K2 = K * (1.0 + 1e-13 * rng.choice([-1.0, 1.0], K.shape))
    x0 = np.array(low.x0)
    xs2, us2 = cv.candidate(oracle, low, x0=x0 * (1.0 + 1e-13 * rng.choice([-1.0, 1.0], x0.shape)))
    assert (us2 == c["us"]).all()
    vk, vb = ps.variances(low, 37)
    base = ps.expected(oracle, low, c["xs"], c["us"], K, vk, vb)
    moved = ps.expected(oracle, low, xs2, us2, K2, vk, vb)
    worst = 0.0
    for k in ps.OUTPUTS:
        if base[k] is None:
            continue
        assert np.isfinite(base[k]).all(), k
        worst = max(worst, cv.traj_relerr(moved[k], base[k]))
    print("%s: worst movement %.2e" % (key, worst))
    assert worst < 1e-11, worst
