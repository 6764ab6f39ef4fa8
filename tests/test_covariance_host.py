"""Closed-loop covariance (aslr_policy_covariance, include/aslr_to_amd_cov.h) on a CPU: the contract of the extension header,
the reference of tests/_covariance.py pinned on the oracle alone -- against the nonlinear closed loop of tests/_policy.py by
finite differences and by sampling, and against the vector form of its own recursion -- and the conditioning of the inputs
the GPU cases use (tests/test_gpu_covariance.py)."""
import ctypes as C

import numpy as np
import pytest

import _covariance as cv
import _policy as pol
from aslr_to_amd import _abi, scenarios


def test_a_null_handle_is_refused_by_name():
    lib = _abi.load_library()
    assert lib.aslr_workspace_bytes(None) < 0     # some other message is in the buffer first
    buf = C.cast((C.c_double * 64)(), C.c_void_p)   # stands where a device pointer goes; never dereferenced
    assert lib.aslr_policy_covariance(None, buf, buf, buf, buf, buf, buf, buf, None) == _abi.E_INVALID
    msg = lib.aslr_last_error().decode()
    assert msg.startswith("aslr_policy_covariance:") and "handle" in msg, msg


def _policy_case(oracle, name, B, T):
    """scenario seed 4, the candidate of tests/_covariance.candidate, the oracle's gains of one backward sweep on it"""
    sc = scenarios.SCENARIOS[name](B=B, T=T, seed=4)
    low = scenarios.lower(sc)
    xs, us = cv.candidate(oracle, low)
    return low, xs, us, pol.oracle_gains(oracle, low, scenarios.solver_params(sc), xs, us)


# scenario -> (T, step of the central difference, disagreement measured at it); the bound is ten times the measured value
JACOBIAN_FD = {"two_dof_sea": (5, 1e-6, 1.5e-11), "talos_arm_sea": (4, 1e-5, 1.8e-11)}


def _fd_disagreement(oracle, low, xs, us, K, h):
    """worst over the trajectories of relerr(helper's Sigma_T for sigma0 = I, Phi Phi^T) with Phi = dx_T/dx_0 of the
    nonlinear closed loop by central differences of step h"""
    B, T, nx = low.B, low.T, low.nx
    want = cv.expected(oracle, low, xs, us, K, sigma0=np.tile(np.eye(nx), (B, 1, 1)))["cov_final"]
    got = np.zeros_like(want)
    for b in range(B):
        Phi = np.zeros((nx, nx))
        for i in range(nx):
            e = np.zeros(nx)
            e[i] = h
            xp = pol.rollout_one(oracle, low, b, xs[:, b], us[:, b], K[:, b], dx0=e)["xs"][T]
            xm = pol.rollout_one(oracle, low, b, xs[:, b], us[:, b], K[:, b], dx0=-e)["xs"][T]
            Phi[:, i] = (xp - xm) / (2 * h)
        got[b] = Phi @ Phi.T
    return cv.traj_relerr(want, got)


@pytest.mark.parametrize("name", sorted(JACOBIAN_FD))
def test_the_recursion_is_the_linearisation_of_the_nonlinear_closed_loop(oracle, name):
    """B = 2; Phi = dx_T/dx_0 by central differences of _policy.rollout_one (dx0 = +-h e_i, no clamp, the oracle's gains):
    with sigma0 = I and no noise the helper must give Sigma_T = Phi Phi^T.

    Finite-difference error is not rounding error and has no a-priori bound, so step and bound were fixed as in
    tests/test_sensitivity_host.py: the disagreement measured on the oracle alone over a scan of steps, the step where it is
    smallest, ten times that value for the other seeds.  Measured (worst trajectory, per step 1e-3 / 1e-4 / 1e-5 / 1e-6 /
    1e-7 / 1e-8; truncation falls with h^2 down to the step where the rounding of the difference takes over):
      two_dof_sea    1.2e-6 / 1.2e-8 / 1.2e-10 / 1.5e-11 / 1.2e-9 / 9.8e-9   -> step 1e-6, bound 1.5e-10  (max |K| 372)
      talos_arm_sea  2.4e-7 / 2.4e-9 / 1.8e-11 / 8.8e-11 / 7.6e-10 / 5.0e-9  -> step 1e-5, bound 1.8e-10  (max |K| 123)"""
    T, h, measured = JACOBIAN_FD[name]
    low, xs, us, K = _policy_case(oracle, name, 2, T)
    assert np.abs(K).max() > 1e-3
    err = _fd_disagreement(oracle, low, xs, us, K, h)
    print("%s: disagreement %.2e at step %.0e (bound %.1e)" % (name, err, h, 10 * measured))
    assert err < 10 * measured, err


def test_the_noise_path_matches_the_sample_variance_of_the_nonlinear_closed_loop(oracle):
    """two_dof_sea, T = 5, one trajectory, N = 4000 seeded samples of _policy.rollout_one with Gaussian disturbances of
    standard deviation 1e-4 on every state entry of every knot: the sample variance of every entry of x_T must sit within
    11.2 % of the helper's x_var[T] for noise_var = 1, scaled by 1e-8.  The relative standard error of a Gaussian sample
    variance is sqrt(2 / (N - 1)) = 2.24 %; the bound is five of those."""
    N, sd = 4000, 1e-4
    low, xs, us, K = _policy_case(oracle, "two_dof_sea", 1, 5)
    T, nx = low.T, low.nx
    want = cv.expected(oracle, low, xs, us, K, noise_var=np.ones((1, T, nx)))["x_var"][0, T] * sd * sd
    w = np.random.default_rng(41).normal(0.0, sd, (N, T, nx))
    xT = np.array([pol.rollout_one(oracle, low, 0, xs[:, 0], us[:, 0], K[:, 0], w=w[n])["xs"][T] for n in range(N)])
    got = xT.var(axis=0, ddof=1)
    rel = np.abs(got - want) / want
    print("sample variance against x_var[T]: worst %.3f (bound %.3f)" % (rel.max(), 5 * np.sqrt(2.0 / (N - 1))))
    assert (want > 0).all()
    assert rel.max() < 5 * np.sqrt(2.0 / (N - 1)), rel


@pytest.mark.parametrize("name, T", [("two_dof_sea", 5), ("talos_arm_sea", 4)])
def test_a_rank_one_sigma0_costs_what_its_vector_costs(oracle, name, T):
    """sigma0 = v v^T, no noise: cost_increase = 1/2 sum_t [dx_t; du_t]^T H_t [dx_t; du_t] + 1/2 dx_T^T Lxx_T dx_T with
    dx_{t+1} = A_t dx_t and du_t = -K_t dx_t propagated as vectors; 1e-12 relative"""
    low, xs, us, K = _policy_case(oracle, name, 2, T)
    deriv = cv.records(oracle, low, xs, us)
    blk, A = cv.blocks(low, deriv), cv.closed_loop(low, deriv, K)
    v = np.random.default_rng(43).uniform(-1.0, 1.0, (low.B, low.nx))
    got = cv.propagate(low, deriv, K, sigma0=np.einsum("bi,bj->bij", v, v))["cost_increase"]
    for b in range(low.B):
        dx, want = v[b], 0.0
        for t in range(low.T):
            du = -K[t, b] @ dx
            want += 0.5 * (dx @ blk["Lxx"][t, b] @ dx + 2.0 * dx @ blk["Lxu"][t, b] @ du + du @ blk["Luu"][t, b] @ du)
            dx = A[t, b] @ dx
        want += 0.5 * dx @ blk["Lxx"][low.T, b] @ dx
        err = abs(got[b] - want) / abs(want)
        print("%s trajectory %d: %.2e" % (name, b, err))
        assert err < 1e-12, err


@pytest.mark.parametrize("key", sorted(cv.CASES))
def test_the_gpu_cases_are_well_conditioned(oracle, key):
    """x0 and K moved by 1e-13 relative (seeded signs; the candidate is rolled out again from the moved x0): every output of
    the helper, for each of the three input combinations, must move by less than 1e-11 in the measure of the GPU tests, so
    that 1e-9 there is a statement about the kernel.  A condition on the choice of inputs.

    What was chosen: the issue's shapes as they are (T <= 5), gains of one backward sweep at XREG = 1e-3 (tests/_policy.XREG),
    the candidate of seeded controls with their own open-loop roll-out.  Measured movement, worst output and combination:
    arm_sea 2.4e-12, arm_vsa 9.7e-13, nu1 4.7e-13, sea 7.3e-13, sea_one 1.2e-13, sea_path 7.2e-13, vsa_box 4.4e-12: no case
    had to be changed.  Zero gain rows: vsa_box 133 of 180, arm_vsa 81 of 168, nu1 9 of 18 (the padded control)."""
    c = cv.case(oracle, key)
    low, sp = c["low"], c["sp"]
    K = pol.oracle_gains(oracle, low, sp, c["xs"], c["us"])
    rng = np.random.default_rng(23)
    K2 = K * (1.0 + 1e-13 * rng.choice([-1.0, 1.0], K.shape))
    x0 = np.array(low.x0)
    xs2, us2 = cv.candidate(oracle, low, x0=x0 * (1.0 + 1e-13 * rng.choice([-1.0, 1.0], x0.shape)))
    assert (us2 == c["us"]).all()
    worst = 0.0
    for which in cv.COMBOS:
        s0, w = cv.combo(c, which)
        base = cv.expected(oracle, low, c["xs"], c["us"], K, s0, w)
        moved = cv.expected(oracle, low, xs2, us2, K2, s0, w)
        assert all(np.isfinite(base[k]).all() for k in cv.OUTPUTS)
        worst = max([worst] + [cv.traj_relerr(moved[k], base[k]) for k in cv.OUTPUTS])
    zero_rows = int((np.abs(K).max(axis=-1) == 0.0).sum())
    print("%s: worst movement %.2e; %d of %d gain rows are zero" % (key, worst, zero_rows, K.shape[0] * K.shape[1] * K.shape[2]))
    assert worst < 1e-11, worst
    if key in ("vsa_box", "arm_vsa"):   # gains after a BoxDDP backward sweep: some rows zero, not all
        assert 0 < zero_rows < K.shape[0] * K.shape[1] * K.shape[2]
