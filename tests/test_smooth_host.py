"""State estimation from measurements (aslr_state_smooth, include/aslr_to_amd_smooth.h) on a CPU: the definition of
tests/_smooth.py pinned on the oracle alone -- against the batch weighted least-squares solution of the linearised problem,
against the gradient of the MAP objective, on exact data, against the Gaussian density of its innovations and the filter of
tests/_lqg.py -- and the conditioning of the inputs the GPU cases use (tests/test_gpu_smooth.py)."""
import ctypes as C

import numpy as np
import pytest

import _covariance as cv
import _lqg as lq
import _smooth as sm
import _traj_oracle
from aslr_to_amd import _abi

KEYS = ("sea", "vsa_box", "nu1", "arm_sea", "arm_vsa")   # the cases of tests/test_gpu_smooth.py
RECOVERY_ITERS = 4    # test_exact_data_give_the_true_run_back finds it; tests/test_gpu_smooth.py reuses it
_made = {}


def _case(oracle, key):
    if key not in _made:
        _made[key] = cv.case(oracle, key)
    return _made[key]


def test_refusals_that_need_no_device_name_their_cause():
    lib = _abi.load_library()
    assert lib.aslr_workspace_bytes(None) < 0     # some other message is in the buffer first
    buf = C.cast((C.c_double * 64)(), C.c_void_p)   # stands where a device pointer goes; never dereferenced
    assert lib.aslr_state_smooth(None, 4, None, buf, buf, buf, buf, buf, 1, 1.0, buf, buf, buf, buf, buf, buf, buf, None) == _abi.E_INVALID
    msg = lib.aslr_last_error().decode()
    assert msg.startswith("aslr_state_smooth:") and "handle" in msg, msg


def _least_squares(low, deriv, xnext, xb, ys, m, r, x0_mean, sigma0, noise_var, b):
    """the weighted least-squares solution of the problem linearised about xb, trajectory b, by its normal equations:
         min  |x_0 - x0_mean|^2_{sigma0^-1} + sum_t |y_t - x_t[m]|^2_{R^-1} + sum_t |x_{t+1} - xnext_t - Fx_t (x_t - xb_t)|^2_{Q_t^-1}
    over X = (x_0 .. x_T).  A term whose covariance is absent is a constraint, met by the choice of unknowns z, X = E z + d:
    without sigma0 x_0 = x0_mean and z = (x_1 .. x_T); without noise_var X follows from z = x_0 through the dynamics.
    -> X [T+1, nx], the condition number of the normal matrix"""
    T, nx, ny = low.T, low.nx, len(m)
    n = (T + 1) * nx
    Fx = cv.blocks(low, deriv)["Fx"][:, b]
    aff = [xnext[t, b] - Fx[t] @ xb[t, b] for t in range(T)]   # x_{t+1} = Fx_t x_t + aff_t
    if noise_var is None:
        E, d = np.zeros((n, nx)), np.zeros(n)
        E[:nx] = np.eye(nx)
        for t in range(T):
            E[(t + 1) * nx:(t + 2) * nx] = Fx[t] @ E[t * nx:(t + 1) * nx]
            d[(t + 1) * nx:(t + 2) * nx] = Fx[t] @ d[t * nx:(t + 1) * nx] + aff[t]
    elif sigma0 is None:
        E, d = np.eye(n)[:, nx:], np.zeros(n)
        d[:nx] = x0_mean[b]
    else:
        E, d = np.eye(n), np.zeros(n)
    rows, rhs, wts = [], [], []
    if sigma0 is not None:
        A = np.zeros((nx, n))
        A[:, :nx] = np.eye(nx)
        rows.append(A), rhs.append(x0_mean[b]), wts.append(np.linalg.inv(sigma0[b]))
    for t in range(T + 1):
        A = np.zeros((ny, n))
        A[np.arange(ny), t * nx + np.array(m)] = 1.0
        rows.append(A), rhs.append(ys[b, t]), wts.append(np.diag(1.0 / r[b]))
    if noise_var is not None:
        for t in range(T):
            A = np.zeros((nx, n))
            A[:, (t + 1) * nx:(t + 2) * nx] = np.eye(nx)
            A[:, t * nx:(t + 1) * nx] = -Fx[t]
            rows.append(A), rhs.append(aff[t]), wts.append(np.diag(1.0 / noise_var[b, t]))
    H, g = np.zeros((E.shape[1], E.shape[1])), np.zeros(E.shape[1])
    for A, y, W in zip(rows, rhs, wts):
        AE = A @ E
        H += AE.T @ W @ AE
        g += AE.T @ W @ (y - A @ d)
    z = np.linalg.solve(H, g)
    return (E @ z + d).reshape(T + 1, nx), np.linalg.cond(H)


@pytest.mark.parametrize("which", lq.SETS)
@pytest.mark.parametrize("key", KEYS)
def test_one_iteration_is_the_weighted_least_squares_solution(oracle, key, which):
    """xs_smooth of one iteration on the oracle's records against the normal equations of the same linearised problem,
    assembled and solved with numpy, for the three sigma0 / noise_var combinations (an absent covariance is a constraint).

    Bound: the two sides are equal in exact arithmetic.  The normal equations are solved with a relative forward error of
    about cond(H) eps, and the recursion carries the conditioning of the problem itself, at most the same; the test allows
    100 cond(H) eps relative to max |X| (eps = 2.2e-16), and never less than 1e-12."""
    c = _case(oracle, key)
    low = c["low"]
    d = sm.inputs(c, which)
    xnext, deriv = sm.sweep(oracle, low, d["nominal"], c["us"])
    for combo in cv.COMBOS:
        s0, w = cv.combo(c, combo)
        got = sm.once(low, deriv, xnext, d["nominal"], d["ys"], d["m"], d["r"], d["x0_mean"], s0, w)
        worst, room = 0.0, 0.0
        for b in range(low.B):
            want, cond = _least_squares(low, deriv, xnext, d["nominal"], d["ys"], d["m"], d["r"], d["x0_mean"], s0, w, b)
            err = np.abs(got["xs_smooth"][b] - want).max() / np.abs(want).max()
            bound = max(1e-12, 100.0 * cond * np.finfo(float).eps)
            worst, room = max(worst, err), max(room, err / bound)
            assert err < bound, (b, err, cond)
        print("%s %s %s: worst %.2e, at most %.2e of its bound" % (key, which, combo, worst, room))
        # the smoother ends on the filter
        np.testing.assert_allclose(got["xs_smooth"][:, low.T], got["x_filt"][:, low.T], rtol=0, atol=1e-12 * np.abs(got["x_filt"]).max())


def _map_gradient(oracle, low, X, us, ys, m, r, x0_mean, sigma0, noise_var, b, h=1e-6):
    """gradient of the MAP objective of trajectory b at X [T+1, nx], the model's Jacobian by central differences of
    oracle.knot(..., diff=False)["xnext"] -> the gradient [T+1, nx] and the sum of the magnitudes of its terms"""
    T, nx = low.T, low.nx
    one = _traj_oracle.single(low, b)
    fr = None if low.frame_ref is None else low.frame_ref[b]
    f = lambda t, x: oracle.knot(one, int(low.node_model[t]), x, us[t, b], frame_ref=fr, diff=False)["xnext"]
    g, mag = np.zeros((T + 1, nx)), np.zeros((T + 1, nx))

    def add(t, v):
        g[t] += v
        mag[t] += np.abs(v)
    add(0, np.linalg.solve(sigma0[b], X[0] - x0_mean[b]))
    for t in range(T + 1):
        v = np.zeros(nx)
        v[m] = -(ys[b, t] - X[t, m]) / r[b]
        add(t, v)
    for t in range(T):
        e = (X[t + 1] - f(t, X[t])) / noise_var[b, t]
        add(t + 1, e)
        J = np.stack([(f(t, X[t] + h * np.eye(nx)[i]) - f(t, X[t] - h * np.eye(nx)[i])) / (2.0 * h) for i in range(nx)], axis=1)
        add(t, -J.T @ e)
    return g, mag


@pytest.mark.parametrize("key", ["sea", "vsa_box"])
def test_the_map_gradient_vanishes_where_the_step_has_stalled(oracle, key):
    """the definition iterated 130 times with relax = 0.5: the noise of these cases is of order 1 in radians, there is no line
    search, and the full step cycles on one trajectory of each (sea: trajectory 3), while the damped one contracts on all of
    them (sea: the worst step falls by 16 per ten iterations, 4e-14 at the end).  Every trajectory must have stalled: its
    last step_norm, the full Gauss-Newton step before relax, is below 1e-9.  There the gradient of
         J(X) = 1/2 |x_0 - x0_mean|^2_{sigma0^-1} + 1/2 sum_t |y_t - x_t[m]|^2_{R^-1} + 1/2 sum_t |x_{t+1} - f(x_t, u_t)|^2_{Q_t^-1},
    built from the oracle's xnext alone (the Jacobian by central differences, h = 1e-6), is zero: its largest entry is below
    1e-6 of the largest sum of the magnitudes of an entry's terms.  Central differences carry h^2 |d3f| / 6 + eps |f| / h,
    about 1e-10 relative to the Jacobian for third derivatives of order 100, and a step of 1e-9 leaves a first-order rest of
    that size times the curvature."""
    c = _case(oracle, key)
    low = c["low"]
    d = sm.inputs(c, "default")
    xb = d["nominal"]
    for _ in range(130):
        out = sm.iterate(oracle, low, xb, c["us"], d["ys"], d["m"], d["r"], d["x0_mean"], c["sigma0"], c["noise_var"], 1, 0.5)
        xb = out["XS"]
    print("%s: last steps %s" % (key, " ".join("%.1e" % v for v in out["step_norm"][:, 0])))
    assert (out["step_norm"][:, 0] < 1e-9).all(), out["step_norm"][:, 0]
    worst = 0.0
    for b in range(low.B):
        g, mag = _map_gradient(oracle, low, xb[:, b], c["us"], d["ys"], d["m"], d["r"], d["x0_mean"], c["sigma0"], c["noise_var"], b)
        worst = max(worst, np.abs(g).max() / mag.max())
    print("%s: max |gradient| / max sum |terms| at most %.2e" % (key, worst))
    assert worst < 1e-6, worst


def _recovery(oracle, key, n_iters):
    """the definition on exact data of the case -> step_norm per iteration (the worst trajectory), the error of xs_smooth"""
    c = _case(oracle, key)
    d = sm.inputs(c, "default", noise=False)
    out = sm.iterate(oracle, c["low"], d["nominal"], c["us"], d["ys"], d["m"], d["r"], c["xs"][0], c["sigma0"], c["noise_var"], n_iters)
    return out["step_norm"].max(axis=0), cv.traj_relerr(out["xs_smooth"], c["xs"].transpose(1, 0, 2))


def test_exact_data_give_the_true_run_back(oracle):
    """noise-free ys, x0_mean the true x0, the model the plant, the nominal 1e-2 off the true run (cases sea and arm_sea, the
    positions measured, sigma0 and noise_var both given): the definition returns the true run.  RECOVERY_ITERS is the first
    count at which step_norm is below 1e-10 on every trajectory of both cases; asserted: it is, and one fewer is not.
    Measured, the worst step per iteration: sea 3.3e-02 5.7e-03 9.1e-08 3.6e-15 (error 3.1e-16), arm_sea 3.3e-02 1.2e-03
    5.1e-09 7.1e-15 (error 1.3e-16), so RECOVERY_ITERS = 4.  The error against the true run is then asserted below 1e-9: ten times the step bound."""
    steps = {key: _recovery(oracle, key, RECOVERY_ITERS) for key in ("sea", "arm_sea")}
    for key, (s, err) in steps.items():
        print("%s: steps %s, error %.2e" % (key, " ".join("%.1e" % v for v in s), err))
    assert all(s[-1] < 1e-10 for s, _ in steps.values())
    assert any(s[-2] >= 1e-10 for s, _ in steps.values())
    assert all(err < 1e-9 for _, err in steps.values())


@pytest.mark.parametrize("key", ["sea", "vsa_box", "arm_sea"])
def test_the_likelihood_and_the_filter_are_what_they_say(oracle, key):
    """neg_log_lik is minus the log-density of the innovations, nu_t ~ N(0, S_t), without the constant: 1/2 sum_t (nu^T S^-1 nu
    + log det S_t), with numpy's slogdet and solve on the definition's own Pm; est_var is the diagonal of tests/_lqg.propagate's
    P on the same records; x_filt is m^- + P[:, m] R^-1 nu with that P (the gain in information form).  1e-10: equal in exact
    arithmetic, and test_the_gpu_cases_are_well_conditioned bounds the amplification of 1e-13 by 100."""
    c = _case(oracle, key)
    low = c["low"]
    for which in lq.SETS:
        d = sm.inputs(c, which)
        m, r = d["m"], d["r"]
        xnext, deriv = sm.sweep(oracle, low, d["nominal"], c["us"])
        for combo in cv.COMBOS:
            s0, w = cv.combo(c, combo)
            got = sm.once(low, deriv, xnext, d["nominal"], d["ys"], m, r, d["x0_mean"], s0, w)
            ref = lq.propagate(low, deriv, np.zeros((low.T, low.B, low.nu, low.nx)), m, r, s0, w)
            want = np.zeros(low.B)
            for b in range(low.B):
                for t in range(low.T + 1):
                    S = got["Pm"][b, t][np.ix_(m, m)] + np.diag(r[b])
                    want[b] += 0.5 * (got["nu"][b, t] @ np.linalg.solve(S, got["nu"][b, t]) + np.linalg.slogdet(S)[1])
            assert np.abs(got["nll"] - want).max() < 1e-10 * np.abs(want).max()
            assert cv.traj_relerr(got["est_var"], ref["est_var"]) < 1e-10
            xf = got["mm"] + np.einsum("btia,bta->bti", ref["P"][:, :, :, m] / r[:, None, None, :], got["nu"])
            assert cv.traj_relerr(xf, got["x_filt"]) < 1e-10


@pytest.mark.parametrize("key", KEYS)
def test_the_gpu_cases_are_well_conditioned(oracle, key):
    """ys, meas_var, x0_mean and the nominal moved by 1e-13 relative (seeded signs): every output of the definition, for
    n_iters = 3, every measured set and each of the three input combinations, must move by less than 1e-11 in the measure
    of the GPU tests, so that 1e-9 there is a statement about the kernels.  A condition on the choice of inputs."""
    c = _case(oracle, key)
    low = c["low"]
    rng = np.random.default_rng(29)
    moved = lambda a: a * (1.0 + 1e-13 * rng.choice([-1.0, 1.0], a.shape))
    worst = 0.0
    for which in lq.SETS:
        d = sm.inputs(c, which)
        d2 = {k: (moved(v) if k != "m" else v) for k, v in d.items()}
        for combo in cv.COMBOS:
            s0, w = cv.combo(c, combo)
            base = sm.iterate(oracle, low, d["nominal"], c["us"], d["ys"], d["m"], d["r"], d["x0_mean"], s0, w, 3)
            other = sm.iterate(oracle, low, d2["nominal"], c["us"], d2["ys"], d["m"], d2["r"], d2["x0_mean"], s0, w, 3)
            assert all(np.isfinite(base[k]).all() for k in sm.OUTPUTS)
            worst = max([worst] + [cv.traj_relerr(other[k], base[k]) for k in sm.OUTPUTS])
    print("%s: worst movement %.2e" % (key, worst))
    assert worst < 1e-11, worst
