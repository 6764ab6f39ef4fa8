"""aslr_policy_covariance on the GPU (include/aslr_to_amd_cov.h; covariance_kernel, csrc/aslr_covariance.inc.hpp) against
tests/_covariance.py: the definition in numpy with full matrices on the oracle's records, fed the DEVICE's own gains so
that only this sweep is compared.

Kernel outputs are held to 1e-9, the per-kernel figure of the parity suites, in the measure max |a - b| / max |b| per output
array and trajectory; tests/test_covariance_host.py shows that the inputs are conditioned for it.  Shapes
(tests/_covariance.CASES): the smallest that leave a partial wave of teams (B = 9 at nx = 8: 8 trajectories per wave; B = 3 at
nx = 28: 2 per wave) and the smallest problem there is (B = 1, T = 1).  Every output sits in a buffer of the test's own,
followed by guard words that must survive."""
import numpy as np
import pytest

import _covariance as cv
import _ext_call as ext
import _gpu_case as gc
import _sweep_gpu as sw
from aslr_to_amd import _abi, crocoddyl, scenarios

pytestmark = pytest.mark.gpu

FIELDS = cv.OUTPUTS
_TO_BATCH_MAJOR = {"x_var": (1, 0, 2), "u_var": (1, 0, 2), "cov_final": (0, 1, 2), "cov": (1, 0, 2, 3), "cost_increase": (0,)}


def _shapes(e):
    return {"x_var": (e.T + 1, e.B, e.nx), "u_var": (e.T, e.B, e.nu), "cov_final": (e.B, e.nx, e.nx),
            "cov": (e.T + 1, e.B, e.nx, e.nx), "cost_increase": (e.B,)}


def _raw(e, sigma0, noise_var, which=FIELDS, expect=_abi.OK):
    """aslr_policy_covariance with the batch-major inputs sigma0 [B, nx, nx] and noise_var [B, T, nx] (None: NULL) and the
    outputs `which` (the others NULL) through the guarded call of tests/_ext_call.py -> dict of batch-major numpy arrays (the
    layout of tests/_covariance.expected; u_var with the device's nu), or the message of the refusal"""
    outs = ext.outputs(e.device, _shapes(e), which, perms=_TO_BATCH_MAJOR)
    args = [e.handle, ext.dev(e.device, sigma0), ext.dev(e.device, noise_var, (1, 0, 2))] + [outs.get(k) for k in FIELDS] + [e._stream()]
    return ext.call(e, "aslr_policy_covariance", args, outs, expect)


def _call(c, b=None):
    """_raw with the case's sigma0 and noise_var bound (b: cut to trajectory b)"""
    cut = slice(None) if b is None else slice(b, b + 1)
    return lambda e, **kw: _raw(e, c["sigma0"][cut], c["noise_var"][cut], **kw)


@pytest.fixture(scope="module")
def cases(oracle):
    """the seeded inputs of every case, built once (the open-loop candidate comes from the oracle) and never changed"""
    return sw.make_cases(oracle, cv.CASES)


@pytest.fixture(scope="module")
def loaded(cases):
    """key -> (engine with the candidate and its gains in place, the device's K): tests/_sweep_gpu.make_loaded"""
    return sw.make_loaded(cases)


@pytest.mark.parametrize("which", sorted(cv.COMBOS))
@pytest.mark.parametrize("key", sorted(cv.CASES))
def test_kernel_matches_the_definition(oracle, cases, loaded, key, which):
    c = cases[key]
    e, K = loaded(key)
    s0, w = cv.combo(c, which)
    got = _raw(e, s0, w)
    want = cv.expected(oracle, c["low"], c["xs"], c["us"], K, s0, w)
    sw.matches(got, want, FIELDS, "%s %s" % (key, which))
    assert np.abs(want["cost_increase"]).min() > 1e-6
    if not (c["low"].T == 1 and s0 is None):   # (T = 1 without sigma0: Sigma_0 = 0, so U_0 = 0 on both sides)
        assert np.abs(want["u_var"]).max() > 1e-6
    sw.zero_gain_rows(key, K, got)
    sw.padded_control(key, got)
    if getattr(c["low"], "ref_path", None) is not None:   # ... and the path is what the records were evaluated against
        plain = scenarios.lower(dict(c["sc"], ref_path=None))
        assert cv.traj_relerr(cv.expected(oracle, plain, c["xs"], c["us"], K, s0, w)["cost_increase"], want["cost_increase"]) > 1e-6


@pytest.mark.parametrize("key", ["sea", "arm_vsa"])
def test_every_output_is_optional(cases, loaded, key):
    """each output alone: the bits of the call with all five, and nothing written past any buffer (_raw checks the guards)"""
    c = cases[key]
    e, _ = loaded(key)
    full = _raw(e, c["sigma0"], c["noise_var"])
    sw.each_output_alone(lambda **kw: _call(c)(e, **kw), full)
    pair = _raw(e, c["sigma0"], c["noise_var"], which=("x_var", "cov_final"))   # (no control terms: the other kernel branch)
    ext.same(pair, {k: full[k] for k in pair}, "states only")


@pytest.mark.parametrize("key", ["sea", "arm_sea"])
def test_a_trajectory_does_not_depend_on_where_it_sits(cases, loaded, key):
    """trajectory B - 1 of the batch against the same trajectory alone in a B = 1 engine, bit for bit (sw.trajectory_alone)"""
    c = cases[key]
    e, K = loaded(key)
    sw.trajectory_alone(c, e, K, _call(c), lambda b: _call(c, b))


@pytest.mark.parametrize("key", ["sea", "arm_vsa"])
def test_the_outputs_are_consistent_with_each_other(oracle, cases, loaded, key):
    """x_var is the diagonal of cov and cov_final is cov[T], bit for bit; the upper triangle of sigma0 is never read; a fresh
    handle (K = 0) gives the open-loop covariance"""
    c = cases[key]
    low = c["low"]
    e, _ = loaded(key)
    got = _raw(e, c["sigma0"], c["noise_var"])
    np.testing.assert_array_equal(np.einsum("btii->bti", got["cov"]).copy().view(np.uint64), got["x_var"].view(np.uint64))
    np.testing.assert_array_equal(got["cov"][:, low.T].copy().view(np.uint64), got["cov_final"].view(np.uint64))
    garbage = np.array(c["sigma0"])
    iu = np.triu_indices(low.nx, 1)
    garbage[:, iu[0], iu[1]] = np.random.default_rng(47).uniform(-1e6, 1e6, (low.B, iu[0].size))
    ext.same(_raw(e, garbage, c["noise_var"]), got, "garbage above the diagonal of sigma0")
    fresh = gc.engine(low)
    gc._upload(fresh, XS=c["xs"], US=c["us"])
    open_loop = _raw(fresh, c["sigma0"], c["noise_var"])
    want = cv.expected(oracle, low, c["xs"], c["us"], np.zeros((low.T, low.B, low.nu, low.nx)), c["sigma0"], c["noise_var"])
    for k in FIELDS:
        err = cv.traj_relerr(open_loop[k], want[k])
        print("%s open loop %s: %.2e" % (key, k, err))
        assert err < 1e-9, (k, err)
    assert (open_loop["u_var"] == 0.0).all()
    assert cv.traj_relerr(open_loop["x_var"], got["x_var"]) > 1e-3   # ... and the gains are what closed the loop above


def test_the_call_has_the_side_effects_of_calc_diff(cases):
    """3 iterations, the call (all inputs, all outputs), 3 more iterations: XS, US, TRAJ_F and TRAJ_I are, bit for bit, those
    of 3 iterations, aslr_calc_diff, 3 iterations on a fresh engine"""
    sw.side_effects_of_calc_diff(cases["vsa_box"], _call(cases["vsa_box"]))


def test_refusals_write_nothing_and_leave_a_live_handle(cases, loaded):
    c = cases["sea"]
    e, _ = loaded("sea")
    ok = _raw(e, c["sigma0"], c["noise_var"])
    msg = _raw(e, c["sigma0"], c["noise_var"], which=(), expect=_abi.E_INVALID)
    assert msg.startswith("aslr_policy_covariance:") and "outputs" in msg and "NULL" in msg, msg
    msg = _raw(e, None, None, expect=_abi.E_INVALID)
    assert msg.startswith("aslr_policy_covariance:") and "sigma0" in msg and "noise_var" in msg, msg
    ext.same(_raw(e, c["sigma0"], c["noise_var"]), ok, "the handle after the refusals")


def test_python_facade(cases):
    """solver.policy_covariance on two_dof_sea, B = 3, T = 8: the documented shapes and the bits of the raw call on the same
    engine; [nx, nx] and [nx] inputs are broadcast; problem.policy_covariance at a stored policy puts the engine's own back;
    double_pendulum_nu1 returns u_var with nu = 1; a sigma0 that is not symmetric and a negative variance raise"""
    B, T, nx = 3, 8, 8
    sc = scenarios.two_dof_sea(B=B, T=T, seed=4)
    problem = crocoddyl.ShootingProblem(sc["x0"], sc["running"], sc["terminal"], frame_refs=sc["frame_refs"])
    solver = crocoddyl.SolverDDP(problem)
    solver.solve([], [], 20)
    e = problem.engine
    s0, w = cv.inputs(e.low, 53)
    res = solver.policy_covariance(s0, w, keep_cov=True)
    gc.sync()
    assert tuple(res.x_var.shape) == (B, T + 1, nx) and tuple(res.u_var.shape) == (B, T, 2)
    assert tuple(res.cov_final.shape) == (B, nx, nx) and tuple(res.cost_increase.shape) == (B,)
    assert tuple(res.cov.shape) == (B, T + 1, nx, nx)
    raw = _raw(e, s0, w)
    for k in FIELDS:
        np.testing.assert_array_equal(gc.to_np(getattr(res, k)).view(np.uint64), raw[k].view(np.uint64), err_msg=k)
    lean = solver.policy_covariance(s0, w)
    assert lean.cov is None
    gc.same_bits(lean.x_var, res.x_var, "without cov")
    # broadcasting
    one = solver.policy_covariance(s0[0], w[0, 0])
    tiled = solver.policy_covariance(np.tile(s0[0], (B, 1, 1)), np.tile(w[0, 0], (B, T, 1)))
    per_b = solver.policy_covariance(noise_var=w[:, 0])
    tiled_b = solver.policy_covariance(noise_var=np.repeat(w[:, :1], T, axis=1))
    for k in ("x_var", "u_var", "cov_final", "cost_increase"):
        gc.same_bits(getattr(one, k), getattr(tiled, k), "broadcast [nx, nx] and [nx]: %s" % k)
        gc.same_bits(getattr(per_b, k), getattr(tiled_b, k), "broadcast [B, nx]: %s" % k)
    # ... at a stored policy, through the problem: the same bits, and the engine's own policy is back afterwards
    sw.stored_policy_round_trip(problem, e, lambda p, *policy: p.policy_covariance(*policy, s0, w), {"cost_increase": res.cost_increase})
    # refusals of the facade
    skew = np.array(s0)
    skew[1, 2, 5] += 1e-9
    with pytest.raises(ValueError, match="symmetric"):
        solver.policy_covariance(skew, w)
    neg = np.array(w)
    neg[2, 3, 4] = -1e-3
    with pytest.raises(ValueError, match="negative"):
        solver.policy_covariance(s0, neg)
    with pytest.raises(_abi.AslrError, match="aslr_policy_covariance:"):
        solver.policy_covariance()
    # padded controls are cut
    sw.padded_controls_are_cut(cases, lambda solver: solver.policy_covariance(np.eye(8)))
