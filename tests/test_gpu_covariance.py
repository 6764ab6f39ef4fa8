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
import _traj_oracle
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


@pytest.fixture(scope="module")
def cases(oracle):
    """the seeded inputs of every case, built once (the open-loop candidate comes from the oracle) and never changed"""
    return {key: cv.case(oracle, key) for key in cv.CASES}


@pytest.fixture(scope="module")
def loaded(cases):
    """key -> (engine with the candidate and its gains in place, the device's K), made on first use and shared: the call
    under test changes nothing it reads"""
    made = {}

    def get(key):
        if key not in made:
            made[key] = ext.with_gains(cases[key])
        return made[key]
    return get


@pytest.mark.parametrize("which", sorted(cv.COMBOS))
@pytest.mark.parametrize("key", sorted(cv.CASES))
def test_kernel_matches_the_definition(oracle, cases, loaded, key, which):
    c = cases[key]
    e, K = loaded(key)
    s0, w = cv.combo(c, which)
    got = _raw(e, s0, w)
    want = cv.expected(oracle, c["low"], c["xs"], c["us"], K, s0, w)
    for k in FIELDS:
        assert got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
        err = cv.traj_relerr(got[k], want[k])
        print("%s %s %s: %.2e (max |reference| %.2e)" % (key, which, k, err, np.abs(want[k]).max()))
        assert err < 1e-9, (k, err)
    assert np.abs(want["cost_increase"]).min() > 1e-6
    if not (c["low"].T == 1 and s0 is None):   # (T = 1 without sigma0: Sigma_0 = 0, so U_0 = 0 on both sides)
        assert np.abs(want["u_var"]).max() > 1e-6
    if key in ("vsa_box", "arm_vsa"):   # gains after a BoxDDP backward sweep: some rows are zero, and so is their variance
        zero = np.abs(K).max(axis=-1) == 0.0
        assert zero.any() and not zero.all()
        assert (got["u_var"].transpose(1, 0, 2)[zero] == 0.0).all()
    if key == "nu1":
        assert (got["u_var"][..., 1] == 0.0).all()   # the padded control
    if getattr(c["low"], "ref_path", None) is not None:   # ... and the path is what the records were evaluated against
        plain = scenarios.lower(dict(c["sc"], ref_path=None))
        assert cv.traj_relerr(cv.expected(oracle, plain, c["xs"], c["us"], K, s0, w)["cost_increase"], want["cost_increase"]) > 1e-6


@pytest.mark.parametrize("key", ["sea", "arm_vsa"])
def test_every_output_is_optional(cases, loaded, key):
    """each output alone: the bits of the call with all five, and nothing written past any buffer (_raw checks the guards)"""
    c = cases[key]
    e, _ = loaded(key)
    full = _raw(e, c["sigma0"], c["noise_var"])
    for k in FIELDS:
        ext.same(_raw(e, c["sigma0"], c["noise_var"], which=(k,)), {k: full[k]}, "alone")
    pair = _raw(e, c["sigma0"], c["noise_var"], which=("x_var", "cov_final"))   # (no control terms: the other kernel branch)
    ext.same(pair, {k: full[k] for k in pair}, "states only")


@pytest.mark.parametrize("key", ["sea", "arm_sea"])
def test_a_trajectory_does_not_depend_on_where_it_sits(cases, loaded, key):
    """trajectory B - 1 of the batch (the one behind the last full wave of teams) against the same trajectory alone in a
    B = 1 engine (tests/_traj_oracle.single: its row of the table in the models) with the batch's gains uploaded: bit for
    bit"""
    c = cases[key]
    low = c["low"]
    e, K = loaded(key)
    batch = _raw(e, c["sigma0"], c["noise_var"])
    b = low.B - 1
    e1 = gc.engine(_traj_oracle.single(low, b))
    gc._upload(e1, XS=c["xs"][:, b:b + 1], US=c["us"][:, b:b + 1], KGAIN=K[:, b:b + 1])
    alone = _raw(e1, c["sigma0"][b:b + 1], c["noise_var"][b:b + 1])
    ext.same({k: v[0] for k, v in alone.items()}, {k: v[b] for k, v in batch.items()}, "trajectory %d" % b)


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
    c = cases["vsa_box"]
    low, sp = c["low"], c["sp"]
    runs = []
    for call in (lambda e: _raw(e, c["sigma0"], c["noise_var"]), lambda e: e.calc_diff()):
        e = gc.engine(low)
        e.set_candidate(None, None)
        e.iterate_n(sp, True, 3)
        call(e)
        e.iterate_n(sp, False, 3)
        gc.sync()
        runs.append(gc.solution(e))
    assert (runs[1]["traj_i"][_abi.TI_ITER] > 3).any()
    for k in runs[0]:
        np.testing.assert_array_equal(runs[0][k], runs[1][k], err_msg=k)


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
    xs, us, K = (e.region(r).clone() for r in (_abi.R_XS, _abi.R_US, _abi.R_KGAIN))
    for r in (_abi.R_XS, _abi.R_US, _abi.R_KGAIN):
        e.region(r).fill_(0.25)
    again = problem.policy_covariance(xs.permute(1, 0, 2), us.permute(1, 0, 2), K.permute(1, 0, 2, 3), s0, w)
    gc.same_bits(again.cost_increase, res.cost_increase, "the stored policy given explicitly")
    for r in (_abi.R_XS, _abi.R_US, _abi.R_KGAIN):
        assert (e.region(r) == 0.25).all()
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
    psc = cases["nu1"]["sc"]
    pp = crocoddyl.ShootingProblem(psc["x0"], psc["running"], psc["terminal"], frame_refs=psc["frame_refs"])
    ps = crocoddyl.SolverDDP(pp)
    ps.solve([], [], 3)
    r1 = ps.policy_covariance(np.eye(8))
    gc.sync()
    assert tuple(r1.u_var.shape) == (3, cases["nu1"]["low"].T, 1) and tuple(r1.x_var.shape) == (3, cases["nu1"]["low"].T + 1, 8)
