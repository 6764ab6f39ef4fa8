"""aslr_policy_lqg on the GPU (include/aslr_to_amd_lqg.h; lqg_kernel, csrc/aslr_lqg.inc.hpp) against tests/_lqg.py: the
definition in numpy with full matrices on the oracle's records, fed the DEVICE's own gains so that only this sweep is
compared.

Kernel outputs are held to 1e-9, the per-kernel figure of the parity suites, in the measure max |a - b| / max |b| per output
array and trajectory; tests/test_lqg_host.py shows that the inputs are conditioned for it.  Shapes (tests/_covariance.CASES):
the smallest that leave a partial wave of teams and the smallest problem there is (B = 1, T = 1).  Every output sits in a
buffer of the test's own, followed by guard words that must survive."""
import ctypes as C

import numpy as np
import pytest

import _covariance as cv
import _ext_call as ext
import _gpu_case as gc
import _lqg as lq
import _sweep_gpu as sw
from aslr_to_amd import _abi, crocoddyl, scenarios

pytestmark = pytest.mark.gpu

FIELDS = lq.OUTPUTS
_TO_BATCH_MAJOR = {"x_var": (1, 0, 2), "u_var": (1, 0, 2), "est_var": (1, 0, 2), "kalman_gain": (1, 0, 2, 3)}


def _raw(e, m, r, sigma0, noise_var, which=FIELDS, expect=_abi.OK, ny=None, null_list=False):
    """aslr_policy_lqg with the measured entries m (null_list: NULL in their place; ny: the count passed, default len(m)), the
    batch-major inputs meas_var r [B, ny], sigma0 [B, nx, nx] and noise_var [B, T, nx] (None: NULL) and the outputs `which`
    (the others NULL) through the guarded call of tests/_ext_call.py -> dict of batch-major numpy arrays (the layout of
    tests/_lqg.propagate; u_var with the device's nu), or the message of the refusal"""
    n = len(m)
    shapes = {"x_var": (e.T + 1, e.B, e.nx), "u_var": (e.T, e.B, e.nu), "est_var": (e.T + 1, e.B, e.nx),
              "cov_final": (e.B, e.nx, e.nx), "est_cov_final": (e.B, e.nx, e.nx), "kalman_gain": (e.T + 1, e.B, e.nx, max(n, 1)),
              "cost_increase": (e.B,)}
    outs = ext.outputs(e.device, shapes, which, perms=_TO_BATCH_MAJOR)
    idx = None if null_list else (C.c_int32 * max(n, 1))(*m)
    args = [e.handle, n if ny is None else ny, idx, ext.dev(e.device, r), ext.dev(e.device, sigma0),
            ext.dev(e.device, noise_var, (1, 0, 2))] + [outs.get(k) for k in FIELDS] + [e._stream()]
    return ext.call(e, "aslr_policy_lqg", args, outs, expect)


@pytest.fixture(scope="module")
def cases(oracle):
    """the seeded inputs of every case, built once (the open-loop candidate and its records come from the oracle) and never
    changed"""
    return sw.make_cases(oracle, cv.CASES, lambda c: c.update(deriv=cv.records(oracle, c["low"], c["xs"], c["us"])))


@pytest.fixture(scope="module")
def loaded(cases):
    """key -> (engine with the candidate and its gains in place, the device's K): tests/_sweep_gpu.make_loaded"""
    return sw.make_loaded(cases)


def _inputs(c, which="default"):
    """-> the measured entries of the set, the seeded meas_var for them"""
    m = lq.measured(c["low"].nx, which)
    return m, lq.meas_var(c["low"].B, len(m), c["key"])


def _call(c, b=None, which="default"):
    """_raw with the measured entries of the set `which`, their meas_var and the case's sigma0 and noise_var bound (b: cut
    to trajectory b)"""
    cut = slice(None) if b is None else slice(b, b + 1)
    m, r = _inputs(c, which)
    return lambda e, **kw: _raw(e, m, r[cut], c["sigma0"][cut], c["noise_var"][cut], **kw)


@pytest.mark.parametrize("which", lq.SETS)
@pytest.mark.parametrize("key", sorted(cv.CASES))
def test_kernel_matches_the_definition(cases, loaded, key, which):
    c = cases[key]
    low = c["low"]
    e, K = loaded(key)
    m, r = _inputs(c, which)
    for combo in sorted(cv.COMBOS):
        s0, w = cv.combo(c, combo)
        got = _raw(e, m, r, s0, w)
        want = lq.propagate(low, c["deriv"], K, m, r, s0, w)
        sw.matches(got, want, FIELDS, "%s %s %s" % (key, which, combo))
        assert np.abs(want["cost_increase"]).min() > 1e-6 and np.abs(want["est_var"]).max() > 1e-6
        assert np.abs(want["kalman_gain"][:, 1:]).max() > 1e-6
        if s0 is not None:   # (without sigma0 Xh_0 = 0, and at T = 1 that is the only knot with a control)
            assert np.abs(want["u_var"]).max() > 1e-6
        sw.zero_gain_rows(key, K, got)
        sw.padded_control(key, got)


@pytest.mark.parametrize("key", ["sea", "arm_vsa"])
def test_every_output_is_optional(cases, loaded, key):
    """each output alone: the bits of the call with all seven, and nothing written past any buffer (_raw checks the guards);
    est_var with kalman_gain: the kernel branch without the estimate's half and the control terms"""
    c = cases[key]
    e, _ = loaded(key)
    m, r = _inputs(c, "odd")
    full = _raw(e, m, r, c["sigma0"], c["noise_var"])
    sw.each_output_alone(lambda **kw: _call(c, which="odd")(e, **kw), full)
    for pair in (("est_var", "kalman_gain"), ("x_var", "cov_final")):
        got = _raw(e, m, r, c["sigma0"], c["noise_var"], which=pair)
        ext.same(got, {k: full[k] for k in pair}, "a pair without the control terms")


@pytest.mark.parametrize("key", ["sea", "arm_sea"])
def test_a_trajectory_does_not_depend_on_where_it_sits(cases, loaded, key):
    """trajectory B - 1 of the batch against the same trajectory alone in a B = 1 engine, bit for bit (sw.trajectory_alone)"""
    c = cases[key]
    e, K = loaded(key)
    sw.trajectory_alone(c, e, K, _call(c), lambda b: _call(c, b))


@pytest.mark.parametrize("key", ["sea", "arm_vsa"])
def test_the_outputs_are_consistent_with_each_other(cases, loaded, key):
    """the filter on a fresh handle (K = 0) has the bits of the filter beside the gains; x_var >= est_var; the diagonals of
    cov_final and est_cov_final are x_var[T] and est_var[T], bit for bit; the upper triangle of sigma0 is never read; a
    permuted list of measured entries gives the same spread and permuted columns of the gain"""
    c = cases[key]
    low = c["low"]
    e, _ = loaded(key)
    m, r = _inputs(c, "odd")
    got = _raw(e, m, r, c["sigma0"], c["noise_var"])
    fresh = gc.engine(low)
    gc._upload(fresh, XS=c["xs"], US=c["us"])
    open_loop = _raw(fresh, m, r, c["sigma0"], c["noise_var"])
    for k in ("est_var", "est_cov_final", "kalman_gain"):
        ext.same(open_loop[k], got[k], "%s without gains" % k)
    assert (open_loop["u_var"] == 0.0).all()
    assert cv.traj_relerr(open_loop["x_var"], got["x_var"]) > 1e-3   # ... and the gains are what closed the loop above
    assert (got["x_var"] >= got["est_var"]).all()
    for full, diag in (("cov_final", "x_var"), ("est_cov_final", "est_var")):
        np.testing.assert_array_equal(np.einsum("bii->bi", got[full]).copy().view(np.uint64), got[diag][:, low.T].copy().view(np.uint64))
    garbage = np.array(c["sigma0"])
    iu = np.triu_indices(low.nx, 1)
    garbage[:, iu[0], iu[1]] = np.random.default_rng(47).uniform(-1e6, 1e6, (low.B, iu[0].size))
    ext.same(_raw(e, m, r, garbage, c["noise_var"]), got, "garbage above the diagonal of sigma0")
    perm = np.arange(len(m))[::-1]
    other = _raw(e, [m[i] for i in perm], r[:, perm], c["sigma0"], c["noise_var"])
    for k in FIELDS:
        ref = got[k][..., perm] if k == "kalman_gain" else got[k]
        err = cv.traj_relerr(other[k], ref)
        print("%s permuted list %s: %.2e" % (key, k, err))
        assert err < 1e-9, (k, err)


@pytest.mark.parametrize("key", ["sea", "arm_vsa"])
def test_the_stored_matrices_are_symmetric_bit_for_bit(cases, loaded, key):
    """the kernel makes P_t and Xh_t symmetric after every update (left to rounding, the difference of the two triangles
    grows by |Fx|^2 per knot and took every trajectory of a 150-knot plan to NaN): est_cov_final, and cov_final as the sum of
    two such matrices, equal their transposes"""
    c = cases[key]
    e, _ = loaded(key)
    for which in ("default", "all"):
        m, r = _inputs(c, which)
        got = _raw(e, m, r, c["sigma0"], c["noise_var"], which=("cov_final", "est_cov_final"))
        for k, v in got.items():
            ext.same(v.transpose(0, 2, 1), v, "%s against its transpose (%s)" % (k, which))
            assert np.abs(v - np.diag(np.diag(v[0]))).max() > 1e-6   # (there is something off the diagonal)


def test_the_call_has_the_side_effects_of_calc_diff(cases):
    """3 iterations, the call (all inputs, all outputs), 3 more iterations: XS, US, TRAJ_F and TRAJ_I are, bit for bit, those
    of 3 iterations, aslr_calc_diff, 3 iterations on a fresh engine"""
    sw.side_effects_of_calc_diff(cases["vsa_box"], _call(cases["vsa_box"]))


def test_refusals_write_nothing_and_leave_a_live_handle(cases, loaded):
    c = cases["sea"]
    e, _ = loaded("sea")
    m, r = _inputs(c)
    s0, w = c["sigma0"], c["noise_var"]
    ok = _raw(e, m, r, s0, w)
    refused = lambda *a, **k: _raw(e, *a, expect=_abi.E_INVALID, **k)
    msgs = {
        "ny < 1": (refused(m, r, s0, w, ny=0), ("ny", "0")),
        "ny > nx": (refused(m, r, s0, w, ny=9, null_list=True), ("ny", "9")),
        "an index past nx": (refused([0, 8, 2, 3], r, s0, w), ("meas_idx", " 8")),
        "a negative index": (refused([0, 1, -1, 3], r, s0, w), ("meas_idx", "-1")),
        "a repeated index": (refused([0, 5, 2, 5], r, s0, w), ("meas_idx", " 5")),
        "meas_var NULL": (refused(m, None, s0, w), ("meas_var", "NULL")),
        "no output": (refused(m, r, s0, w, which=()), ("outputs", "NULL")),
        "nothing to propagate": (refused(m, r, None, None), ("sigma0", "noise_var")),
    }
    for what, (msg, words) in msgs.items():
        assert msg.startswith("aslr_policy_lqg:") and all(x in msg for x in words), (what, msg)
    ext.same(_raw(e, m, r, s0, w), ok, "the handle after the refusals")
    ext.same(_raw(e, m, r, s0, w, null_list=True), ok, "a NULL list: the first ny entries")


def test_python_facade(cases):
    """solver.policy_lqg on two_dof_sea, B = 3, T = 8: the documented shapes and the bits of the raw call on the same engine;
    every shorter input form is broadcast; problem.policy_lqg at a stored policy puts the engine's own back;
    double_pendulum_nu1 returns u_var with nu = 1; the four refusals of the facade"""
    B, T, nx = 3, 8, 8
    sc = scenarios.two_dof_sea(B=B, T=T, seed=4)
    problem = crocoddyl.ShootingProblem(sc["x0"], sc["running"], sc["terminal"], frame_refs=sc["frame_refs"])
    solver = crocoddyl.SolverDDP(problem)
    solver.solve([], [], 20)
    e = problem.engine
    s0, w = cv.inputs(e.low, 53)
    m = lq.measured(nx, "odd")
    r = lq.meas_var(B, len(m))
    res = solver.policy_lqg(r, m, s0, w, keep_gains=True)
    gc.sync()
    assert tuple(res.x_var.shape) == (B, T + 1, nx) and tuple(res.u_var.shape) == (B, T, 2) and tuple(res.est_var.shape) == (B, T + 1, nx)
    assert tuple(res.cov_final.shape) == (B, nx, nx) and tuple(res.est_cov_final.shape) == (B, nx, nx)
    assert tuple(res.cost_increase.shape) == (B,) and tuple(res.kalman_gain.shape) == (B, T + 1, nx, len(m)) and res.measured == m
    raw = _raw(e, m, r, s0, w)
    for k in FIELDS:
        np.testing.assert_array_equal(gc.to_np(getattr(res, k)).view(np.uint64), raw[k].view(np.uint64), err_msg=k)
    lean = solver.policy_lqg(r, m, s0, w)
    assert lean.kalman_gain is None
    gc.same_bits(lean.x_var, res.x_var, "without the gains")
    # the default list is the positions
    dflt = solver.policy_lqg(r[:, :1].repeat(4, axis=1), None, s0, w)
    assert dflt.measured == [0, 1, 2, 3]
    np.testing.assert_array_equal(gc.to_np(dflt.x_var).view(np.uint64), _raw(e, [0, 1, 2, 3], r[:, :1].repeat(4, axis=1), s0, w)["x_var"].view(np.uint64))
    # broadcasting
    fields = ("x_var", "u_var", "est_var", "cov_final", "est_cov_final", "cost_increase")
    pairs = {
        "scalar meas_var": (solver.policy_lqg(0.3, m, s0, w), solver.policy_lqg(np.full((B, len(m)), 0.3), m, s0, w)),
        "[ny] meas_var": (solver.policy_lqg(r[0], m, s0, w), solver.policy_lqg(np.tile(r[0], (B, 1)), m, s0, w)),
        "[nx, nx] and [nx]": (solver.policy_lqg(r, m, s0[0], w[0, 0]),
                              solver.policy_lqg(r, m, np.tile(s0[0], (B, 1, 1)), np.tile(w[0, 0], (B, T, 1)))),
        "[B, nx]": (solver.policy_lqg(r, m, noise_var=w[:, 0]), solver.policy_lqg(r, m, noise_var=np.repeat(w[:, :1], T, axis=1))),
    }
    for what, (short, tiled) in pairs.items():
        for k in fields:
            gc.same_bits(getattr(short, k), getattr(tiled, k), "broadcast %s: %s" % (what, k))
    # ... at a stored policy, through the problem: the same bits, and the engine's own policy is back afterwards
    sw.stored_policy_round_trip(problem, e, lambda p, *policy: p.policy_lqg(*policy, r, m, s0, w), {"cost_increase": res.cost_increase})
    # refusals of the facade
    skew = np.array(s0)
    skew[1, 2, 5] += 1e-9
    with pytest.raises(ValueError, match="symmetric"):
        solver.policy_lqg(r, m, skew, w)
    neg = np.array(w)
    neg[2, 3, 4] = -1e-3
    with pytest.raises(ValueError, match="negative"):
        solver.policy_lqg(r, m, s0, neg)
    for bad in (0.0, -0.1, np.where(np.arange(len(m)) == 1, 0.0, r)):
        with pytest.raises(ValueError, match="positive"):
            solver.policy_lqg(bad, m, s0, w)
    for bad in ([], [0, 8], [-1], [2, 2], [0.5], list(range(9))):
        with pytest.raises(ValueError, match="measured"):
            solver.policy_lqg(0.3, bad, s0, w)
    with pytest.raises(_abi.AslrError, match="aslr_policy_lqg:"):
        solver.policy_lqg(r, m)
    # padded controls are cut
    sw.padded_controls_are_cut(cases, lambda solver: solver.policy_lqg(0.5, sigma0=np.eye(8)))
