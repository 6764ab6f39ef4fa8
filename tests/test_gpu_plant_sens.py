"""aslr_policy_plant_sensitivity on the GPU (include/aslr_to_amd_plant_sens.h; plant_sens_kernel,
csrc/aslr_plant_sens.inc.hpp) against tests/_plant_sens.py: the definition in numpy with full matrices on the oracle's
records, fed the DEVICE's own gains so that only this sweep is compared.

Kernel outputs are held to 1e-9 in the measure max |a - b| / max |b| per output array and trajectory (cv.traj_relerr);
tests/test_plant_sens_host.py shows that the inputs are conditioned for it and pins the definition on the oracle alone.
Shapes (tests/_covariance.CASES): the smallest that leave a partial wave of teams (B = 9 at nx = 8: 8 trajectories per wave;
B = 3 at nx = 28: 2 per wave) and the smallest problem there is (B = 1, T = 1).  Every output sits in a buffer of the test's
own, followed by guard words that must survive."""
import numpy as np
import pytest

import _covariance as cv
import _ext_call as ext
import _gpu_case as gc
import _plant_sens as ps
import _policy as pol
import _sensitivity as sens
import _sweep_gpu as sw
import _traj_oracle
from aslr_to_amd import _abi, crocoddyl, scenarios

pytestmark = pytest.mark.gpu

FIELDS = ps.OUTPUTS   # in the order of the C arguments
_TO_BATCH_MAJOR = {"dx_dstiffness": (1, 0, 2, 3), "dx_dmotor_inertia": (1, 0, 2, 3), "dxT_dstiffness": (0, 1, 2),
                   "dxT_dmotor_inertia": (0, 1, 2), "dcost_dstiffness": (1, 0), "dcost_dmotor_inertia": (1, 0),
                   "x_var": (1, 0, 2), "u_var": (1, 0, 2)}
MOTOR = tuple(k for k in FIELDS if k.endswith("motor_inertia"))
VAR_SEED = 37


def _shapes(e):
    nj = e.nx // 4
    return {"dx_dstiffness": (e.T + 1, e.B, e.nx, nj), "dx_dmotor_inertia": (e.T + 1, e.B, e.nx, nj),
            "dxT_dstiffness": (e.B, e.nx, nj), "dxT_dmotor_inertia": (e.B, e.nx, nj), "dcost_dstiffness": (nj, e.B),
            "dcost_dmotor_inertia": (nj, e.B), "x_var": (e.T + 1, e.B, e.nx), "u_var": (e.T, e.B, e.nu)}


def _fields(low):
    """the outputs a model has: no stiffness ones for VSA"""
    return tuple(k for k in FIELDS if ps.has_stiffness(low) or not k.endswith("stiffness"))


def _raw(e, stiffness_var, motor_inertia_var, which=None, expect=_abi.OK):
    """aslr_policy_plant_sensitivity with the batch-major variances [B, nj] (None: NULL) and the outputs `which` (default:
    all the model has; the others NULL) through the guarded call of tests/_ext_call.py -> dict of batch-major numpy arrays
    (the layout of tests/_plant_sens.expected; u_var with the device's nu), or the message of the refusal"""
    outs = ext.outputs(e.device, _shapes(e), _fields(e.low) if which is None else which, perms=_TO_BATCH_MAJOR)
    args = [e.handle, ext.dev(e.device, stiffness_var, (1, 0)), ext.dev(e.device, motor_inertia_var, (1, 0))]
    return ext.call(e, "aslr_policy_plant_sensitivity", args + [outs.get(k) for k in FIELDS] + [e._stream()], outs, expect)


def _call(c, b=None):
    """_raw with the case's two variances bound (b: cut to trajectory b)"""
    cut = slice(None) if b is None else slice(b, b + 1)
    vk, vb = c["var"]
    return lambda e, **kw: _raw(e, None if vk is None else vk[cut], vb[cut], **kw)


@pytest.fixture(scope="module")
def cases(oracle):
    """the seeded inputs of every case, built once (the open-loop candidate comes from the oracle) and never changed; var:
    the seeded variances (stiffness or None, motor inertia)"""
    return sw.make_cases(oracle, ps.CASES, lambda c: c.update(var=ps.variances(c["low"], VAR_SEED)))


@pytest.fixture(scope="module")
def loaded(cases):
    """key -> (engine with the candidate and its gains in place, the device's K): tests/_sweep_gpu.make_loaded"""
    return sw.make_loaded(cases)


@pytest.mark.parametrize("key", sorted(ps.CASES))
def test_kernel_matches_the_definition(oracle, cases, loaded, key):
    c = cases[key]
    low = c["low"]
    e, K = loaded(key)
    vk, vb = c["var"]
    got = _raw(e, vk, vb)
    want = ps.expected(oracle, low, c["xs"], c["us"], K, vk, vb)
    assert set(got) == set(_fields(low))
    sw.matches(got, want, _fields(low), key)
    assert np.abs(want["dxT_dmotor_inertia"]).max() > 1e-3 and np.abs(want["x_var"]).max() > 1e-6
    if low.T > 1:
        assert np.abs(want["u_var"]).max() > 1e-6 and np.abs(want["dcost_dmotor_inertia"]).max() > 1e-3
    else:   # T = 1: S_0 = 0, so V_0 = 0 on both sides
        assert (got["u_var"] == 0.0).all()
    sw.zero_gain_rows(key, K, got)
    sw.padded_control(key, got)
    if getattr(low, "ref_path", None) is not None:   # ... and the path is what the records were evaluated against
        plain = scenarios.lower(dict(c["sc"], ref_path=None))
        other = ps.expected(oracle, plain, c["xs"], c["us"], K, vk, vb)
        assert cv.traj_relerr(other["dcost_dmotor_inertia"], want["dcost_dmotor_inertia"]) > 1e-6


@pytest.mark.parametrize("key", ["sea", "arm_sea", "arm_vsa"])
def test_every_output_is_optional(cases, loaded, key):
    """each output alone: the bits of the call with all of them, and nothing written past any buffer (_raw checks the
    guards).  The motor-inertia outputs alone, without a stiffness variance, run the kernel without the stiffness columns:
    the same bits again, also for x_var and u_var against a call that computes those columns for dx_dstiffness only"""
    c = cases[key]
    e, _ = loaded(key)
    vk, vb = c["var"]
    full = _raw(e, vk, vb)
    sw.each_output_alone(lambda **kw: _call(c)(e, **kw), full)
    ext.same(_raw(e, None, vb, which=MOTOR), {k: full[k] for k in MOTOR}, "motor inertia only")
    if vk is not None:
        ext.same(_raw(e, vk, None, which=MOTOR), {k: full[k] for k in MOTOR}, "motor inertia outputs, stiffness variance")
        lean = _raw(e, None, vb, which=MOTOR + ("x_var", "u_var"))
        wide = _raw(e, None, vb, which=MOTOR + ("x_var", "u_var", "dx_dstiffness"))
        ext.same(lean, {k: wide[k] for k in lean}, "variances with and without the stiffness columns")
        ext.same({"dx_dstiffness": wide["dx_dstiffness"]}, {"dx_dstiffness": full["dx_dstiffness"]}, "stiffness columns")
        assert cv.traj_relerr(lean["x_var"], full["x_var"]) > 1e-6   # (the stiffness variance is what was left out)


@pytest.mark.parametrize("key", ["sea", "arm_sea", "arm_vsa"])
def test_a_trajectory_does_not_depend_on_where_it_sits(cases, loaded, key):
    """trajectory B - 1 of the batch against the same trajectory alone in a B = 1 engine, bit for bit (sw.trajectory_alone)"""
    c = cases[key]
    e, K = loaded(key)
    sw.trajectory_alone(c, e, K, _call(c), lambda b: _call(c, b))


@pytest.mark.parametrize("key", ["sea", "arm_vsa"])
def test_the_outputs_are_consistent_with_each_other(cases, loaded, key):
    """dxT_* is dx_*[T], bit for bit; on a fresh handle (K = 0) dcost_* agrees with aslr_cost_sensitivity on the same handle
    to 1e-9 (the tangent and the adjoint sweep are dual) and u_var is exactly 0"""
    c = cases[key]
    low = c["low"]
    e, _ = loaded(key)
    vk, vb = c["var"]
    got = _raw(e, vk, vb)
    for kind in ps.KINDS:
        if "dx_d" + kind in got:
            np.testing.assert_array_equal(got["dx_d" + kind][:, low.T].copy().view(np.uint64), got["dxT_d" + kind].view(np.uint64))
    fresh = gc.engine(low)
    gc._upload(fresh, XS=c["xs"], US=c["us"])
    open_loop = _raw(fresh, vk, vb)
    adjoint = fresh.cost_sensitivity()
    gc.sync()
    for kind in ps.KINDS:
        if "dcost_d" + kind not in open_loop:
            assert adjoint.stiffness is None
            continue
        ref = gc.to_np(getattr(adjoint, kind))
        err = cv.traj_relerr(open_loop["dcost_d" + kind], ref)
        print("%s open loop dcost_d%s against the adjoint sweep: %.2e (max |reference| %.2e)" % (key, kind, err, np.abs(ref).max()))
        assert err < 1e-9, (kind, err)
        assert np.abs(ref).max() > 1e-3
    assert (open_loop["u_var"] == 0.0).all()
    assert cv.traj_relerr(open_loop["dxT_dmotor_inertia"], got["dxT_dmotor_inertia"]) > 1e-3   # ... the gains closed the loop above


def test_the_sweep_agrees_with_sampled_plants(cases, loaded):
    """the 2-joint sea case: the device's own aslr_policy_rollout, clamp off, on plants theta_p (1 +- h), two samples per
    parameter; central differences of x_final and of the cost against dx_final_* and dcost_*, within ten times the
    disagreement tests/_plant_sens.FD records for that step (the definition against the oracle's closed loop)"""
    c = cases["sea"]
    low = c["low"]
    e, _ = loaded("sea")
    h, measured, _ = ps.FD["sea"]
    B, nj = low.B, low.nj
    k0 = np.array([pol.nominal_diag(low, b, "K") for b in range(B)])
    b0 = np.array([pol.nominal_diag(low, b, "B") for b in range(B)])
    S = 4 * nj
    pk, pb = np.repeat(k0[:, None, :], S, axis=1), np.repeat(b0[:, None, :], S, axis=1)
    for p in range(2 * nj):
        arr = pk if p < nj else pb
        arr[:, 2 * p, p % nj] *= 1.0 + h
        arr[:, 2 * p + 1, p % nj] *= 1.0 - h
    got = _raw(e, None, None, which=("dxT_dstiffness", "dxT_dmotor_inertia", "dcost_dstiffness", "dcost_dmotor_inertia"))
    res = e.policy_rollout(S, plant_stiffness=pk, plant_motor_inertia=pb, clamp=False)
    gc.sync()
    assert (gc.to_np(res.failed_knot) < 0).all()
    xf, cost = gc.to_np(res.x_final), gc.to_np(res.cost)
    for kind, th, p0 in (("stiffness", k0, 0), ("motor_inertia", b0, nj)):
        dxT, dJ = np.zeros((B, low.nx, nj)), np.zeros((B, nj))
        for j in range(nj):
            step = 2.0 * h * th[:, j]
            dxT[:, :, j] = (xf[:, 2 * (p0 + j)] - xf[:, 2 * (p0 + j) + 1]) / step[:, None]
            dJ[:, j] = (cost[:, 2 * (p0 + j)] - cost[:, 2 * (p0 + j) + 1]) / step
        for name, fd in (("dxT_d" + kind, dxT), ("dcost_d" + kind, dJ)):
            err = cv.traj_relerr(got[name], fd)
            print("%s against sampled plants: %.2e (bound %.1e)" % (name, err, 10 * measured))
            assert err < 10 * measured, (name, err)


def test_the_call_has_the_side_effects_of_calc_diff(cases):
    """3 iterations, the call (both variances, all outputs), 3 more iterations: XS, US, TRAJ_F and TRAJ_I are, bit for bit,
    those of 3 iterations, aslr_calc_diff, 3 iterations on a fresh engine"""
    sw.side_effects_of_calc_diff(cases["vsa_box"], _call(cases["vsa_box"]))


def _refused(e, vk, vb, which, *words):
    msg = _raw(e, vk, vb, which=which, expect=_abi.E_INVALID)
    assert msg.startswith("aslr_policy_plant_sensitivity:") and all(w in msg for w in words), msg


def test_refusals_write_nothing_and_leave_a_live_handle_that_still_solves(cases, loaded):
    """every refusal of the header that a handle can be brought to (the four record shapes are all a handle can have today)"""
    c = cases["sea"]
    sc, low = c["sc"], c["low"]
    vk, vb = c["var"]
    sp = scenarios.solver_params(sc, maxiter=8)
    _, fresh = gc.solve_gpu(low, sp)
    e, K = ext.with_gains(c)
    ok = _raw(e, vk, vb)
    _refused(e, vk, vb, (), "outputs", "NULL")
    _refused(e, None, None, ("x_var",), "stiffness_var", "motor_inertia_var")
    _refused(e, None, None, ("dxT_dmotor_inertia", "u_var"), "stiffness_var", "motor_inertia_var")
    # a zero in the stiffness rows of the table: refused when a stiffness quantity is asked for, and only then
    tp = {k: v for k, v in sc["traj_params"].items() if v is not None}
    zero = np.array(tp["stiffness"])
    zero[2, 1] = 0.0
    e.set_trajectory_params(**dict(tp, stiffness=zero))
    _refused(e, vk, vb, None, "stiffness", "table")
    _refused(e, vk, None, ("x_var",), "stiffness", "table")
    assert set(_raw(e, None, vb, which=MOTOR + ("x_var", "u_var"))) == set(MOTOR + ("x_var", "u_var"))
    e.set_trajectory_params(**tp)
    gc._upload(e, XS=c["xs"], US=c["us"], KGAIN=K)
    ext.same(_raw(e, vk, vb), ok, "the handle after the refusals")
    # ... in the models: a zero stiffness, a K and a B that are not diagonal
    nj = low.nj
    lb = sens.moved(low, 0, "K", 1, 0.0)
    e0 = gc.engine(lb)
    gc._upload(e0, XS=c["xs"][:, :1], US=c["us"][:, :1])
    _refused(e0, vk[:1], vb[:1], None, "stiffness", "K[1]")
    assert set(_raw(e0, None, vb[:1], which=MOTOR)) == set(MOTOR)
    for field in ("K", "B"):
        lb = _traj_oracle.single(scenarios.lower(dict(sc, traj_params=None)), 0)
        for i in range(lb.desc.nmodels):
            getattr(lb.desc.models[i], field)[0 * nj + 1] = 1e-3
        _refused(gc.engine(lb), None, vb[:1], MOTOR, "diagonal")
    # a VSA model refuses every stiffness argument, input or output
    v = cases["vsa_box"]
    ev, _ = loaded("vsa_box")
    vvb = v["var"][1]
    assert v["var"][0] is None
    _refused(ev, vvb, vvb, _fields(v["low"]), "VSA")
    for k in ("dx_dstiffness", "dxT_dstiffness", "dcost_dstiffness"):
        _refused(ev, None, vvb, (k,), "VSA")
    assert set(_raw(ev, None, vvb)) == set(_fields(v["low"]))
    # ... and the handle still solves as a fresh one does
    e.set_candidate(None, None)
    e.solve(sp)
    gc.sync()
    after = gc.solution(e)
    for k in ("xs", "us", "traj_i"):
        np.testing.assert_array_equal(after[k], fresh[k], err_msg=k)


def test_python_facade(cases):
    """solver.policy_plant_sensitivity on two_dof_sea, B = 3, T = 8: the documented shapes and the bits of the raw call on the
    same engine; [nj] variances are broadcast; no variance: x_var and u_var are None; problem.policy_plant_sensitivity at a
    stored policy puts the engine's own back; a VSA model has None in the stiffness fields and refuses stiffness_var;
    double_pendulum_nu1 returns u_var with nu = 1; a negative variance and a wrong shape raise"""
    B, T, nx, nj = 3, 8, 8, 2
    sc = scenarios.two_dof_sea(B=B, T=T, seed=4)
    problem = crocoddyl.ShootingProblem(sc["x0"], sc["running"], sc["terminal"], frame_refs=sc["frame_refs"])
    solver = crocoddyl.SolverDDP(problem)
    solver.solve([], [], 20)
    e = problem.engine
    vk, vb = ps.variances(e.low, 53)
    res = solver.policy_plant_sensitivity(vk, vb, keep_trajectories=True)
    gc.sync()
    for name in ("dx_final_dstiffness", "dx_final_dmotor_inertia"):
        assert tuple(getattr(res, name).shape) == (B, nx, nj), name
    for name in ("dcost_dstiffness", "dcost_dmotor_inertia"):
        assert tuple(getattr(res, name).shape) == (B, nj), name
    for name in ("dxs_dstiffness", "dxs_dmotor_inertia"):
        assert tuple(getattr(res, name).shape) == (B, T + 1, nx, nj), name
    assert tuple(res.x_var.shape) == (B, T + 1, nx) and tuple(res.u_var.shape) == (B, T, 2)
    raw = _raw(e, vk, vb)
    names = {"dx_final_dstiffness": "dxT_dstiffness", "dx_final_dmotor_inertia": "dxT_dmotor_inertia",
             "dxs_dstiffness": "dx_dstiffness", "dxs_dmotor_inertia": "dx_dmotor_inertia", "dcost_dstiffness": "dcost_dstiffness",
             "dcost_dmotor_inertia": "dcost_dmotor_inertia", "x_var": "x_var", "u_var": "u_var"}
    for name, k in names.items():
        np.testing.assert_array_equal(gc.to_np(getattr(res, name)).view(np.uint64), raw[k].view(np.uint64), err_msg=name)
    lean = solver.policy_plant_sensitivity()
    assert lean.x_var is None and lean.u_var is None and lean.dxs_dstiffness is None and lean.dxs_dmotor_inertia is None
    gc.same_bits(lean.dx_final_dstiffness, res.dx_final_dstiffness, "without variances")
    gc.same_bits(lean.dcost_dmotor_inertia, res.dcost_dmotor_inertia, "without variances")
    # broadcasting
    one = solver.policy_plant_sensitivity(vk[0], vb[0])
    tiled = solver.policy_plant_sensitivity(np.tile(vk[0], (B, 1)), np.tile(vb[0], (B, 1)))
    for k in ("x_var", "u_var"):
        gc.same_bits(getattr(one, k), getattr(tiled, k), "broadcast [nj]: %s" % k)
    # ... at a stored policy, through the problem: the same bits, and the engine's own policy is back afterwards
    xs, _, _ = sw.stored_policy_round_trip(problem, e, lambda p, *policy: p.policy_plant_sensitivity(*policy, vk, vb),
                                           {"x_var": res.x_var, "dcost_dstiffness": res.dcost_dstiffness})
    # refusals of the facade
    neg = np.array(vb)
    neg[2, 1] = -1e-3
    with pytest.raises(ValueError, match="negative"):
        solver.policy_plant_sensitivity(vk, neg)
    with pytest.raises(ValueError, match="shape"):
        solver.policy_plant_sensitivity(vk, np.ones((B, nj + 1)))
    with pytest.raises(ValueError, match="together"):
        problem.policy_plant_sensitivity(xs.permute(1, 0, 2), None, None)
    # a VSA model: None in the stiffness fields, stiffness_var refused
    vsc = scenarios.two_dof_vsa_boxddp(B=B, T=T, seed=4)
    vp = crocoddyl.ShootingProblem(vsc["x0"], vsc["running"], vsc["terminal"], frame_refs=vsc["frame_refs"])
    vs = crocoddyl.SolverBoxDDP(vp)
    vs.solve([], [], 5)
    rv = vs.policy_plant_sensitivity(motor_inertia_var=vb[0])
    gc.sync()
    assert rv.dx_final_dstiffness is None and rv.dcost_dstiffness is None and rv.dxs_dstiffness is None
    assert tuple(rv.dx_final_dmotor_inertia.shape) == (B, nx, nj) and tuple(rv.u_var.shape) == (B, T, 4)
    with pytest.raises(ValueError, match="VSA"):
        vs.policy_plant_sensitivity(stiffness_var=vb[0])
    # padded controls are cut
    sw.padded_controls_are_cut(cases, lambda solver: solver.policy_plant_sensitivity(motor_inertia_var=np.ones(2)))
