"""aslr_state_smooth on the GPU (include/aslr_to_amd_smooth.h; smooth_filter_kernel and smooth_adjoint_kernel,
csrc/aslr_smooth.inc.hpp) against tests/_smooth.py: the definition in numpy with full matrices, iterated with the nominal
re-evaluated through the oracle each time.

Outputs are held to 1e-9, the per-kernel figure of the parity suites, in the measure max |a - b| / max |b| per output array
and trajectory; tests/test_smooth_host.py shows that the inputs are conditioned for it.  Shapes (tests/_covariance.CASES): the
smallest that leave a partial wave of teams.  Every output sits in a buffer of the test's own, followed by guard words that
must survive; the call changes XS, so every call starts from the nominal uploaded anew."""
import ctypes as C

import numpy as np
import pytest

import _covariance as cv
import _ext_call as ext
import _gpu_case as gc
import _identify as I
import _lqg as lq
import _smooth as sm
import _sweep_gpu as sw
import _traj_oracle
from aslr_to_amd import _abi, crocoddyl, scenarios
from test_smooth_host import RECOVERY_ITERS

pytestmark = pytest.mark.gpu

KEYS = ("sea", "vsa_box", "nu1", "arm_sea", "arm_vsa")
FIELDS = sm.OUTPUTS
_TO_BATCH_MAJOR = {"xs_smooth": (1, 0, 2), "x_filt": (1, 0, 2), "est_var": (1, 0, 2), "nis": (1, 0), "neg_log_lik": (1, 0),
                   "step_norm": (1, 0)}


def _raw(e, a, n_iters=1, relax=1.0, which=FIELDS, expect=_abi.OK, ny=None, null_list=False, null=(), upload=True):
    """aslr_state_smooth from the nominal a["nominal"] and controls a["us"] (time-major, uploaded first) with the measured
    entries a["m"] (null_list: NULL in their place; ny: the count passed), the batch-major inputs ys, r, x0_mean, sigma0,
    noise_var of `a` (None, or named in `null`: NULL) and the outputs `which` through the guarded call of tests/_ext_call.py
    -> dict of batch-major numpy arrays (the layout of tests/_smooth.iterate), or the message of the refusal"""
    if upload:
        gc._upload(e, XS=a["nominal"], US=a["us"])
    m = a["m"]
    n, N = len(m), max(n_iters, 1)
    shapes = {"xs_smooth": (e.T + 1, e.B, e.nx), "x_filt": (e.T + 1, e.B, e.nx), "est_var": (e.T + 1, e.B, e.nx),
              "nis": (e.T + 1, e.B), "neg_log_lik": (N, e.B), "step_norm": (N, e.B)}
    outs = ext.outputs(e.device, shapes, which, perms=_TO_BATCH_MAJOR)
    work = ext.alloc(((e.T + 1) * e.B * (e.nx * e.nx + e.nx * max(n, 1) + e.nx + max(n, 1)),), e.device)
    idx = None if null_list else (C.c_int32 * max(n, 1))(*m)
    inp = {"ys": ext.dev(e.device, a["ys"], (1, 0, 2)), "meas_var": ext.dev(e.device, a["r"]), "x0_mean": ext.dev(e.device, a["x0_mean"]),
           "sigma0": ext.dev(e.device, a["sigma0"]), "noise_var": ext.dev(e.device, a["noise_var"], (1, 0, 2)), "work": work}
    inp = {k: (None if k in null else v) for k, v in inp.items()}
    args = [e.handle, n if ny is None else ny, idx, inp["ys"], inp["meas_var"], inp["x0_mean"], inp["sigma0"], inp["noise_var"],
            n_iters, float(relax), inp["work"]] + [outs.get(k) for k in FIELDS] + [e._stream()]
    got = ext.call(e, "aslr_state_smooth", args, outs, expect)
    assert ext.guard_intact(work), "the guard behind work was overwritten"
    if expect != _abi.OK:
        assert ext.untouched(work), "work was written by the refused call"
    return got


@pytest.fixture(scope="module")
def cases(oracle):
    """the seeded inputs of every case, built once and never changed"""
    return sw.make_cases(oracle, KEYS)


@pytest.fixture(scope="module")
def engines(cases):
    made = {}

    def get(key):
        if key not in made:
            made[key] = gc.engine(cases[key]["low"])
        return made[key]
    return get


def _args(c, which="default", combo="both", b=None, noise=True):
    """the arguments of a call on the case: tests/_smooth.inputs for the measured set, sigma0 / noise_var of the combination,
    the controls; b: cut to trajectory b"""
    s0, w = cv.combo(c, combo)
    a = dict(sm.inputs(c, which, noise=noise), sigma0=s0, noise_var=w, us=c["us"])
    if b is not None:
        cut = slice(b, b + 1)
        a = dict(a, r=a["r"][cut], ys=a["ys"][cut], x0_mean=a["x0_mean"][cut], nominal=a["nominal"][:, cut], us=a["us"][:, cut],
                 sigma0=None if s0 is None else s0[cut], noise_var=None if w is None else w[cut])
    return a


def _definition(oracle, c, a, n_iters, relax=1.0):
    return sm.iterate(oracle, c["low"], a["nominal"], a["us"], a["ys"], a["m"], a["r"], a["x0_mean"], a["sigma0"], a["noise_var"],
                      n_iters, relax)


@pytest.mark.parametrize("which", lq.SETS)
@pytest.mark.parametrize("key", KEYS)
def test_kernels_match_the_definition(oracle, cases, engines, key, which):
    """every output against the definition for n_iters = 1 and 3, every measured set and the three sigma0 / noise_var
    combinations, within 1e-9 (sw.matches prints every figure); XS afterwards is the definition's.  Worst figure measured:
    profiles/smooth/README.md."""
    c = cases[key]
    e = engines(key)
    for combo in sorted(cv.COMBOS):
        a = _args(c, which, combo)
        for n in (1, 3):
            got = _raw(e, a, n)
            want = _definition(oracle, c, a, n)
            sw.matches(got, want, FIELDS, "%s %s %s n_iters %d" % (key, which, combo, n))
            err = cv.traj_relerr(gc.to_np(e.region(_abi.R_XS)).transpose(1, 0, 2), want["XS"].transpose(1, 0, 2))
            print("%s %s %s n_iters %d XS: %.2e" % (key, which, combo, n, err))
            assert err < 1e-9, err
            assert want["step_norm"][:, 0].min() > 1e-6 and np.abs(want["nis"]).max() > 1e-6   # (something moved)


@pytest.mark.parametrize("key", ["sea", "arm_vsa"])
def test_every_output_is_optional_and_iterations_chain(cases, engines, key):
    """each output alone: the bits of the call with all six; n_iters = 3 is three calls with n_iters = 1, bit for bit (the
    later two start from the XS the one before left)"""
    c = cases[key]
    e = engines(key)
    a = _args(c, "odd")
    full = _raw(e, a, 3)
    xs3 = gc.to_np(e.region(_abi.R_XS))
    sw.each_output_alone(lambda **kw: _raw(e, a, 3, **kw), full)
    singles = [_raw(e, a, 1, upload=(s == 0)) for s in range(3)]
    ext.same(gc.to_np(e.region(_abi.R_XS)), xs3, "XS after three single calls")
    for k in ("xs_smooth", "x_filt", "est_var", "nis"):
        ext.same(singles[2][k], full[k], "%s of the third single call" % k)
    for k in ("neg_log_lik", "step_norm"):
        ext.same(np.concatenate([s[k] for s in singles], axis=1), full[k], "%s of three single calls" % k)


@pytest.mark.parametrize("key", ["sea", "arm_sea"])
def test_a_trajectory_does_not_depend_on_where_it_sits(cases, engines, key):
    """trajectory B - 1 of the batch (the one behind the last full wave of teams) against the same trajectory alone in a
    B = 1 engine (tests/_traj_oracle.single), n_iters = 3: bit for bit"""
    c = cases[key]
    low = c["low"]
    b = low.B - 1
    batch = _raw(engines(key), _args(c), 3)
    alone = _raw(gc.engine(_traj_oracle.single(low, b)), _args(c, b=b), 3)
    ext.same({k: v[0] for k, v in alone.items()}, {k: v[b] for k, v in batch.items()}, "trajectory %d" % b)


@pytest.mark.parametrize("relax", [1.0, 0.5])
def test_side_effects(cases, relax):
    """US, KGAIN and the per-trajectory solver words are unchanged; XS is nominal + relax (xs_smooth - nominal), bit for bit;
    a solve on the used handle equals a solve on a fresh one (ext.solve_matches_a_fresh_handle)"""
    c = cases["vsa_box"]
    low = c["low"]
    e, _ = ext.with_gains(c)
    a = _args(c)
    gc._upload(e, XS=a["nominal"], US=a["us"])
    gc.sync()
    rids = (_abi.R_US, _abi.R_KGAIN, _abi.R_TRAJ_F, _abi.R_TRAJ_I)
    before = {r: gc.to_np(e.region(r)) for r in rids}
    got = _raw(e, a, 1, relax, upload=False)
    for r in rids:
        ext.same(gc.to_np(e.region(r)), before[r], "region %d" % r)
    xs = got["xs_smooth"].transpose(1, 0, 2)
    ext.same(gc.to_np(e.region(_abi.R_XS)), a["nominal"] + relax * (xs - a["nominal"]), "XS")
    assert np.abs(xs - a["nominal"]).max() > 1e-3
    ext.solve_matches_a_fresh_handle(e, low, c["sp"], ext.SOLVE_REGIONS, "after aslr_state_smooth")


def test_refusals_write_nothing_and_leave_a_live_handle(cases, engines):
    c = cases["sea"]
    e = engines("sea")
    a = _args(c)
    ok = _raw(e, a, 2)
    gc._upload(e, XS=a["nominal"], US=a["us"])
    gc.sync()
    xs0 = gc.to_np(e.region(_abi.R_XS))
    refused = lambda a_=a, **k: _raw(e, a_, k.pop("n_iters", 2), k.pop("relax", 1.0), expect=_abi.E_INVALID, upload=False, **k)
    msgs = {
        "ny < 1": (refused(ny=0), ("ny", "0")),
        "ny > nx": (refused(ny=9, null_list=True), ("ny", "9")),
        "an index past nx": (refused(dict(a, m=[0, 8, 2, 3])), ("meas_idx", " 8")),
        "a negative index": (refused(dict(a, m=[0, 1, -1, 3])), ("meas_idx", "-1")),
        "a repeated index": (refused(dict(a, m=[0, 5, 2, 5])), ("meas_idx", " 5")),
        "ys NULL": (refused(null=("ys",)), ("ys", "NULL")),
        "meas_var NULL": (refused(null=("meas_var",)), ("meas_var", "NULL")),
        "x0_mean NULL": (refused(null=("x0_mean",)), ("x0_mean", "NULL")),
        "work NULL": (refused(null=("work",)), ("work", "NULL")),
        "no output": (refused(which=()), ("outputs", "NULL")),
        "nothing to propagate": (refused(null=("sigma0", "noise_var")), ("sigma0", "noise_var")),
        "n_iters < 1": (refused(n_iters=0), ("n_iters", "0")),
        "relax = 0": (refused(relax=0.0), ("relax", "0")),
        "relax > 1": (refused(relax=1.5), ("relax", "1.5")),
        "relax NaN": (refused(relax=float("nan")), ("relax", "nan")),
    }
    for what, (msg, words) in msgs.items():
        assert msg.startswith("aslr_state_smooth:") and all(x in msg for x in words), (what, msg)
    ext.same(gc.to_np(e.region(_abi.R_XS)), xs0, "XS after the refusals")
    ext.same(_raw(e, a, 2), ok, "the handle after the refusals")
    ext.same(_raw(e, a, 2, null_list=True), ok, "a NULL list: the first ny entries")


@pytest.mark.parametrize("key", ["sea", "arm_sea"])
def test_nan_stays_with_its_trajectory(cases, engines, key):
    """meas_var of one trajectory set to -1, no sigma0 (Pm_0 = 0, so the first pivot is -1): its outputs are NaN, every one,
    through three iterations, and its neighbours have the bits of the clean run"""
    c = cases[key]
    e = engines(key)
    a = _args(c, "default", "noise")
    clean = _raw(e, a, 3)
    bad = 1
    r = np.array(a["r"])
    r[bad] = -1.0
    got = _raw(e, dict(a, r=r), 3)
    keep = np.arange(c["low"].B) != bad
    for k in FIELDS:
        assert np.isnan(got[k][bad]).all(), k
        ext.same(got[k][keep], clean[k][keep], "%s of the neighbours" % k)
    assert np.isnan(gc.to_np(e.region(_abi.R_XS))[:, bad]).all()


@pytest.mark.parametrize("key", ["sea", "arm_sea"])
def test_exact_data_give_the_true_run_back(cases, engines, key):
    """the recovery of tests/test_smooth_host.py at its n_iters: noise-free ys, x0_mean the true x0, the nominal 1e-2 off:
    the last step is below 1e-10 and xs_smooth is the true run within 1e-9"""
    c = cases[key]
    a = dict(_args(c, noise=False), x0_mean=c["xs"][0])
    got = _raw(engines(key), a, RECOVERY_ITERS)
    err = cv.traj_relerr(got["xs_smooth"], c["xs"].transpose(1, 0, 2))
    print("%s: steps %s, error %.2e" % (key, " ".join("%.1e" % v for v in got["step_norm"].max(axis=0)), err))
    assert got["step_norm"][:, -1].max() < 1e-10
    assert err < 1e-9, err


def _facade_problem(B=3, T=8):
    sc = scenarios.two_dof_sea(B=B, T=T, seed=4)
    problem = crocoddyl.ShootingProblem(sc["x0"], sc["running"], sc["terminal"], frame_refs=sc["frame_refs"])
    us = np.random.default_rng(5).uniform(-1.0, 1.0, (B, T, 2))
    xs = gc.to_np(problem.rollout(us))
    return sc, problem, xs, us


def test_python_facade():
    """problem.estimate_states on two_dof_sea, B = 3, T = 8: the documented shapes and the bits of the raw call on the same
    engine; the default `measured` is the positions; the default xs_init is the positions of ys and their forward
    differences over dt, the last row repeated; x0_mean defaults to xs_init at knot 0; keep_filter; the refusals"""
    B, T, nx = 3, 8, 8
    sc, problem, xs, us = _facade_problem(B, T)
    e = problem.engine
    dt = float(problem.runningModels[0].dt)
    s0, w = cv.inputs(e.low, 53)
    rng = np.random.default_rng(7)
    ys = xs[:, :, :4] + 1e-3 * rng.standard_normal((B, T + 1, 4))
    res = problem.estimate_states(ys, us, 1e-6, sigma0=s0, noise_var=w, n_iters=2, keep_filter=True)
    gc.sync()
    assert tuple(res.xs.shape) == (B, T + 1, nx) and tuple(res.neg_log_lik.shape) == (B, 2) and tuple(res.step_norm.shape) == (B, 2)
    assert tuple(res.x_filt.shape) == (B, T + 1, nx) and tuple(res.est_var.shape) == (B, T + 1, nx) and tuple(res.nis.shape) == (B, T + 1)
    assert res.measured == [0, 1, 2, 3]
    v = (ys[:, 1:] - ys[:, :-1]) / dt
    init = np.concatenate([ys, np.concatenate([v, v[:, -1:]], axis=1)], axis=2)
    a = dict(m=[0, 1, 2, 3], r=np.full((B, 4), 1e-6), ys=ys, x0_mean=init[:, 0], sigma0=s0, noise_var=w,
             nominal=np.ascontiguousarray(init.transpose(1, 0, 2)), us=gc.to_np(e.region(_abi.R_US)))
    raw = _raw(e, a, 2)
    for k, f in (("xs_smooth", "xs"), ("x_filt", "x_filt"), ("est_var", "est_var"), ("nis", "nis"), ("neg_log_lik", "neg_log_lik"),
                 ("step_norm", "step_norm")):
        ext.same(gc.to_np(getattr(res, f)), raw[k], f)
    lean = problem.estimate_states(ys, us, 1e-6, sigma0=s0, noise_var=w, n_iters=2)
    assert lean.x_filt is None and lean.est_var is None and lean.nis is None
    gc.same_bits(lean.xs, res.xs, "without the filter")
    # a list of its own needs xs_init: with one given, the bits of the raw call with that list
    perm = [2, 0, 3, 1]
    other = problem.estimate_states(ys[:, :, perm], us, 1e-6, measured=perm, xs_init=init, x0_mean=init[:, 0], sigma0=s0, noise_var=w, n_iters=2)
    gc.sync()
    raw_perm = _raw(e, dict(a, m=perm, ys=np.ascontiguousarray(ys[:, :, perm])), 2)
    assert other.measured == perm
    for k, f in (("xs_smooth", "xs"), ("neg_log_lik", "neg_log_lik"), ("step_norm", "step_norm")):
        ext.same(gc.to_np(getattr(other, f)), raw_perm[k], "%s with a list of its own" % f)
    assert cv.traj_relerr(raw_perm["xs_smooth"], raw["xs_smooth"]) < 1e-9   # (the order of the list changes rounding only)
    with pytest.raises(ValueError, match="xs_init"):
        problem.estimate_states(ys[:, :, perm], us, 1e-6, measured=perm, sigma0=s0)
    with pytest.raises(ValueError, match="positive"):
        problem.estimate_states(ys, us, 0.0, sigma0=s0)
    with pytest.raises(ValueError, match="n_iters"):
        problem.estimate_states(ys, us, 1e-6, sigma0=s0, n_iters=0)
    with pytest.raises(ValueError, match="ys"):
        problem.estimate_states(ys[:, :-1], us, 1e-6, sigma0=s0)
    with pytest.raises(_abi.AslrError, match="aslr_state_smooth:"):
        problem.estimate_states(ys, us, 1e-6)
    with pytest.raises(_abi.AslrError, match="relax"):
        problem.estimate_states(ys, us, 1e-6, sigma0=s0, relax=2.0)


def test_the_estimate_goes_into_identify_plant():
    """two_dof_sea: noise-free positions of a roll-out on the plant whose parameters the problem holds -> estimate_states
    (RECOVERY_ITERS iterations from the finite-difference default) -> identify_plant: those parameters come back within
    16 tests/_identify.RECOVERY["sea"][0], the bound tests/test_gpu_identify.py has for exact data."""
    B, T = 3, 8
    sc, problem, xs, us = _facade_problem(B, T)
    nj = 2
    k0 = np.array([[float(m.differential.K[j, j]) for j in range(nj)] for m in problem.runningModels[:1]])[0]
    b0 = np.array([[float(m.differential.B[j, j]) for j in range(nj)] for m in problem.runningModels[:1]])[0]
    est = problem.estimate_states(xs[:, :, :4], us, 1e-8, x0_mean=xs[:, 0], sigma0=1e-8 * np.eye(8), noise_var=1e-8 * np.ones(8),
                                  n_iters=RECOVERY_ITERS)
    print("steps %s, state error %.2e" % (gc.to_np(est.step_norm).max(axis=0), cv.traj_relerr(gc.to_np(est.xs), xs)))
    r = problem.identify_plant(est.xs, us, n_steps=I.N_RECOVER, stiffness_bounds=(0.1 * k0, 10.0 * k0), motor_inertia_bounds=(0.1 * b0, 10.0 * b0))
    rec = max(np.abs(gc.to_np(r.stiffness) / k0 - 1.0).max(), np.abs(gc.to_np(r.motor_inertia) / b0 - 1.0).max())
    print("recovery %.2e (bound %.2e)" % (rec, 16 * I.RECOVERY["sea"][0]))
    assert rec < 16 * I.RECOVERY["sea"][0], rec
