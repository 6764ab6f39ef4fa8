"""aslr_policy_rollout_all on the GPU (include/aslr_to_amd_policy_all.h; policy_rollout_team_kernel,
csrc/aslr_policy_team.inc.hpp) against tests/_policy.py: the definition as a numpy loop over the oracle's knot evaluation,
fed the DEVICE's own gains so that only the roll-out is compared.

Kernel outputs are held to 1e-9 relative, the per-kernel bound of the parity suites (max |a - b| / (1 + |b|));
tests/test_policy_team_host.py shows that the inputs are conditioned for it.  Shapes: tests/_policy_team.CASES.  The entry
point is called raw, every output in a buffer of the test's own, followed by guard words that must survive."""
import numpy as np
import pytest

import _covariance as cv
import _ext_call as ext
import _gpu_case as gc
import _plant_sens as ps
import _policy as pol
import _policy_team as pt
from aslr_to_amd import _abi, crocoddyl, scenarios

pytestmark = pytest.mark.gpu

FIELDS = ext.POLICY_FIELDS
NAME = "aslr_policy_rollout_all"


def _raw(e, *args, name=NAME, **kw):
    """ext.policy_rollout(e, name, S, pert=None, clamp=False, which=FIELDS, expect=OK, room=None)"""
    return ext.policy_rollout(e, name, *args, **kw)


@pytest.fixture(scope="module")
def cases(oracle):
    """the seeded inputs of a case, built on first use (the open-loop candidate comes from the oracle) and never changed"""
    made = {}

    def get(key):
        if key not in made:
            made[key] = pt.case(oracle, key) if isinstance(key, tuple) or key in pt.CASES else pol.case(oracle, key)
        return made[key]
    return get


@pytest.fixture(scope="module")
def loaded(cases):
    """key -> (engine with the candidate and its gains in place, the device's K, the call with all inputs and all outputs),
    made on first use and shared: the call under test changes nothing it reads"""
    made = {}

    def get(key):
        if key not in made:
            c = cases(key)
            e, K = ext.with_gains(c)
            made[key] = (e, K, _raw(e, c["S"], c["pert"], c["clamp"]))
        return made[key]
    return get


@pytest.mark.parametrize("key", sorted(pt.CASES))
def test_kernel_matches_the_definition(oracle, cases, loaded, key):
    c = cases(key)
    low, S = c["low"], c["S"]
    e, K, got = loaded(key)
    want = pol.rollout(oracle, low, c["xs"], c["us"], K, S, clamp=c["clamp"], **c["pert"])
    assert (want["failed_knot"] == -1).all()
    np.testing.assert_array_equal(got["failed_knot"], want["failed_knot"])
    assert np.abs(want["xs"] - c["xs"].transpose(1, 0, 2)[:, None]).max() > 1e-3   # the perturbations moved the loop
    for k in pol.OUTPUTS:
        print("%s %s: %.2e" % (key, k, gc.relerr(got[k], want[k])))
    for k in pol.OUTPUTS:
        gc._assert_close("%s %s" % (key, k), got[k], want[k], 1e-9)
    if c["clamp"]:
        assert want["bound"].any() and not want["bound"].all(), "the narrowed box must bind on some samples"
    if getattr(low, "ref_path", None) is not None:   # ... and the path is what the costs were evaluated against
        plain = scenarios.lower(dict(c["sc"], ref_path=None))
        assert gc.relerr(pol.rollout(oracle, plain, c["xs"], c["us"], K, S, **c["pert"])["cost"], want["cost"]) > 1e-6


@pytest.mark.parametrize("name", ["talos_arm_sea", "talos_arm_vsa"])
def test_without_perturbations_a_solution_rolls_out_onto_itself(name):
    """After a converged solve of the arm (B = 2, T = 4), every input NULL, S = 2: xs_closed is XS, us_closed is US and the
    cost is TF_COST, all within 1e-9 (the kernel is held to the definition, not to the bits of the solver's roll-out; whether
    the bits are equal is printed)"""
    sc = scenarios.SCENARIOS[name](B=2, T=4, seed=4)
    low, sp = scenarios.lower(sc), scenarios.solver_params(sc)
    e, sol = gc.solve_gpu(low, sp)
    assert ((sol["traj_i"][_abi.TI_STATUS] & _abi.ST_CONVERGED) != 0).all(), sol["traj_i"][_abi.TI_STATUS]
    got = _raw(e, 2, None, sp.solver == _abi.SOLVER_BOXDDP)
    assert (got["failed_knot"] == -1).all()
    for s in range(2):
        for k, ref in (("xs", sol["xs"].transpose(1, 0, 2)), ("us", sol["us"].transpose(1, 0, 2)), ("x_final", sol["xs"][-1]),
                       ("cost", sol["traj_f"][_abi.TF_COST])):
            a = np.ascontiguousarray(got[k][:, s])
            print("%s sample %d %s: %.2e, bits equal: %s" % (name, s, k, gc.relerr(a, ref),
                                                            bool((a.view(np.uint64) == np.ascontiguousarray(ref).view(np.uint64)).all())))
            gc._assert_close("%s %s" % (name, k), a, ref, 1e-9)


def test_a_sample_does_not_depend_on_where_it_sits(cases, loaded):
    """sample s of trajectory b at (B, S) = (3, 17) against the same sample run alone at (1, 1), its inputs sliced out (its
    own row of the table, the batch's gains): bit for bit; and the call with only `cost` requested returns the bits of the
    call with all five outputs"""
    c = cases("arm_sea_table")
    sc, S = c["sc"], c["S"]
    e, K, batch = loaded("arm_sea_table")
    ext.same(_raw(e, S, c["pert"], which=("cost",)), {"cost": batch["cost"]}, "cost alone")
    for b, s in ((0, 0), (1, 7), (2, 8), (2, 16), (1, 15)):
        one = dict(sc, x0=sc["x0"][b:b + 1], frame_refs=sc["frame_refs"][b:b + 1])
        one["traj_params"] = {k: (None if v is None else v[b:b + 1]) for k, v in sc["traj_params"].items()}
        e1 = gc.engine(scenarios.lower(one))
        gc._upload(e1, XS=c["xs"][:, b:b + 1], US=c["us"][:, b:b + 1], KGAIN=K[:, b:b + 1])
        alone = _raw(e1, 1, {k: (None if v is None else v[b:b + 1, s:s + 1]) for k, v in c["pert"].items()})
        ext.same({k: v[0, 0] for k, v in alone.items()}, {k: v[b, s] for k, v in batch.items()}, "sample %d of trajectory %d" % (s, b))


@pytest.mark.parametrize("key", ["arm_sea_table", "arm_sea_plain"])
def test_the_nominal_plant_given_explicitly_is_the_null_plant(cases, loaded, key):
    """the trajectories' own K and B passed as plant arrays: the bits of passing NULL (dx0 and disturbance as in the case)"""
    c = cases(key)
    low, S = c["low"], c["S"]
    e = loaded(key)[0]
    nom = lambda f: np.repeat(np.array([pol.nominal_diag(low, b, f) for b in range(low.B)])[:, None, :], S, axis=1)
    none = dict(c["pert"], plant_stiffness=None, plant_motor_inertia=None)
    null = _raw(e, S, none)
    ext.same(_raw(e, S, dict(none, plant_stiffness=nom("K"), plant_motor_inertia=nom("B"))), null, "explicit nominal plant against NULL")
    ext.same(_raw(e, S, dict(none, plant_stiffness=nom("K"))), null, "stiffness alone")


def test_the_call_leaves_a_solve_in_progress_as_it_was(cases):
    """3 iterations, the call (all inputs, all outputs), 3 more iterations: XS, US, TRAJ_F and TRAJ_I are, bit for bit, those
    of 6 iterations on a fresh engine"""
    c = cases("arm_vsa_box")
    low, sp = c["low"], c["sp"]
    e = gc.engine(low)
    e.set_candidate(None, None)
    e.iterate_n(sp, True, 3)
    _raw(e, c["S"], c["pert"], True)
    e.iterate_n(sp, False, 3)
    gc.sync()
    with_call = gc.solution(e)
    e6 = gc.engine(low)
    e6.set_candidate(None, None)
    e6.iterate_n(sp, True, 6)
    gc.sync()
    six = gc.solution(e6)
    assert (six["traj_i"][_abi.TI_ITER] == 6).all()
    ext.same(with_call, six, "3 + call + 3 against 6")


def test_a_diverging_sample_fails_alone(oracle, cases):
    """B = 2, S = 3: the motor inertias of one sample are set to -1e-300, so that its first step leaves 1e30 behind; it reports
    the knot the oracle's loop reports and a NaN cost, and its neighbours in the same wave keep, bit for bit, what they give
    without it"""
    c = cases(("talos_arm_sea", False, False, 2, 3, 4, False, False))
    low, S = c["low"], c["S"]
    e, K = ext.with_gains(c)
    base = _raw(e, S, c["pert"])
    pb = np.array(c["pert"]["plant_motor_inertia"])
    pb[1, 1] = -1e-300
    pert = dict(c["pert"], plant_motor_inertia=pb)
    got = _raw(e, S, pert)
    want = pol.rollout(oracle, low, c["xs"], c["us"], K, S, **pert)
    assert want["failed_knot"][1, 1] >= 0
    np.testing.assert_array_equal(got["failed_knot"], want["failed_knot"])
    assert np.isnan(got["cost"][1, 1])
    keep = np.ones((low.B, S), dtype=bool)
    keep[1, 1] = False
    assert (got["failed_knot"][keep] == -1).all()
    ext.same({k: v[keep] for k, v in got.items()}, {k: v[keep] for k, v in base.items()}, "the other samples")


@pytest.mark.parametrize("key", ["sea_table", "vsa_box"])
def test_a_two_joint_handle_gets_the_bits_of_the_old_entry_point(cases, key):
    c = cases(key)
    e, _ = ext.with_gains(c)
    ext.same(_raw(e, c["S"], c["pert"], c["clamp"]), _raw(e, c["S"], c["pert"], c["clamp"], name="aslr_policy_rollout"),
          "aslr_policy_rollout_all against aslr_policy_rollout")


def test_refusals_write_nothing_and_leave_a_live_handle(oracle, cases, loaded):
    c = cases("arm_vsa_box")
    e, _, ok = loaded("arm_vsa_box")
    S = c["S"]

    def refused(eng, S_, pert, *words, **kw):
        msg = _raw(eng, S_, pert, expect=_abi.E_INVALID, **kw)
        assert msg.startswith(NAME + ":") and all(w in msg for w in words), msg

    for bad_s in (0, -3):
        refused(e, bad_s, None, "n_samples")
    refused(e, 16 * 65535 + 1, None, "n_samples", "above", room=1)
    refused(e, S, c["pert"], "NULL", which=())
    refused(e, S, dict(c["pert"], plant_stiffness=np.ones((c["low"].B, S, 7))), "VSA")
    ext.same(_raw(e, S, c["pert"], True), ok, "the handle after the refusals")
    # K that is not diagonal: refused with a plant argument, rolled out on the full rows without one (open loop: K = 0)
    low = scenarios.lower(scenarios.talos_arm_sea(B=2, T=3, seed=4))
    for i in range(low.desc.nmodels):   # (the lowered description is what aslr_problem_create reads)
        low.desc.models[i].K[1] = low.desc.models[i].K[7] = 0.03
    e2 = gc.engine(low)
    refused(e2, 2, dict(plant_motor_inertia=np.full((2, 2, 7), 1e-2)), "diagonal")
    zx, zu, zk = np.zeros((4, 2, 28)), np.zeros((3, 2, 7)), np.zeros((3, 2, 7, 28))
    gc._upload(e2, XS=zx, US=zu, KGAIN=zk)
    got = _raw(e2, 2, None)
    want = pol.rollout(oracle, low, zx, zu, zk, 2)
    diag = scenarios.lower(scenarios.talos_arm_sea(B=2, T=3, seed=4))
    assert gc.relerr(pol.rollout(oracle, diag, zx, zu, zk, 2)["x_final"], want["x_final"]) > 1e-6   # the off-diagonals matter
    for k in pol.OUTPUTS:
        print("full rows %s: %.2e" % (k, gc.relerr(got[k], want[k])))
    for k in pol.OUTPUTS:
        gc._assert_close("full rows %s" % k, got[k], want[k], 1e-9)


def test_the_first_order_sweep_agrees_with_sampled_plants(oracle):
    """the 7-joint arm_sea case of tests/_plant_sens.py: the roll-outs of this kernel, clamp off, on plants theta_p (1 +- h),
    two samples per parameter (S = 4 nj); central differences of x_final and of the cost against dx_final_* and dcost_* of
    aslr_policy_plant_sensitivity, within ten times the disagreement tests/_plant_sens.FD records for that step"""
    c = cv.case(oracle, "arm_sea")
    low = c["low"]
    e, _ = ext.with_gains(c)
    h, measured, _ = ps.FD["arm_sea"]
    B, nj = low.B, low.nj
    assert nj == 7
    k0 = np.array([pol.nominal_diag(low, b, "K") for b in range(B)])
    b0 = np.array([pol.nominal_diag(low, b, "B") for b in range(B)])
    S = 4 * nj
    pk, pb = np.repeat(k0[:, None, :], S, axis=1), np.repeat(b0[:, None, :], S, axis=1)
    for p in range(2 * nj):
        arr = pk if p < nj else pb
        arr[:, 2 * p, p % nj] *= 1.0 + h
        arr[:, 2 * p + 1, p % nj] *= 1.0 - h
    sweep = e.policy_plant_sensitivity()
    res = _raw(e, S, dict(plant_stiffness=pk, plant_motor_inertia=pb), which=("cost", "failed_knot", "x_final"))
    assert (res["failed_knot"] < 0).all()
    xf, cost = res["x_final"], res["cost"]
    for kind, th, p0 in (("stiffness", k0, 0), ("motor_inertia", b0, nj)):
        dxT, dJ = np.zeros((B, low.nx, nj)), np.zeros((B, nj))
        for j in range(nj):
            step = 2.0 * h * th[:, j]
            dxT[:, :, j] = (xf[:, 2 * (p0 + j)] - xf[:, 2 * (p0 + j) + 1]) / step[:, None]
            dJ[:, j] = (cost[:, 2 * (p0 + j)] - cost[:, 2 * (p0 + j) + 1]) / step
        for name, fd in (("dx_final_d" + kind, dxT), ("dcost_d" + kind, dJ)):
            err = cv.traj_relerr(gc.to_np(getattr(sweep, name)), fd)
            print("%s against sampled plants: %.2e (bound %.1e)" % (name, err, 10 * measured))
            assert err < 10 * measured, (name, err)


def test_python_facade():
    """solver.policy_rollout on talos_arm_sea: the documented shapes, and the bits of the raw call on the same engine;
    problem.policy_rollout at the stored policy given explicitly returns the same bits"""
    import torch
    B, T, S = 2, 4, 5
    sc = scenarios.talos_arm_sea(B=B, T=T, seed=4)
    problem = crocoddyl.ShootingProblem(sc["x0"], sc["running"], sc["terminal"], frame_refs=sc["frame_refs"])
    solver = getattr(crocoddyl, sc["solver"])(problem)
    solver.solve([], [], 5)
    e = problem.engine
    pert = pol.perturbations(e.low, S, 29)
    res = solver.policy_rollout(S, keep_trajectories=True, **pert)
    gc.sync()
    assert tuple(res.cost.shape) == (B, S) and tuple(res.failed_knot.shape) == (B, S) and res.failed_knot.dtype == torch.int32
    assert tuple(res.x_final.shape) == (B, S, 28) and tuple(res.xs.shape) == (B, S, T + 1, 28) and tuple(res.us.shape) == (B, S, T, 7)
    raw = _raw(e, S, pert, clamp=sc["solver"] == "SolverBoxDDP")
    for k in FIELDS:
        a = gc.to_np(getattr(res, k))
        np.testing.assert_array_equal(a.view(np.uint64) if a.dtype == np.float64 else a,
                                      raw[k].view(np.uint64) if raw[k].dtype == np.float64 else raw[k], err_msg=k)
    lean = solver.policy_rollout(S, **pert)
    assert lean.xs is None and lean.us is None
    gc.same_bits(lean.cost, res.cost, "costs without the trajectories")
    xs, us, K = (e.region(r).clone() for r in (_abi.R_XS, _abi.R_US, _abi.R_KGAIN))
    again = problem.policy_rollout(xs.permute(1, 0, 2), us.permute(1, 0, 2), K.permute(1, 0, 2, 3), S, **pert)
    gc.same_bits(again.cost, res.cost, "the stored policy given explicitly")
