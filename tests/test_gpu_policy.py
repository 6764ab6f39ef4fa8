"""aslr_policy_rollout on the GPU (include/aslr_to_amd_policy.h; policy_rollout_kernel, csrc/aslr_policy.inc.hpp) against
tests/_policy.py: the definition as a numpy loop over the oracle's knot evaluation, fed the DEVICE's own gains so that only
the roll-out is compared.

Kernel outputs are held to 1e-9 relative, the per-kernel bound of the parity suites (max |a - b| / (1 + |b|));
tests/test_policy_host.py shows that the inputs are conditioned for it.  Shapes (tests/_policy.CASES): the smallest that
leave a partial wave of teams (B = 5) and a sample group with one live lane (S = 17), the smallest problem there is, and a
full wave.  Every output sits in a buffer of the test's own, followed by guard words that must survive."""
import numpy as np
import pytest

import _ext_call as ext
import _gpu_case as gc
import _policy as pol
from aslr_to_amd import _abi, crocoddyl, scenarios

pytestmark = pytest.mark.gpu

FIELDS = ext.POLICY_FIELDS


def _raw(e, *args, **kw):
    """ext.policy_rollout(e, "aslr_policy_rollout", S, pert=None, clamp=False, which=FIELDS, expect=OK)"""
    return ext.policy_rollout(e, "aslr_policy_rollout", *args, **kw)


@pytest.fixture(scope="module")
def cases(oracle):
    """the seeded inputs of every case, built once (the open-loop candidate comes from the oracle) and never changed"""
    return {key: pol.case(oracle, key) for key in pol.CASES}


@pytest.mark.parametrize("key", sorted(pol.CASES))
def test_kernel_matches_the_definition(oracle, cases, monkeypatch, key):
    c = cases[key]
    low, S = c["low"], c["S"]
    e, K = ext.with_gains(c, monkeypatch)
    got = _raw(e, S, c["pert"], c["clamp"])
    want = pol.rollout(oracle, low, c["xs"], c["us"], K, S, clamp=c["clamp"], **c["pert"])
    assert (want["failed_knot"] == -1).all()
    np.testing.assert_array_equal(got["failed_knot"], want["failed_knot"])
    assert np.abs(want["xs"] - c["xs"].transpose(1, 0, 2)[:, None]).max() > 1e-3   # the perturbations moved the loop
    for k in pol.OUTPUTS:
        gc._assert_close("%s %s" % (key, k), got[k], want[k], 1e-9)
    if c["clamp"]:
        assert want["bound"].any() and not want["bound"].all(), "the narrowed box must bind on some samples"
        free = pol.rollout(oracle, low, c["xs"], c["us"], K, S, clamp=False, **c["pert"])
        assert gc.relerr(free["us"], want["us"]) > 1e-3     # ... and the clamp is what the kernel applied
    if getattr(low, "ref_path", None) is not None:   # ... and the path is what the costs were evaluated against
        plain = scenarios.lower(dict(c["sc"], ref_path=None))
        assert gc.relerr(pol.rollout(oracle, plain, c["xs"], c["us"], K, S, **c["pert"])["cost"], want["cost"]) > 1e-6


def test_without_perturbations_a_solution_rolls_out_onto_itself(oracle):
    """After a converged SolverBoxDDP solve (B = 5, T = 9; the stiffness box is active), every input NULL, S = 2, clamp on:
    xs_closed is XS and us_closed is US, bit for bit, for both samples -- the property that keeps rolled-out candidates gap
    free; the cost is TF_COST within 1e-12 relative and no sample fails."""
    sc = scenarios.two_dof_vsa_boxddp(B=5, T=9, seed=4)
    low, sp = scenarios.lower(sc), scenarios.solver_params(sc)
    e, sol = gc.solve_gpu(low, sp)
    assert ((sol["traj_i"][_abi.TI_STATUS] & _abi.ST_CONVERGED) != 0).all()
    assert (sol["us"][..., 2:] == 0.0).any()    # the box is active
    got = _raw(e, 2, None, True)
    for s in range(2):
        np.testing.assert_array_equal(got["xs"][:, s].view(np.uint64), sol["xs"].transpose(1, 0, 2).copy().view(np.uint64))
        np.testing.assert_array_equal(got["us"][:, s].view(np.uint64), sol["us"].transpose(1, 0, 2).copy().view(np.uint64))
        np.testing.assert_array_equal(got["x_final"][:, s].view(np.uint64), sol["xs"][-1].copy().view(np.uint64))
        cost = sol["traj_f"][_abi.TF_COST]
        err = (np.abs(got["cost"][:, s] - cost) / np.abs(cost)).max()
        print("cost against TF_COST: %.2e relative" % err)
        assert err < 1e-12, err
    assert (got["failed_knot"] == -1).all()


@pytest.mark.parametrize("key", ["sea_table", "sea_plain", "vsa_box"])
def test_the_nominal_plant_given_explicitly_is_the_null_plant(cases, monkeypatch, key):
    """the trajectories' own K and B passed as plant arrays: the bits of passing NULL (dx0 and disturbance as in the case)"""
    c = cases[key]
    low, S = c["low"], c["S"]
    e, _ = ext.with_gains(c, monkeypatch)
    nom = lambda f: np.repeat(np.array([pol.nominal_diag(low, b, f) for b in range(low.B)])[:, None, :], S, axis=1)
    sea = low.dam == _abi.DAM_SEA
    none = dict(c["pert"], plant_stiffness=None, plant_motor_inertia=None)
    explicit = dict(none, plant_stiffness=nom("K") if sea else None, plant_motor_inertia=nom("B"))
    ext.same(_raw(e, S, explicit, c["clamp"]), _raw(e, S, none, c["clamp"]), "explicit nominal plant against NULL")
    if sea:   # ... and each plant argument alone
        ext.same(_raw(e, S, dict(none, plant_stiffness=nom("K")), c["clamp"]), _raw(e, S, none, c["clamp"]), "stiffness alone")


@pytest.mark.parametrize("key", ["sea_table", "sea_path"])
def test_a_sample_does_not_depend_on_where_it_sits(cases, monkeypatch, key):
    """sample s of trajectory b at (B, S) = (5, 17) against the same sample run alone at (1, 1), its inputs sliced out
    (its own row of the table, its own path, the batch's gains): bit for bit"""
    c = cases[key]
    sc, low, S = c["sc"], c["low"], c["S"]
    e, K = ext.with_gains(c, monkeypatch)
    batch = _raw(e, S, c["pert"])
    for b, s in ((0, 0), (3, 15), (4, 16), (4, 0), (1, 16)):
        one = dict(sc, x0=sc["x0"][b:b + 1], frame_refs=sc["frame_refs"][b:b + 1])
        one["traj_params"] = {k: (None if v is None else v[b:b + 1]) for k, v in sc["traj_params"].items()}
        if sc.get("ref_path") is not None:
            one["ref_path"] = sc["ref_path"][b:b + 1]
        e1 = gc.engine(scenarios.lower(one))
        gc._upload(e1, XS=c["xs"][:, b:b + 1], US=c["us"][:, b:b + 1], KGAIN=K[:, b:b + 1])
        alone = _raw(e1, 1, {k: (None if v is None else v[b:b + 1, s:s + 1]) for k, v in c["pert"].items()})
        ext.same({k: v[0, 0] for k, v in alone.items()}, {k: v[b, s] for k, v in batch.items()}, "sample %d of trajectory %d" % (s, b))


def test_a_failing_sample_fails_alone(cases, monkeypatch):
    """one sample gets dx0 = 1e31: its failed_knot is 0 and its cost NaN; every other sample's outputs are, bit for bit,
    those of the run without it"""
    c = cases["sea_table"]
    S = c["S"]
    e, _ = ext.with_gains(c, monkeypatch)
    base = _raw(e, S, c["pert"])
    dx0 = np.array(c["pert"]["dx0"])
    dx0[2, 5] = 1e31
    got = _raw(e, S, dict(c["pert"], dx0=dx0))
    assert got["failed_knot"][2, 5] == 0 and np.isnan(got["cost"][2, 5])
    keep = np.ones((c["low"].B, S), dtype=bool)
    keep[2, 5] = False
    assert (got["failed_knot"][keep] == -1).all()
    ext.same({k: v[keep] for k, v in got.items()}, {k: v[keep] for k, v in base.items()}, "the other samples")


@pytest.mark.parametrize("key", ["sea_table", "vsa_box"])
def test_every_output_is_optional(cases, monkeypatch, key):
    """each output alone: the bits of the call with all five, and nothing written past any buffer (_raw checks the guards)"""
    c = cases[key]
    e, _ = ext.with_gains(c, monkeypatch)
    full = _raw(e, c["S"], c["pert"], c["clamp"])
    for k in FIELDS:
        alone = _raw(e, c["S"], c["pert"], c["clamp"], which=(k,))
        assert list(alone) == [k]
        ext.same(alone, {k: full[k]}, "alone")
    both = _raw(e, c["S"], c["pert"], c["clamp"], which=("xs", "us"))
    ext.same(both, {k: full[k] for k in both}, "trajectories only")


def test_the_call_leaves_a_solve_in_progress_as_it_was(cases):
    """3 iterations, the call (all inputs, all outputs), 3 more iterations: XS, US, TRAJ_F and TRAJ_I are, bit for bit, those
    of 6 iterations on a fresh engine"""
    c = cases["vsa_box"]
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


def test_refusals_write_nothing_and_leave_a_live_handle(cases, monkeypatch):
    c = cases["vsa_box"]
    e, _ = ext.with_gains(c, monkeypatch)
    S = c["S"]
    ok = _raw(e, S, c["pert"], True)
    for bad_s in (0, -3):
        msg = _raw(e, bad_s, None, expect=_abi.E_INVALID)
        assert msg.startswith("aslr_policy_rollout:") and "n_samples" in msg, msg
    msg = _raw(e, S, c["pert"], which=(), expect=_abi.E_INVALID)
    assert msg.startswith("aslr_policy_rollout:") and "NULL" in msg, msg
    stiff = dict(c["pert"], plant_stiffness=np.ones((c["low"].B, S, 2)))
    msg = _raw(e, S, stiff, expect=_abi.E_INVALID)
    assert msg.startswith("aslr_policy_rollout:") and "VSA" in msg, msg
    ext.same(_raw(e, S, c["pert"], True), ok, "the handle after the refusals")
    # K that is not diagonal: refused with a plant argument, rolled out without one
    low = scenarios.lower(scenarios.two_dof_sea(B=2, T=3, seed=4))
    for i in range(low.desc.nmodels):   # (the lowered description is what aslr_problem_create reads)
        low.desc.models[i].K[1] = low.desc.models[i].K[2] = 0.1
    e2 = gc.engine(low)
    msg = _raw(e2, 2, dict(plant_motor_inertia=np.full((2, 2, 2), 1e-2)), expect=_abi.E_INVALID)
    assert msg.startswith("aslr_policy_rollout:") and "diagonal" in msg, msg
    assert np.isfinite(_raw(e2, 2, None)["cost"]).all()
    # a 7-joint handle
    e7 = gc.engine(scenarios.lower(scenarios.talos_arm_sea(B=2, T=3, seed=4)))
    msg = _raw(e7, 2, None, expect=_abi.E_INVALID)
    assert msg.startswith("aslr_policy_rollout:") and "7-joint" in msg, msg


def test_python_facade(cases, monkeypatch):
    """solver.policy_rollout on two_dof_sea: the documented shapes, and the bits of the raw call on the same engine; clamp
    None follows the solver class; problem.policy_rollout at a stored policy puts the engine's own back;
    double_pendulum_nu1 returns us with nu = 1"""
    import torch
    B, T, S = 3, 8, 5
    sc = scenarios.two_dof_sea(B=B, T=T, seed=4)
    problem = crocoddyl.ShootingProblem(sc["x0"], sc["running"], sc["terminal"], frame_refs=sc["frame_refs"])
    solver = crocoddyl.SolverDDP(problem)
    solver.solve([], [], 20)
    low = problem.engine.low
    pert = pol.perturbations(low, S, 29)
    res = solver.policy_rollout(S, keep_trajectories=True, **pert)
    gc.sync()
    assert tuple(res.cost.shape) == (B, S) and tuple(res.failed_knot.shape) == (B, S) and res.failed_knot.dtype == torch.int32
    assert tuple(res.x_final.shape) == (B, S, 8) and tuple(res.xs.shape) == (B, S, T + 1, 8) and tuple(res.us.shape) == (B, S, T, 2)
    raw = _raw(problem.engine, S, pert)
    for k in FIELDS:
        a = gc.to_np(getattr(res, k))
        np.testing.assert_array_equal(a.view(np.uint64) if a.dtype == np.float64 else a,
                                      raw[k].view(np.uint64) if raw[k].dtype == np.float64 else raw[k], err_msg=k)
    lean = solver.policy_rollout(S, **pert)
    assert lean.xs is None and lean.us is None
    gc.same_bits(lean.cost, res.cost, "costs without the trajectories")
    # ... at a stored policy, through the problem: the same bits, and the engine's own policy is back afterwards
    e = problem.engine
    xs, us, K = (e.region(r).clone() for r in (_abi.R_XS, _abi.R_US, _abi.R_KGAIN))
    e.region(_abi.R_KGAIN).zero_()
    again = problem.policy_rollout(xs.permute(1, 0, 2), us.permute(1, 0, 2), K.permute(1, 0, 2, 3), S, **pert)
    gc.same_bits(again.cost, res.cost, "the stored policy given explicitly")
    assert (e.region(_abi.R_KGAIN) == 0).all()
    # padded controls are cut
    c = cases["pendulum_nu1_3d"]
    psc = c["sc"]
    pp = crocoddyl.ShootingProblem(psc["x0"], psc["running"], psc["terminal"], frame_refs=psc["frame_refs"])
    ps = crocoddyl.SolverDDP(pp)
    ps.solve([], [], 3)
    r1 = ps.policy_rollout(c["S"], dx0=c["pert"]["dx0"], keep_trajectories=True)
    gc.sync()
    assert tuple(r1.us.shape) == (5, c["S"], c["low"].T, 1) and tuple(r1.xs.shape) == (5, c["S"], c["low"].T + 1, 8)
    assert crocoddyl.SolverBoxDDP(problem).policy_rollout(S).cost.shape == (B, S)
