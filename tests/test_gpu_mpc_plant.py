"""aslr_mpc_run_plant on the GPU (include/aslr_to_amd_mpc_plant.h; mpc_plant_kernel, csrc/aslr_mpc_plant.inc.hpp;
mpc_advance_kernel, csrc/aslr_abi.hip) against tests/_mpc_plant.py; the assertion bodies shared with
tests/test_gpu_mpc_plant_team.py are tests/_mpc_plant_gpu.py's.

The oracle's solve returns no gains, so the call is held to its definition by induction: ONE control step against the
definition (a twin handle's plain solve gives the plan and the gains; the plant phase is a numpy loop over the oracle's
knot), then the loop against itself, bit for bit; at hold = 1, where no gain is read, the whole loop against the oracle's.
Kernel outputs are held to 1e-9 relative, max |a - b| / (1 + |b|), the bound of the policy suite.  Every output sits in a
guarded buffer of tests/_ext_call.py."""
import numpy as np
import pytest

import _ext_call as ext
import _gpu_case as gc
import _mpc_plant as mp
import _mpc_plant_gpu as mg
import _policy as pol
import _ref_path
import test_mpc_host as H
from aslr_to_amd import _abi, crocoddyl, scenarios

pytestmark = pytest.mark.gpu

AFTER = "after a refused aslr_mpc_run_plant"


def _raw(e, *args, **kw):
    """ext.mpc_run_plant(e, "aslr_mpc_run_plant", sp, n, first, per, hold=1, pk=None, pb=None, dist=None, clamp=False,
    cost=True, failed=True, expect=OK)"""
    return ext.mpc_run_plant(e, "aslr_mpc_run_plant", *args, **kw)


# ---- 1. one control step is the definition ----
def _sea(B, T):
    return scenarios.two_dof_sea(B=B, T=T, seed=4)


def _vsa_box():
    """two_dof_vsa_boxddp with tests/_policy.scenario's table (seed 5) and narrowed box, B = 5, T = 4, scenario seed 14.  The
    seed was chosen on the REFERENCE's `bound` alone (mp.plant_phase fed a plain solve's plan and gains): after three BoxDDP
    iterations the controls on the box have zero gain rows and the free ones sit inside it, so with hold = 2 (one feedback
    knot) the narrowed box moves no control of the reference at 23 of the scenario seeds 0..23 -- _policy.scenario's own
    seed 4 among them -- and one control of one trajectory, by 0.11, at seed 14."""
    sc = scenarios.with_traj_params(scenarios.two_dof_vsa_boxddp(B=5, T=4, seed=14), seed=5)
    sc["traj_params"]["u_lb"] = np.tile(np.array(pol.BOX_LB), (5, 1))
    sc["traj_params"]["u_ub"] = np.tile(np.array(pol.BOX_UB), (5, 1))
    return sc


ONE_STEP = {
    "sea_B5_T3_hold1": (lambda: _sea(5, 3), 1, {}),
    "sea_B65_T3_hold2": (lambda: _sea(65, 3), 2, {}),
    "sea_B5_T3_hold3": (lambda: _sea(5, 3), 3, {}),
    "sea_table": (lambda: pol.scenario("two_dof_sea", 5, 4, True, False), 2, dict(plants=False)),
    "sea_table_and_plants": (lambda: pol.scenario("two_dof_sea", 5, 4, True, False), 2, dict(plants_win=True)),
    "sea_path": (lambda: pol.scenario("two_dof_sea", 5, 5, False, True), 2, {}),
    "vsa_box": (_vsa_box, 2, dict(clamp=True)),
    "pendulum_3d": (lambda: pol.scenario("double_pendulum", 5, 3, False, False), 2, dict(three_d=True)),
}


@pytest.mark.parametrize("key", sorted(ONE_STEP))
def test_one_control_step_is_the_definition(oracle, monkeypatch, key):
    """n_steps = 1, three SolverFDDP / SolverBoxDDP iterations from the empty candidate, plants within +-30 %, disturbance
    U(-1e-3, 1e-3): the records, the cost and failed_knot against mp.plant_phase on the twin's XS / US / KGAIN; the shifted
    plan, X0 and the statistics exactly; KFF, GAPS, VXXF zero.  B = 5 leaves a partial wave, B = 65 crosses one; hold = 3 = T
    is the shift whose every source is the clamped last row."""
    make, hold, opt = ONE_STEP[key]
    if opt.get("three_d"):
        monkeypatch.setenv("ASLR_NO_PLANAR", "1")   # (read when the handle is created: the general 3-D chain path)
    sc = make()
    low = scenarios.lower(sc)
    vsa = low.dam == _abi.DAM_VSA
    sp = scenarios.solver_params(sc, solver="SolverBoxDDP" if vsa else "SolverFDDP", maxiter=3)
    clamp = bool(opt.get("clamp"))
    B, T = low.B, low.T
    pk, pb = mp.plants(low, seed=21, rng_range=0.3) if opt.get("plants", True) else (None, None)
    dist = np.random.default_rng(7).uniform(-1e-3, 1e-3, (hold, B, low.nx))
    e, twin = ext.fresh(low), ext.fresh(low)
    row_before = e.reference_row
    got = _raw(e, sp, 1, 3, 3, hold, pk, pb, dist, clamp)
    twin.solve(sp, poll_every=0)
    gc.sync()
    X, U, K = (gc.to_np(twin.region(r)) for r in (_abi.R_XS, _abi.R_US, _abi.R_KGAIN))
    assert (gc.to_np(twin.traj_i(_abi.TI_ITER)) >= 1).any() and (hold == 1 or np.abs(K[1:hold]).max() > 1e-3)
    pick = lambda a, b: None if a is None else a[b]
    ref = [mp.plant_phase(oracle, low, b, X[:, b], U[:, b], K[:, b], hold, pick(pk, b), pick(pb, b), dist[:, b], clamp)
           for b in range(B)]
    want_x, want_u = np.stack([r["x"] for r in ref], axis=1), np.stack([r["u"] for r in ref], axis=1)
    want_c, want_f = np.array([r["cost"] for r in ref]), np.array([r["failed"] for r in ref], dtype=np.int32)
    assert (want_f == -1).all()
    errs = dict(x=gc.relerr(got["x"], want_x), u=gc.relerr(got["u"], want_u), cost=gc.relerr(got["cost"], want_c))
    print("%s: relerr %s" % (key, {k: "%.2e" % v for k, v in errs.items()}))
    assert max(errs.values()) < 1e-9, errs
    np.testing.assert_array_equal(got["failed"], want_f)
    if hold > 1:   # the plant and the disturbance moved the loop off the plan, so the feedback term was at work
        assert np.abs(got["x"][1:hold] - X[1:hold]).max() > 1e-6
    if clamp:
        assert any(r["bound"] for r in ref), "the narrowed box must move some control of the reference"
        free = [mp.plant_phase(oracle, low, b, X[:, b], U[:, b], K[:, b], hold, pick(pk, b), pick(pb, b), dist[:, b], False)
                for b in range(B)]
        assert gc.relerr(np.stack([r["u"] for r in free], axis=1), want_u) > 1e-3   # ... and the clamp is what the kernel applied
    if opt.get("plants_win"):   # the plants given on top of the table are what the kernel used, not the table's rows
        table = [mp.plant_phase(oracle, low, b, X[:, b], U[:, b], K[:, b], hold, None, None, dist[:, b], clamp) for b in range(B)]
        assert gc.relerr(np.stack([r["x"] for r in table], axis=1), want_x) > 1e-6
    mg.one_step_leaves_the_shifted_plan(e, twin, low, got, X, U, hold, clamp, row_before)


# ---- 2. the loop is its own step, bit for bit ----
def test_the_loop_is_its_own_step_bit_for_bit():
    B, T, n, hold, first, per = 64, 20, 4, 2, 6, 2
    sc = scenarios.two_dof_sea(B=B, T=T)
    sc = _ref_path.with_path(sc, _ref_path.random_path(sc, 30, 13), row0=0)
    low = scenarios.lower(sc)
    sp = scenarios.solver_params(sc, solver="SolverFDDP", maxiter=400)
    pk, pb = mp.plants(low, seed=21, rng_range=0.3)
    dist = np.random.default_rng(7).uniform(-1e-3, 1e-3, (n * hold, B, low.nx))
    dev, twin = mg.the_loop_is_its_own_step(_raw, low, sp, n, hold, first, per, pk, pb, dist, "two_dof_sea")
    assert dev.reference_row == twin.reference_row == n * hold


def test_a_failing_trajectory_fails_alone_and_is_counted_in_applied_knots():
    """n_steps = 2, hold = 2 (two_dof_sea, B = 5, T = 4).  Trajectory 1 is pushed by 1e31 after applied knot 0, trajectory 3
    after applied knot 1: the next knot's plant state then fails the solver's test, so failed_knot is 1 (inside step 0) and 2
    (the first knot of step 1: the index counts applied knots over the steps, not knots of the step); both costs are NaN,
    through the second step as well; a plant inertia of 0 on trajectory 4 fails at knot 0.  Every other trajectory has, bit
    for bit, the outputs of the run without the failures."""
    sc = _sea(5, 4)
    low = scenarios.lower(sc)
    sp = scenarios.solver_params(sc, solver="SolverFDDP", maxiter=400)
    n, hold = 2, 2
    pk, pb = mp.plants(low, seed=21, rng_range=0.3)
    dist = np.random.default_rng(7).uniform(-1e-3, 1e-3, (n * hold, 5, low.nx))
    base = _raw(ext.fresh(low), sp, n, 3, 2, hold, pk, pb, dist)
    pushed, pb0 = np.array(dist), np.array(pb)
    pushed[0, 1], pushed[1, 3], pb0[4] = 1e31, 1e31, 0.0
    got = _raw(ext.fresh(low), sp, n, 3, 2, hold, pk, pb0, pushed)
    mg.a_failing_trajectory_fails_alone(base, got, [-1, 1, -1, 2, 0], before=(2, 3))


# ---- 3. the oracle loop at hold = 1 on a mismatched plant ----
@pytest.mark.parametrize("row", mp.ROWS, ids=mp.ROW_IDS)
def test_hold_one_matches_the_oracle_loop_on_a_mismatched_plant(oracle, row):
    """the rows tests/test_mpc_plant_host.py holds to the stability criterion; the bounds of
    test_gpu_mpc.test_closed_loop_matches_the_oracle_loop: iteration counts and status words exactly, states, controls and
    the final plan within 1e-6 of the trajectory's scale, step costs and the closed cost within 1e-4 of max(1, |cost|)"""
    mg.hold_one_matches_the_oracle_loop(oracle, row, H)


# ---- 4. delegation and neutrality ----
def _table_case(B=64, T=20):
    """the recipe of tests/test_gpu_mpc.py's _table_case"""
    sc = scenarios.with_traj_params(scenarios.two_dof_vsa_boxddp(B=B, T=T), seed=4, stiffness_floors=(0.0, 0.002))
    rng = np.random.default_rng(5)
    tp = sc["traj_params"]
    tp["u_ub"] = rng.uniform(50.0, 100.0, tp["u_ub"].shape)
    tp["u_lb"][:, :2] = -rng.uniform(50.0, 100.0, (B, 2))
    return sc


def test_defaults_are_aslr_mpc_run_bit_for_bit():
    sc = _table_case()
    low = scenarios.lower(sc)
    sp = scenarios.solver_params(sc, maxiter=400)
    mg.defaults_are_aslr_mpc_run(_raw, low, sp, 4, 6, 2)


@pytest.mark.parametrize("case", ["sea", "vsa_table"])
def test_the_nominal_plant_is_neutral_and_a_plant_off_is_not(case):
    """ONE step with the trajectories' own K and B passed as plant arrays and the cost requested: x_closed[1] within 1e-11 of
    the trajectory's scale of aslr_mpc_run's (the calc and the plant instantiations need not share bits, and a longer loop
    would amplify the difference); with the plant 20 % off it moves by more than 1e-6."""
    sc = _sea(65, 6) if case == "sea" else _table_case()
    low = scenarios.lower(sc)
    sp = scenarios.solver_params(sc, solver="SolverFDDP" if case == "sea" else "SolverBoxDDP", maxiter=400)
    mg.the_nominal_plant_is_neutral_and_a_plant_off_is_not(_raw, low, sp, 6, 2, case)


# ---- 5. schedule independence ----
def test_results_do_not_depend_on_subshards_or_batch():
    sc = _sea(65, 6)
    low = scenarios.lower(sc)
    sp = scenarios.solver_params(sc, solver="SolverFDDP", maxiter=400)
    n, hold, first, per = 3, 2, 6, 2
    pk, pb = mp.plants(low, seed=21, rng_range=0.3)
    dist = np.random.default_rng(7).uniform(-1e-3, 1e-3, (n * hold, 65, low.nx))
    e1, r1 = mg.two_subshards_give_the_same_bits(_raw, low, sp, n, first, per, hold, pk, pb, dist)
    five = dict(sc, x0=sc["x0"][:5], frame_refs=sc["frame_refs"][:5])
    e3 = ext.fresh(scenarios.lower(five))
    r3 = _raw(e3, sp, n, first, per, hold, pk[:5], pb[:5], dist[:, :5])
    mg.the_head_of_a_batch_is_a_batch_of_its_own(e1, r1, e3, r3, 5)


# ---- 6. refusals ----
def _refused(e, sp, word, *args, **kw):
    msg = _raw(e, sp, *args, expect=_abi.E_INVALID, **kw)
    assert msg.startswith("aslr_mpc_run_plant:") and word in msg, msg


def test_refusals_enqueue_nothing_and_leave_the_handle_usable():
    import copy
    sc = _sea(4, 6)
    sp = scenarios.solver_params(sc, solver="SolverFDDP", maxiter=20)
    low = scenarios.lower(sc)
    e = ext.fresh(low)
    ones = np.ones((4, 2))
    # what aslr_mpc_run refuses
    for args in ((0, 5, 2), (2, 0, 2), (2, 5, 0)):
        _refused(e, sp, "n_steps, first_maxiter and iters_per_step must be >= 1", *args, hold=2)
    e.enable_iteration_log(20)
    _refused(e, sp, "an iteration log is set", 2, 5, 2, hold=2)
    e.enable_iteration_log(0)
    # the hold
    for hold in (0, -1, 7):
        _refused(e, sp, "hold", 2, 5, 2, hold=hold)
    ext.solve_matches_a_fresh_handle(e, low, sp, ext.SOLVE_REGIONS, AFTER)
    assert _raw(e, sp, 2, 5, 2, 6, ones, 1e-2 * ones)["x"].shape == (13, 4, 8)   # (hold = T runs, on the same handle)
    # two distinct running models
    mixed = dict(sc)
    mixed["running"] = [sc["running"][0]] * 3 + [copy.copy(sc["running"][0])] * 3
    lowm = scenarios.lower(mixed)
    em = ext.fresh(lowm)
    _refused(em, sp, "more than one action model", 2, 5, 2, hold=2)
    ext.solve_matches_a_fresh_handle(em, lowm, sp, ext.SOLVE_REGIONS, AFTER)
    # plant_stiffness on a VSA model
    scv = scenarios.two_dof_vsa_boxddp(B=4, T=6, seed=4)
    lowv, spv = scenarios.lower(scv), scenarios.solver_params(scv, maxiter=20)
    ev = ext.fresh(lowv)
    _refused(ev, spv, "VSA", 2, 5, 2, hold=2, pk=ones)
    ext.solve_matches_a_fresh_handle(ev, lowv, spv, ext.SOLVE_REGIONS, AFTER)
    # K that is not diagonal: refused with a plant argument, run without one
    lown = scenarios.lower(_sea(2, 3))
    for i in range(lown.desc.nmodels):   # (the lowered description is what aslr_problem_create reads)
        lown.desc.models[i].K[1] = lown.desc.models[i].K[2] = 0.1
    en = ext.fresh(lown)
    _refused(en, sp, "diagonal", 2, 5, 2, hold=2, pb=np.full((2, 2), 1e-2))
    assert np.isfinite(_raw(en, sp, 2, 5, 2, 2)["cost"]).all()
    # a 7-joint handle
    sc7 = scenarios.talos_arm_sea(B=2, T=4, seed=4)
    low7, sp7 = scenarios.lower(sc7), scenarios.solver_params(sc7, maxiter=10)
    e7 = ext.fresh(low7)
    _refused(e7, sp7, "7-joint", 2, 5, 2, hold=2)
    _refused(e7, sp7, "nx = 8", 2, 5, 2, hold=1, cost=False, failed=False)
    ext.solve_matches_a_fresh_handle(e7, low7, sp7, ext.SOLVE_REGIONS, AFTER)
    # (7, VSA) with SolverDDP: aslr_mpc_run's refusal comes first
    sc7v = scenarios.talos_arm_vsa(B=2, T=4)
    e7v = ext.fresh(scenarios.lower(sc7v))
    _refused(e7v, scenarios.solver_params(sc7v, solver="SolverDDP", maxiter=5), "built for SolverBoxDDP only", 2, 5, 2, hold=2)


# ---- 7. Python ----
def test_python_facade():
    import torch
    B, T = 3, 8
    sc = scenarios.two_dof_sea(B=B, T=T, seed=4)
    make = lambda cls: cls(crocoddyl.ShootingProblem(sc["x0"], sc["running"], sc["terminal"], frame_refs=sc["frame_refs"]))
    solver = make(crocoddyl.SolverFDDP)
    pb = 1.2 * np.array([pol.nominal_diag(solver.problem.engine.low, b, "B") for b in range(B)])
    r = solver.solve_mpc(3, 2, maxiter=6, hold=2, plant_motor_inertia=pb, closed_cost=True)
    assert tuple(r.xs_closed.shape) == (B, 7, 8) and tuple(r.us_closed.shape) == (B, 6, 2)
    assert tuple(r.closed_cost.shape) == (B,) and tuple(r.failed_knot.shape) == (B,) and r.failed_knot.dtype == torch.int32
    assert r.hold == 2 and tuple(r.iters.shape) == (B, 3) and tuple(r.cost.shape) == (B, 3)
    assert torch.isfinite(r.closed_cost).all() and (r.failed_knot == -1).all()
    # the defaults: Engine.mpc_run, an MpcResult with exactly the fields it had
    plain = make(crocoddyl.SolverFDDP).solve_mpc(3, 2, maxiter=6)
    assert sorted(plain.__dict__) == sorted(("xs_closed", "us_closed", "iters", "status", "cost", "stop", "x_reg", "step",
                                             "reference_row"))
    assert tuple(plain.xs_closed.shape) == (B, 4, 8)
    lean = make(crocoddyl.SolverFDDP).solve_mpc(3, 2, maxiter=6, hold=2)
    assert lean.closed_cost is None and tuple(lean.xs_closed.shape) == (B, 7, 8)
    # clamp=None follows the solver class: SolverBoxDDP clamps the feedback control to the (narrowed) box, clamp=False does not
    scv = pol.scenario("two_dof_vsa_boxddp", 5, 6, True, False)
    tp = scv["traj_params"]
    makev = lambda: crocoddyl.SolverBoxDDP(crocoddyl.ShootingProblem(scv["x0"], scv["running"], scv["terminal"],
                                                                     frame_refs=scv["frame_refs"], **tp))
    pbv = 1.3 * np.asarray(tp["motor_inertia"])
    runs = {c: makev().solve_mpc(2, 3, maxiter=3, hold=3, plant_motor_inertia=pbv, clamp=c) for c in (None, True, False)}
    gc.same_bits(runs[None].us_closed, runs[True].us_closed, "clamp=None under SolverBoxDDP is clamp=True")
    box = lambda v: torch.as_tensor(v, dtype=torch.float64, device=runs[True].us_closed.device)
    lb, ub = box(pol.BOX_LB), box(pol.BOX_UB)
    assert ((runs[True].us_closed >= lb) & (runs[True].us_closed <= ub)).all()
    under_fddp = make(crocoddyl.SolverFDDP).solve_mpc(2, 3, maxiter=3, hold=3, plant_motor_inertia=pb)
    gc.same_bits(under_fddp.us_closed,
                 make(crocoddyl.SolverFDDP).solve_mpc(2, 3, maxiter=3, hold=3, plant_motor_inertia=pb, clamp=False).us_closed,
                 "clamp=None under SolverFDDP is clamp=False")
