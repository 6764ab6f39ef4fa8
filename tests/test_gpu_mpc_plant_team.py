"""aslr_mpc_run_plant_all on the GPU (include/aslr_to_amd_mpc_plant_all.h; mpc_plant_team_kernel,
csrc/aslr_mpc_plant_team.inc.hpp) against tests/_mpc_plant.py, on the 7-joint arms.

As tests/test_gpu_mpc_plant.py: the oracle's solve returns no gains, so the call is held to its definition by induction --
ONE control step against the definition (a twin handle's plain solve gives the plan and the gains; the plant phase is a numpy
loop over the oracle's knot), then the loop against itself, bit for bit; at hold = 1, where no gain is read, the whole loop
against the oracle's.  Kernel outputs are held to 1e-9 relative, max |a - b| / (1 + |b|); tests/test_mpc_plant_team_host.py
shows that the inputs are conditioned for it.  Shapes: tests/_mpc_plant_team.py.  Every output sits in a guarded buffer of
tests/_ext_call.py."""
import copy
import ctypes as C

import numpy as np
import pytest

import _ext_call as ext
import _gpu_case as gc
import _mpc_plant as mp
import _mpc_plant_gpu as mg
import _mpc_plant_team as mt
import _policy as pol
import _policy_team as pt
import _traj_oracle
import test_mpc_host as H
from aslr_to_amd import _abi, crocoddyl, scenarios

pytestmark = pytest.mark.gpu

NAME = mt.NAME
AFTER = "after a refused " + NAME


def _raw(e, *args, name=NAME, **kw):
    """ext.mpc_run_plant(e, name, sp, n, first, per, hold=1, pk=None, pb=None, dist=None, clamp=False, cost=True, failed=True,
    expect=OK)"""
    return ext.mpc_run_plant(e, name, *args, **kw)


def _arm(name, B, T):
    sc = scenarios.SCENARIOS[name](B=B, T=T, seed=mt.SCENARIO_SEED)
    low = scenarios.lower(sc)
    sp = scenarios.solver_params(sc, solver="SolverBoxDDP" if low.dam == _abi.DAM_VSA else "SolverFDDP", maxiter=3)
    return sc, low, sp


def _plants_and_noise(low, N):
    pk, pb = mp.plants(low, seed=mt.PLANT_SEED, rng_range=mt.PLANT_RANGE)
    return pk, pb, np.random.default_rng(mt.DIST_SEED).uniform(-mt.DIST, mt.DIST, (N, low.B, low.nx))


# ---- 1. one control step is the definition ----
@pytest.mark.parametrize("key", sorted(mt.ONE_STEP))
def test_one_control_step_is_the_definition(oracle, key):
    """n_steps = 1, three SolverFDDP / SolverBoxDDP iterations from the empty candidate, plants within +-30 %, disturbance
    U(-1e-3, 1e-3): the records, the cost and failed_knot against mp.plant_phase on the twin's XS / US / KGAIN within 1e-9;
    the shifted plan, X0 and the statistics exactly; KFF, GAPS, VXXF zero.  B = 3 leaves five idle teams, B = 9 crosses a
    wave (= a block); hold = 4 = T is the shift whose every source is the clamped last row; vsa_box runs T = 6, hold = 6
    (tests/_mpc_plant_team.py says why)."""
    c = mt.one_step(key)
    low, sp, hold, clamp, pk, pb, dist = (c[k] for k in ("low", "sp", "hold", "clamp", "pk", "pb", "dist"))
    e, twin = ext.fresh(low), ext.fresh(low)
    row_before = e.reference_row
    got = _raw(e, sp, 1, 3, 3, hold, pk, pb, dist, clamp)
    twin.solve(sp, poll_every=0)
    gc.sync()
    X, U, K = (gc.to_np(twin.region(r)) for r in (_abi.R_XS, _abi.R_US, _abi.R_KGAIN))
    assert (gc.to_np(twin.traj_i(_abi.TI_ITER)) >= 1).any() and (hold == 1 or np.abs(K[1:hold]).max() > 1e-3)
    want = mt.reference(oracle, c, X, U[..., :low.nu], K[..., :low.nu, :])
    assert (want["failed"] == -1).all()
    errs = dict(x=gc.relerr(got["x"], want["x"]), u=gc.relerr(got["u"][..., :low.nu], want["u"]), cost=gc.relerr(got["cost"], want["cost"]))
    print("%s: relerr %s" % (key, {k: "%.2e" % v for k, v in errs.items()}))
    assert max(errs.values()) < 1e-9, errs
    np.testing.assert_array_equal(got["failed"], want["failed"])
    if hold > 1:   # the plant and the disturbance moved the loop off the plan, so the feedback term was at work
        assert np.abs(got["x"][1:hold] - X[1:hold]).max() > 1e-6
    if clamp:
        assert want["bound"].any() and not want["bound"].all(), "the narrowed box must move some control of the reference, not on every trajectory"
        free = mt.reference(oracle, c, X, U[..., :low.nu], K[..., :low.nu, :], clamp=False)
        assert gc.relerr(free["u"], want["u"]) > 1e-3   # ... and the clamp is what the kernel applied
    if c["table"] and c["arrays"]:   # the plants given on top of the table are what the kernel used, not the table's rows
        table = mt.reference(oracle, c, X, U[..., :low.nu], K[..., :low.nu, :], plants=False)
        assert gc.relerr(table["x"], want["x"]) > 1e-6
    mg.one_step_leaves_the_shifted_plan(e, twin, low, got, X, U, hold, clamp, row_before)


# ---- 2. the loop is its own step, bit for bit ----
@pytest.mark.parametrize("name", ["talos_arm_sea", "talos_arm_vsa"])
def test_the_loop_is_its_own_step_bit_for_bit(name):
    """one call of three control steps against three calls of one, hold = 2, B = 9, T = 6"""
    n, hold, first, per = 3, 2, 3, 2
    sc, low, sp = _arm(name, 9, 6)
    pk, pb, dist = _plants_and_noise(low, n * hold)
    mg.the_loop_is_its_own_step(_raw, low, sp, n, hold, first, per, pk, pb, dist, name)


# ---- 3. the oracle loop at hold = 1 on a mismatched plant ----
@pytest.mark.parametrize("row", mt.ROWS, ids=mt.ROW_IDS)
def test_hold_one_matches_the_oracle_loop_on_a_mismatched_plant(oracle, row):
    """the rows tests/test_mpc_plant_team_host.py holds to the stability criterion; the bounds of
    test_gpu_mpc_plant's test of the same name: iteration counts and status words exactly, states, controls and the final
    plan within 1e-6 of the trajectory's scale, step costs and the closed cost within 1e-4 of max(1, |cost|)"""
    mg.hold_one_matches_the_oracle_loop(oracle, row, H)


# ---- 4. delegation and neutrality ----
def test_defaults_are_aslr_mpc_run_bit_for_bit():
    """hold = 1 and nothing asked of the plant on a 7-joint handle: records, statistics and the regions of aslr_mpc_run"""
    sc, low, sp = _arm("talos_arm_sea", 9, 6)
    mg.defaults_are_aslr_mpc_run(_raw, low, sp, 3, 3, 2)


@pytest.mark.parametrize("name", ["talos_arm_sea", "talos_arm_vsa"])
def test_the_nominal_plant_is_neutral_and_a_plant_off_is_not(name):
    """ONE step with the trajectories' own K and B passed as plant arrays and the cost requested: x_closed[1] within 1e-11 of
    the trajectory's scale of aslr_mpc_run's (the calc and the plant kernels need not share bits); with the plant 20 % off
    it moves by more than 1e-6."""
    sc, low, sp = _arm(name, 9, 6)
    mg.the_nominal_plant_is_neutral_and_a_plant_off_is_not(_raw, low, sp, 3, 2, name)


# ---- 5. schedule and position independence ----
def test_results_do_not_depend_on_subshards_or_batch():
    """one and two sub-shards give the same bits (B = 65: the sub-shard boundary lies on a multiple of 64 trajectories);
    trajectories 0..2 of a batch of 9 equal a batch of 3"""
    n, hold, first, per = 2, 2, 3, 2
    sc, low, sp = _arm("talos_arm_sea", 65, 4)
    pk, pb, dist = _plants_and_noise(low, n * hold)
    mg.two_subshards_give_the_same_bits(_raw, low, sp, n, first, per, hold, pk, pb, dist)
    sc9, low9, _ = _arm("talos_arm_sea", 9, 4)
    pk9, pb9, dist9 = _plants_and_noise(low9, n * hold)
    e9 = ext.fresh(low9)
    r9 = _raw(e9, sp, n, first, per, hold, pk9, pb9, dist9)
    three = dict(sc9, x0=sc9["x0"][:3], frame_refs=sc9["frame_refs"][:3])
    e3 = ext.fresh(scenarios.lower(three))
    r3 = _raw(e3, sp, n, first, per, hold, pk9[:3], pb9[:3], dist9[:, :3])
    mg.the_head_of_a_batch_is_a_batch_of_its_own(e9, r9, e3, r3, 3)


# ---- 6. a trajectory fails alone ----
@pytest.mark.parametrize("name", ["talos_arm_sea", "talos_arm_vsa"])
def test_a_failing_trajectory_fails_alone_and_is_counted_in_applied_knots(name):
    """n_steps = 2, hold = 2, B = 9 (trajectories 0..7 are the eight teams of one wave, trajectory 8 sits in the next).
    Trajectory 4 has a plant motor inertia of 0: it fails at applied knot 0.  Trajectory 2 is pushed by 1e31 behind applied
    knot 2, the first of the SECOND step: the next knot's plant state fails the solver's test, so failed_knot is 3 (the index
    counts applied knots over the steps).  Both costs are NaN.  Every other trajectory -- the six wave mates of the failing
    ones among them -- has, bit for bit, the outputs of the run without the failures."""
    n, hold = 2, 2
    sc, low, sp = _arm(name, 9, 4)
    pk, pb, dist = _plants_and_noise(low, n * hold)
    base = _raw(ext.fresh(low), sp, n, 3, 2, hold, pk, pb, dist)
    pushed, pb0 = np.array(dist), np.array(pb)
    pushed[2, 2], pb0[4] = 1e31, 0.0
    got = _raw(ext.fresh(low), sp, n, 3, 2, hold, pk, pb0, pushed)
    mg.a_failing_trajectory_fails_alone(base, got, [-1, -1, 3, -1, 0, -1, -1, -1, -1], before=(3, 2))


# ---- 7. against the other kernel ----
@pytest.mark.parametrize("name", ["talos_arm_sea", "talos_arm_vsa"])
def test_one_step_over_the_whole_horizon_is_the_policy_rollout(oracle, name):
    """n_steps = 1, hold = T, a plant and no disturbance, against aslr_policy_rollout_all on a twin handle after the same
    solve, with S = 1, the same plant and the trajectories kept.  policy_rollout_team_kernel and mpc_plant_team_kernel take
    the plant step from one place (csrc/aslr_team_step.hpp); what each still writes for itself is the control law, the fetch
    of the gains and of the plan (a stage per wave there, registers per lane here), the indexing and the cost sum.
    x_closed[0..T] against xs_closed and u_closed against us_closed bit for bit (the printed differences were exactly 0 on
    both arms before the step was shared and after); closed_cost, the roll-out's cost minus the terminal node's (the
    oracle's knot on the roll-out's last state), within 1e-9 (measured 6.9e-15 and 1.3e-15)."""
    sc, low, sp = _arm(name, 9, 4)
    B, T = low.B, low.T
    pk, pb, _ = _plants_and_noise(low, T)
    e, twin = ext.fresh(low), ext.fresh(low)
    got = _raw(e, sp, 1, 3, 3, T, pk, pb, None)
    twin.solve(sp, poll_every=0)
    roll = twin.policy_rollout(1, None if pk is None else pk[:, None], pb[:, None], keep_trajectories=True)
    gc.sync()
    assert np.abs(gc.to_np(twin.region(_abi.R_KGAIN))[1:]).max() > 1e-3
    xs = gc.to_np(roll.xs)[:, 0].transpose(1, 0, 2)
    us = gc.to_np(twin.pad_u(roll.us[:, 0])).transpose(1, 0, 2)
    ex, eu = gc.relerr(got["x"], xs), gc.relerr(got["u"], us)
    term = np.array([oracle.knot(_traj_oracle.single(low, i), int(low.node_model[T]), xs[T, i], None,
                                 frame_ref=None if low.frame_ref is None else low.frame_ref[i], diff=False)["cost"] for i in range(B)])
    ec = gc.relerr(got["cost"], gc.to_np(roll.cost)[:, 0] - term)
    print("%s: against the policy roll-out: x %.2e, u %.2e, cost %.2e" % (name, ex, eu, ec))
    assert (got["failed"] == -1).all() and (gc.to_np(roll.failed_knot) == -1).all()
    ext.same(got["x"], xs, "x_closed against xs_closed")  # (gc.same_bits on numpy arrays)
    ext.same(got["u"], us, "u_closed against us_closed")
    assert ec < 1e-9, ec
    assert np.abs(got["x"][1:] - gc.to_np(twin.region(_abi.R_XS))[1:]).max() > 1e-6   # (the plant moved the loop off the plan)


# ---- 8. 2-joint handles ----
@pytest.mark.parametrize("case", ["sea", "vsa_table"])
def test_two_joint_handles_get_the_bits_of_aslr_mpc_run_plant(case):
    n, hold, first, per = 2, 2, 3, 2
    sc = scenarios.two_dof_sea(B=5, T=4, seed=4) if case == "sea" else pol.scenario("two_dof_vsa_boxddp", 5, 4, True, False)
    low = scenarios.lower(sc)
    sp = scenarios.solver_params(sc, solver="SolverFDDP" if case == "sea" else "SolverBoxDDP", maxiter=3)
    pk, pb, dist = _plants_and_noise(low, n * hold)
    a, b = ext.fresh(low), ext.fresh(low)
    new = _raw(a, sp, n, first, per, hold, pk, pb, dist, case != "sea")
    old = _raw(b, sp, n, first, per, hold, pk, pb, dist, case != "sea", name="aslr_mpc_run_plant")
    ext.same(new, old, "aslr_mpc_run_plant_all against aslr_mpc_run_plant")
    for rid in ext.MPC_REGIONS:
        gc.same_bits(a.region(rid), b.region(rid), "region %d" % rid)
    assert (new["failed"] == -1).all() and (new["stat_i"][:, 0].max(axis=1) >= 1).all()


# ---- 9. refusals ----
def _refused(e, sp, word, *args, **kw):
    name = kw.get("name", NAME)
    msg = _raw(e, sp, *args, expect=_abi.E_INVALID, **kw)
    assert msg.startswith(name + ":") and word in msg, msg
    return msg


def test_refusals_enqueue_nothing_and_leave_the_handle_usable():
    sc, low, sp = _arm("talos_arm_sea", 3, 4)
    e = ext.fresh(low)
    ones = np.ones((3, 7))
    # what aslr_mpc_run refuses
    for args in ((0, 3, 2), (2, 0, 2), (2, 3, 0)):
        _refused(e, sp, "n_steps, first_maxiter and iters_per_step must be >= 1", *args, hold=2)
    e.enable_iteration_log(20)
    _refused(e, sp, "an iteration log is set", 2, 3, 2, hold=2)
    e.enable_iteration_log(0)
    # the hold
    for hold in (0, -1, 5):
        _refused(e, sp, "hold", 2, 3, 2, hold=hold)
    # n_steps * hold beyond INT32_MAX: refused before anything is sized by it (the small buffers here are never touched)
    small = ext.outputs(e.device, {"f": (0,), "i": (0,)}, ("f", "i"), int32=("i",))   # (GUARD words each)
    mpc = _abi.Mpc()
    mpc.n_steps, mpc.first_maxiter, mpc.iters_per_step = 2 ** 29, 3, 2
    mpc.x_closed = mpc.u_closed = mpc.stat_f = small["f"].buf.data_ptr()
    mpc.stat_i = small["i"].buf.data_ptr()
    msg = ext.call(e, NAME, [e.handle, C.byref(sp), C.byref(mpc), 4, None, None, 0, None, None, e._stream()], small, _abi.E_INVALID)
    assert msg.startswith(NAME + ":") and "overflow" in msg, msg
    ext.solve_matches_a_fresh_handle(e, low, sp, ext.SOLVE_REGIONS, AFTER)
    assert _raw(e, sp, 2, 3, 2, 4, ones * pol.nominal_diag(low, 0, "K"), ones * pol.nominal_diag(low, 0, "B"))["x"].shape == (9, 3, 28)   # (hold = T runs, on the same handle)
    # two distinct running models
    mixed = dict(sc)
    mixed["running"] = [sc["running"][0]] * 2 + [copy.copy(sc["running"][0])] * 2
    lowm = scenarios.lower(mixed)
    em = ext.fresh(lowm)
    _refused(em, sp, "more than one action model", 2, 3, 2, hold=2)
    ext.solve_matches_a_fresh_handle(em, lowm, sp, ext.SOLVE_REGIONS, AFTER)
    # plant_stiffness on a VSA model; (7, VSA) with SolverDDP: aslr_mpc_run's refusal
    scv, lowv, spv = _arm("talos_arm_vsa", 3, 4)
    ev = ext.fresh(lowv)
    _refused(ev, spv, "VSA", 2, 3, 2, hold=2, pk=ones)
    _refused(ev, scenarios.solver_params(scv, solver="SolverDDP", maxiter=3), "built for SolverBoxDDP only", 2, 3, 2, hold=2)
    ext.solve_matches_a_fresh_handle(ev, lowv, spv, ext.SOLVE_REGIONS, AFTER)
    # K that is not diagonal: refused with a plant argument, run on the model's full rows without one
    lown = scenarios.lower(scenarios.talos_arm_sea(B=3, T=4, seed=mt.SCENARIO_SEED))
    for i in range(lown.desc.nmodels):   # (the lowered description is what aslr_problem_create reads)
        lown.desc.models[i].K[1] = lown.desc.models[i].K[7] = 0.03
    en = ext.fresh(lown)
    _refused(en, sp, "diagonal", 2, 3, 2, hold=2, pb=np.full((3, 7), 1e-2))
    ext.solve_matches_a_fresh_handle(en, lown, sp, ext.SOLVE_REGIONS, AFTER)
    # the old entry point still refuses the 7-joint handle, in its own name, also when nothing is asked of the plant
    e7 = ext.fresh(low)   # (the run above moved X0 of `e`)
    msg = _refused(e7, sp, "7-joint", 2, 3, 2, hold=2, name="aslr_mpc_run_plant")
    assert "nx = 8" in msg
    _refused(e7, sp, "nx = 8", 2, 3, 2, hold=1, cost=False, failed=False, name="aslr_mpc_run_plant")
    ext.solve_matches_a_fresh_handle(e7, low, sp, ext.SOLVE_REGIONS, AFTER)


def test_a_model_that_is_not_diagonal_runs_on_its_full_rows(oracle):
    """no plant argument and no table: K with off-diagonal entries is the plant, as in policy_rollout_team_kernel -- one
    control step against mp.plant_phase within 1e-9, and the off-diagonal entries are seen (the diagonal model differs)"""
    hold = 2
    sc, low, sp = _arm("talos_arm_sea", 3, 4)
    lown = scenarios.lower(sc)
    for i in range(lown.desc.nmodels):
        lown.desc.models[i].K[1] = lown.desc.models[i].K[7] = 0.03
    dist = np.random.default_rng(mt.DIST_SEED).uniform(-mt.DIST, mt.DIST, (hold, 3, low.nx))
    e, twin = ext.fresh(lown), ext.fresh(lown)
    got = _raw(e, sp, 1, 3, 3, hold, None, None, dist)
    twin.solve(sp, poll_every=0)
    gc.sync()
    X, U, K = (gc.to_np(twin.region(r)) for r in (_abi.R_XS, _abi.R_US, _abi.R_KGAIN))
    ref = [mp.plant_phase(oracle, lown, b, X[:, b], U[:, b], K[:, b], hold, None, None, dist[:, b]) for b in range(3)]
    errs = dict(x=gc.relerr(got["x"], np.stack([r["x"] for r in ref], axis=1)), u=gc.relerr(got["u"], np.stack([r["u"] for r in ref], axis=1)),
                cost=gc.relerr(got["cost"], np.array([r["cost"] for r in ref])))
    print("not diagonal: relerr %s" % {k: "%.2e" % v for k, v in errs.items()})
    assert max(errs.values()) < 1e-9, errs
    diag = _raw(ext.fresh(low), sp, 1, 3, 3, hold, None, None, dist)
    assert np.abs(diag["x"][1] - got["x"][1]).max() > 1e-6


# ---- 10. Python ----
def test_python_facade():
    import torch
    B, T = 3, 8
    sc = scenarios.talos_arm_sea(B=B, T=T, seed=4)
    make = lambda cls, s: cls(crocoddyl.ShootingProblem(s["x0"], s["running"], s["terminal"], frame_refs=s["frame_refs"]))
    solver = make(crocoddyl.SolverFDDP, sc)
    pb = 1.2 * np.array([pol.nominal_diag(solver.problem.engine.low, b, "B") for b in range(B)])
    r = solver.solve_mpc(3, 2, maxiter=6, hold=2, plant_motor_inertia=pb, closed_cost=True)
    assert tuple(r.xs_closed.shape) == (B, 7, 28) and tuple(r.us_closed.shape) == (B, 6, 7)
    assert tuple(r.closed_cost.shape) == (B,) and tuple(r.failed_knot.shape) == (B,) and r.failed_knot.dtype == torch.int32
    assert r.hold == 2 and tuple(r.iters.shape) == (B, 3) and tuple(r.cost.shape) == (B, 3)
    assert torch.isfinite(r.closed_cost).all() and (r.failed_knot == -1).all()
    # clamp=None follows the solver class: SolverBoxDDP clamps the feedback control to the (narrowed) box
    scv = mt.scenario("talos_arm_vsa", B, T, table=True, box=True)
    tp = scv["traj_params"]
    makev = lambda: crocoddyl.SolverBoxDDP(crocoddyl.ShootingProblem(scv["x0"], scv["running"], scv["terminal"],
                                                                     frame_refs=scv["frame_refs"], **tp))
    pbv = 1.3 * np.asarray(tp["motor_inertia"])
    runs = {c: makev().solve_mpc(2, 3, maxiter=3, hold=3, plant_motor_inertia=pbv, clamp=c) for c in (None, True)}
    gc.same_bits(runs[None].us_closed, runs[True].us_closed, "clamp=None under SolverBoxDDP is clamp=True")
    box = lambda v: torch.as_tensor(v, dtype=torch.float64, device=runs[True].us_closed.device)
    lb, ub = (box(v) for v in pt.box(7))
    assert ((runs[True].us_closed >= lb) & (runs[True].us_closed <= ub)).all()
