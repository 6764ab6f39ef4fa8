"""Time-varying reference placements (aslr_set_reference_path) on the GPU against the CPU oracle (tests/_ref_path.py: a
sweep is oracle.knot per (t, b) with the knot's row; a full solve over held via-points is a four-model B = 1 problem per
trajectory), against the same problem written with four action models, and against the device MPC loop composed from the
older entry points one step at a time.

Tolerances are the project's own: tests/_gpu_case.assert_records_match (1e-11 states and costs, 1e-9 the record),
assert_forward_matches (1e-9), tests/_parity.compare (identical iteration counts and decision bits, 1e-6 on xs / us, 1e-4 on
the cost)."""
import ctypes as C

import numpy as np
import pytest

import _ext_call as ext
import _gpu_case as gc
import _mpc_loop
import _ref_path as RP
import test_gpu_traj_params as G
from aslr_to_amd import _abi, crocoddyl, scenarios

pytestmark = pytest.mark.gpu

SOLUTION = ("xs", "us", "traj_f", "traj_i")
AFTER = "after a declined call"


def _same_solution(a, b, what):
    for k in SOLUTION:
        av, bv = (np.ascontiguousarray(v).view(np.int64 if v.dtype == np.float64 else v.dtype) for v in (a[k], b[k]))
        np.testing.assert_array_equal(av, bv, err_msg="%s: %s" % (what, k))


# ---- 1. calc / calcDiff per knot ----
@pytest.mark.parametrize("key, table", [("sea2", False), ("vsa2", False), ("sea7", False), ("sea2", True)])
def test_calc_and_calc_diff_read_the_row_of_each_knot(oracle, key, table):
    """B = 70: two calc blocks, the second partial; T = 5, a path of 6 rows read from row 2, so knots 4 and 5 hold the last
    row.  calcDiff, calc alone, and calcDiff at a second point (the sweep that skips the model-only chunks); one case with a
    per-trajectory parameter table set as well."""
    B, T, n_rows, row0 = 70, 5, 6, 2
    sc = RP.SCENARIOS[key](B=B, T=T, seed=4)
    if table:
        sc = scenarios.with_traj_params(sc, seed=5)
    low = scenarios.lower(RP.with_path(sc, RP.random_path(sc, n_rows, seed=6), row0))
    path_tm = low.ref_path[0]
    assert path_tm.shape == (n_rows, B, 12) and RP.row_of(3, row0, n_rows) == 5 == RP.row_of(5, row0, n_rows)
    e = gc.engine(low)
    assert e.reference_row == row0
    xs, us = gc.random_candidate(low, 1)
    ref = RP.sweep(oracle, low, xs, us, path_tm, row0)
    gc.assert_records_match(*gc.run_calc_diff(e, xs, us), ref=ref)
    gc.assert_records_match(*gc.run_calc(e), None, ref=ref)
    xs2, us2 = gc.random_candidate(low, 5)
    ref2 = RP.sweep(oracle, low, xs2, us2, path_tm, row0)
    assert np.abs(ref2[2] - ref[2]).max() > 1e-3        # the point really changed
    gc.assert_records_match(*gc.run_calc_diff(e, xs2, us2), ref=ref2)
    # the rows are what made the difference: every knot's cost is elsewhere with the create-time references, and -- but for
    # knot 5, where both reads have reached the last row -- with the path read from row 0
    plain = RP.sweep(oracle, low, xs2, us2, np.asarray(sc["frame_refs"], dtype=np.float64)[None], 0, diff=False)[1]
    from_row0 = RP.sweep(oracle, low, xs2, us2, path_tm, 0, diff=False)[1]
    assert (np.abs(plain - ref2[1]).max(axis=1) > 1e-6).all()
    assert (np.abs(from_row0 - ref2[1]).max(axis=1)[:5] > 1e-6).all()


# ---- 2. trial costs ----
def _forward_case(oracle, key, solver, T, B=6, n_rows=6, row0=1):
    sc = RP.SCENARIOS[key](B=B, T=T, seed=4)
    low = scenarios.lower(RP.with_path(sc, RP.random_path(sc, n_rows, seed=7), row0))
    sp = scenarios.solver_params(sc, solver=solver)
    return low, sp, gc.forward_inputs(oracle, low, sp, 5, False)


@pytest.mark.parametrize("key, solver", [("vsa2", "SolverBoxDDP"), ("sea7", "SolverDDP")])
def test_trial_costs_read_the_row_of_each_knot(oracle, monkeypatch, key, solver):
    """B = 6 (a partial group of the interleaved candidate slabs), T = 6, rows 1 .. 5 of 6 (knots 4 .. 6 hold the last one).
    Candidates against the oracle's forward pass; the cost of every step length against the sum, in knot order, of the
    oracle's knot costs on ITS candidates with that knot's row."""
    monkeypatch.delenv("ASLR_PIPELINE", raising=False)
    low, sp, (xs, us, K, k, _) = _forward_case(oracle, key, solver, T=6)
    path_tm, row0 = low.ref_path
    XT, UT, costs = gc.forward_outputs(gc.run_forward(low, sp, xs, us, K, k, None, 1))
    for a in range(_abi.NALPHA):
        xs_try, us_try, cost_plain, fail = oracle.forward_pass(low, sp, 0.5 ** a, xs, us, K, k)
        assert not np.asarray(fail).any()
        gc._assert_close("xs_try[%d]" % a, XT[a], xs_try, 1e-9)
        gc._assert_close("us_try[%d]" % a, UT[a], us_try, 1e-9)
        want = RP.trial_cost(oracle, low, xs_try, us_try, path_tm, row0)
        gc._assert_close("cost_try[%d]" % a, costs[a], want, 1e-9)
        assert (np.abs(want - cost_plain) > 1e-6 * (1.0 + np.abs(want))).all()   # (the create-time references cost otherwise)


@pytest.mark.parametrize("T", [6, 17])
def test_pipelined_forward_pass_gives_the_same_bits(oracle, monkeypatch, T):
    """nj = 2: the two-launch pipeline (trial costs of the first half inside the launch that rolls out the second,
    rollout_and_cost_kernel) and ASLR_PIPELINE=0.  T = 6 is the shape of the test above; a horizon below 16 is rolled out in
    one launch either way, so T = 17 is added: there the trial costs do run inside rollout_and_cost_kernel."""
    import torch
    out = {}
    for pl in (None, "0"):
        if pl is None:
            monkeypatch.delenv("ASLR_PIPELINE", raising=False)
        else:
            monkeypatch.setenv("ASLR_PIPELINE", pl)
        low, sp, (xs, us, K, k, _) = _forward_case(oracle, "vsa2", "SolverBoxDDP", T=T, n_rows=T, row0=1)
        e = gc.run_forward(low, sp, xs, us, K, k, None, 1)
        out[pl] = [e.region(r).clone() for r in (_abi.R_XS_TRY, _abi.R_US_TRY, _abi.R_COST_TRY, _abi.R_TRAJ_F, _abi.R_TRAJ_I)]
        path_tm, row0 = low.ref_path
    for a, b in zip(out[None], out["0"]):
        gc.same_bits(a, b, "ASLR_PIPELINE unset and 0")
    assert bool(torch.isfinite(out[None][2]).all())
    # ... and what both hold is the path's cost (step length 1)
    xs_try, us_try, _, _ = oracle.forward_pass(low, sp, 1.0, xs, us, K, k)
    gc._assert_close("cost_try[0]", gc.to_np(out[None][3])[_abi.TF_COST_TRY0], RP.trial_cost(oracle, low, xs_try, us_try, path_tm, row0), 1e-9)


# ---- 3. nothing changes where nothing should ----
@pytest.mark.parametrize("key", ["sea2", "vsa2", "sea7"])
def test_a_one_row_path_of_the_create_time_references_changes_no_bit(key):
    sc = RP.SCENARIOS[key](B=16, T=30, seed=4)
    sp = scenarios.solver_params(sc, maxiter=25)
    _, plain = gc.solve_gpu(scenarios.lower(sc), sp)
    one_row = np.asarray(sc["frame_refs"], dtype=np.float64)[:, None, :]
    e, got = gc.solve_gpu(scenarios.lower(RP.with_path(sc, one_row)), sp)
    assert e._ref_path is not None and tuple(e._ref_path.shape) == (1, 16, 12)
    assert int(plain["traj_i"][_abi.TI_ITER].min()) >= 1
    _same_solution(got, plain, "one-row path against no path")


def test_clearing_a_path_gives_a_fresh_handle():
    sc = RP.SCENARIOS["sea2"](B=8, T=30, seed=4)
    sp = scenarios.solver_params(sc, maxiter=20)
    low = scenarios.lower(sc)
    _, fresh = gc.solve_gpu(low, sp)
    e, first = gc.solve_gpu(scenarios.lower(RP.with_path(sc, RP.random_path(sc, 31, seed=3), 4)), sp)
    assert np.abs(first["xs"] - fresh["xs"]).max() > 1e-6 and e.reference_row == 4
    e.set_reference_path(None)
    assert e.reference_row == 0 and e._ref_path is None
    e.set_candidate(None, None)
    e.solve(sp)
    gc.sync()
    _same_solution(gc.solution(e), fresh, "after clearing the path")


# ---- 4. full solves ----
@pytest.mark.parametrize("name", sorted(RP.FULL_SOLVE_CASES))
def test_full_solve_matches_the_four_model_oracle(oracle, name):
    """Cold-started solves over held via-points (scenario seed 5, scenarios.reference_via_points(seed=11), the scenario's own
    solver, maxiter and th_stop) against the per-trajectory four-model oracle: identical iteration counts and decision
    bits, converged trajectories within 1e-6 (xs, us) and 1e-4 (cost).  The cases were chosen on the oracle alone;
    tests/test_ref_path_host.py asserts the conditions (>= 90 % converge, no iteration count moves and xs move by less
    than 1e-6 when x0 is scaled by 1 + 1e-14)."""
    sc, via, sp = RP.full_solve_case(name)
    low = scenarios.lower(RP.with_path(sc, scenarios.hold_via_points(via, len(sc["running"]))))
    ref = RP.solve(oracle, low, via, sp, log_cap=sp.maxiter)
    conv = int(((ref["traj_i"][_abi.TI_STATUS] & _abi.ST_CONVERGED) != 0).sum())
    assert conv >= 0.9 * low.B
    _, gpu = gc.solve_gpu(low, sp, log_cap=sp.maxiter)
    G._assert_solve_parity(gpu, ref, sp, {})


@pytest.mark.parametrize("name", ["two_dof_sea", "talos_arm_sea"])
def test_a_shared_path_equals_the_problem_written_with_four_models(name):
    """one path for all trajectories: the GPU solve with the path and the GPU solve of the same problem lowered with four
    action models (their `ref`s the four rows, no frame_ref table) agree bit for bit"""
    sc, via, sp = RP.full_solve_case(name)
    T, B = len(sc["running"]), sc["x0"].shape[0]
    shared = np.repeat(via[:1], B, axis=0)
    low = scenarios.lower(sc)
    _, with_path = gc.solve_gpu(scenarios.lower(RP.with_path(sc, scenarios.hold_via_points(shared, T))), sp)
    _, with_models = gc.solve_gpu(RP.four_models(low, via[0]), sp)
    assert int(with_path["traj_i"][_abi.TI_ITER].min()) >= 1
    _same_solution(with_path, with_models, "path against four models")
    _, plain = gc.solve_gpu(low, sp)
    assert np.abs(plain["xs"] - with_path["xs"]).max() > 1e-6


# ---- 5. sub-shards ----
def test_two_subshards_give_the_same_bits():
    sc = RP.SCENARIOS["vsa2"](B=128, T=20, seed=4)
    sp = scenarios.solver_params(sc, maxiter=12)
    low = scenarios.lower(RP.with_path(sc, RP.random_path(sc, 21, seed=3)))
    _, one = gc.solve_gpu(low, sp)
    _, two = gc.solve_gpu(low, sp, subshards=2)
    assert int(one["traj_i"][_abi.TI_ITER].min()) >= 1
    _same_solution(one, two, "two sub-shards against one")


# ---- 6. MPC ----
def test_mpc_slides_along_the_path():
    """aslr_mpc_run with a path against the composition: the host-driven loop of tests/_mpc_loop.py called one control step
    at a time, the path repositioned at row0 + s before step s.  11 rows from row 1, T = 8, 4 steps: the last steps hold the
    last row."""
    import torch
    B, T, n, first, per, row0 = 5, 8, 4, 6, 2, 1
    sc = RP.SCENARIOS["vsa2"](B=B, T=T, seed=4)
    path = RP.random_path(sc, 11, seed=9)
    low = scenarios.lower(RP.with_path(sc, path, row0))
    sp = scenarios.solver_params(sc, maxiter=400)
    dist = np.random.default_rng(7).uniform(-1e-3, 1e-3, (n, B, low.nx))
    dev, host = gc.engine(low), gc.engine(low)
    for h in (dev, host):
        h.set_candidate(None, None)
    r = dev.mpc_run(sp, n, first, per, np.ascontiguousarray(dist.transpose(1, 0, 2)))
    assert r.reference_row == row0 + n == 5 and dev.reference_row == 5
    dist_d = torch.as_tensor(dist, device=host.device)
    steps = []
    for s in range(n):
        host.set_reference_path(path, row0 + s)
        steps.append(_mpc_loop.host_driven_mpc(host, sp, 1, first if s == 0 else per, per, dist_d[s:s + 1]))
    gc.sync()
    assert host.reference_row == row0 + n - 1     # (the composition sets it; only aslr_mpc_run advances it)
    x_closed = torch.cat([w["x_closed"][:1] for w in steps] + [steps[-1]["x_closed"][1:]])
    gc.same_bits(r.xs_closed, x_closed.permute(1, 0, 2), "xs_closed")
    gc.same_bits(r.us_closed, torch.cat([w["u_closed"] for w in steps]).permute(1, 0, 2), "us_closed")
    sf, si = torch.cat([w["stat_f"] for w in steps]), torch.cat([w["stat_i"] for w in steps])
    for i, k in enumerate(("cost", "stop", "x_reg", "step")):
        gc.same_bits(getattr(r, k), sf[:, i].t(), k)
    gc.same_bits(r.iters, si[:, 0].t(), "iters")
    gc.same_bits(r.status, si[:, 1].t(), "status")
    for rid in (_abi.R_XS, _abi.R_US, _abi.R_TRAJ_F, _abi.R_TRAJ_I, _abi.R_X0):
        gc.same_bits(dev.region(rid), host.region(rid), "region %d" % rid)
    # (every trajectory iterates in step 0 and some trajectory in every step; as in tests/test_gpu_mpc.py, a trajectory whose
    #  short solves let the plant run away may raise its regularisation to the maximum before it completes an iteration)
    assert int(r.iters[:, 0].min()) >= 1 and int(r.iters.max(dim=0).values.min()) >= 1
    # not vacuous: the constant reference steers elsewhere
    const = gc.engine(scenarios.lower(sc))
    const.set_candidate(None, None)
    rc = const.mpc_run(sp, n, first, per, np.ascontiguousarray(dist.transpose(1, 0, 2)))
    assert rc.reference_row == 0
    assert float((rc.xs_closed - r.xs_closed).abs().max()) > 1e-6
    # the facade: ShootingProblem(frame_ref_path=) + set_reference_path(row0) + solve_mpc is the same run
    problem = crocoddyl.ShootingProblem(sc["x0"], sc["running"], sc["terminal"], frame_refs=sc["frame_refs"], frame_ref_path=path)
    problem.set_reference_path(path, row0)
    solver = crocoddyl.SolverBoxDDP(problem)
    solver.th_stop = sp.th_stop
    rf = solver.solve_mpc(n, per, maxiter=first, disturbance=np.ascontiguousarray(dist.transpose(1, 0, 2)))
    assert rf.reference_row == 5 == problem.reference_row
    gc.same_bits(rf.xs_closed, r.xs_closed, "xs_closed through the facade")
    # a second run carries on from row 5; repositioning starts over
    problem.set_reference_path(path, row0)
    assert problem.reference_row == row0


# ---- 7. declines ----
def test_declines_leave_the_handle_as_it_was():
    import torch
    B = 4
    sc = RP.SCENARIOS["sea2"](B=B, T=6, seed=4)
    sp = scenarios.solver_params(sc, solver="SolverFDDP", maxiter=20)
    low = scenarios.lower(sc)
    e = gc.engine(low)
    buf = torch.as_tensor(RP.random_path(sc, 3, seed=1).transpose(1, 0, 2), device=e.device).contiguous()
    ptr = C.c_void_p(buf.data_ptr())
    for n_rows, row0, msg in ((0, 0, "n_rows must be >= 1"), (-2, 0, "n_rows must be >= 1"), (3, -1, r"row0 must lie in \[0, n_rows\)"),
                              (3, 3, r"row0 must lie in \[0, n_rows\)")):
        with pytest.raises(_abi.AslrError, match="aslr_set_reference_path: " + msg):
            e._call("aslr_set_reference_path", ptr, n_rows, row0, e._stream())
        assert e.reference_row == 0
    ext.solve_matches_a_fresh_handle(e, low, sp, ext.SOLVE_REGIONS, AFTER)      # no path was set by any of them
    # ... and a path that IS set survives a declined call
    e._call("aslr_set_reference_path", ptr, 3, 1, e._stream())
    with pytest.raises(_abi.AslrError, match="row0 must lie in"):
        e._call("aslr_set_reference_path", ptr, 3, 7, e._stream())
    assert e.reference_row == 1
    low_path = scenarios.lower(RP.with_path(sc, RP.random_path(sc, 3, seed=1), 1))
    ext.solve_matches_a_fresh_handle(e, low_path, sp, ext.SOLVE_REGIONS, AFTER)
    # a pool solve on a handle with a path set
    with pytest.raises(_abi.AslrError, match="aslr_solve_pool: the handle has a reference path set"):
        e.solve_pool(low.x0, low.frame_ref, sp)
    assert e.reference_row == 1
    ext.solve_matches_a_fresh_handle(e, low_path, sp, ext.SOLVE_REGIONS, AFTER)
    e.set_reference_path(None)
    assert e.solve_pool(low.x0, low.frame_ref, sp)["xs"].shape[0] == B   # cleared: the pool runs
    # no frame-placement cost in the problem
    pc = scenarios.double_pendulum(T=6)
    lowp = scenarios.lower(pc)
    ep = gc.engine(lowp)
    one = torch.zeros((1, 1, 12), dtype=torch.float64, device=ep.device)
    with pytest.raises(_abi.AslrError, match="aslr_set_reference_path: no model of the problem has a frame-placement cost"):
        ep._call("aslr_set_reference_path", C.c_void_p(one.data_ptr()), 1, 0, ep._stream())
    ext.solve_matches_a_fresh_handle(ep, lowp, scenarios.solver_params(pc, maxiter=10), ext.SOLVE_REGIONS, AFTER)
