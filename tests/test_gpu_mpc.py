"""Receding-horizon runs on the device (aslr_mpc_run / Engine.mpc_run / Solver*.solve_mpc): against the oracle loop of
tests/test_mpc_host.py, the advance kernel exactly, against the same loop driven from Python through the older entry
points bit for bit, independence of the schedule, and the declines."""
import copy

import numpy as np
import pytest

from aslr_to_amd import _abi, crocoddyl, scenarios

import _ext_call as ext
import _gpu_case as gc
import _mpc_loop
import _parity
import test_mpc_host as H

pytestmark = pytest.mark.gpu

AFTER = "after a declined aslr_mpc_run"


def _result_arrays(r):
    return dict(xs_closed=r.xs_closed, us_closed=r.us_closed, iters=r.iters, status=r.status, cost=r.cost, stop=r.stop,
                x_reg=r.x_reg, step=r.step)


def _dist_bm(dist):
    """time-major numpy [n, B, nx] -> what Engine.mpc_run takes, [B, n, nx]"""
    return None if dist is None else np.ascontiguousarray(dist.transpose(1, 0, 2))


# ---- 1. the oracle loop ----
@pytest.mark.parametrize("row", H.ROWS, ids=H.ROW_IDS)
def test_closed_loop_matches_the_oracle_loop(oracle, row):
    """Per step: iteration counts and decision bits exactly; closed-loop states and controls within 1e-6 of the
    trajectory's scale, costs within 1e-4 of max(1, |cost|) (the bounds of test_gpu_warm_start.py)."""
    ref = H.parity_reference(oracle, row)
    sc, sp, dist = H.parity_case(*row)
    solver = getattr(crocoddyl, row[1])(crocoddyl.ShootingProblem(sc["x0"], sc["running"], sc["terminal"], frame_refs=sc["frame_refs"]))
    solver.th_stop = sp.th_stop
    r = solver.solve_mpc(H.N_STEPS, H.ITERS_PER_STEP, maxiter=H.FIRST_MAXITER, disturbance=_dist_bm(dist))
    e = solver.problem.engine
    xc, uc = gc.to_np(r.xs_closed).transpose(1, 0, 2), gc.to_np(e.pad_u(r.us_closed)).transpose(1, 0, 2)
    for s in range(H.N_STEPS):
        np.testing.assert_array_equal(gc.to_np(r.iters)[:, s], ref["iters"][s], err_msg="iterations of step %d" % s)
        _parity.assert_status_words_match(gc.to_np(r.status)[:, s], ref["status"][s])
    scale = np.maximum(1.0, np.maximum(np.abs(ref["x_closed"]).max(axis=(0, 2)), np.abs(ref["u_closed"]).max(axis=(0, 2))))
    dx = (np.abs(xc - ref["x_closed"]).max(axis=(0, 2)) / scale).max()
    du = (np.abs(uc - ref["u_closed"]).max(axis=(0, 2)) / scale).max()
    dc = (np.abs(gc.to_np(r.cost).T - ref["cost"]) / np.maximum(1.0, np.abs(ref["cost"]))).max()
    # the plan the run leaves behind is the oracle loop's last shifted plan
    dp = (np.abs(gc.to_np(e.region(_abi.R_XS)) - ref["xs"]).max(axis=(0, 2)) / scale).max()
    print("%s %s: iterations of step 0 %d..%d, max rel |dx| %.2e |du| %.2e |dcost| %.2e, final plan %.2e"
          % (row[0], row[1], ref["iters"][0].min(), ref["iters"][0].max(), dx, du, dc, dp))
    assert dx < 1e-6 and du < 1e-6 and dp < 1e-6, (dx, du, dp)
    assert dc < 1e-4, dc
    np.testing.assert_array_equal(gc.to_np(solver.xs), gc.to_np(e.xs))   # solver.xs / us: the last shifted plan
    assert tuple(r.xs_closed.shape) == (row[2], H.N_STEPS + 1, e.nx) and tuple(r.us_closed.shape) == (row[2], H.N_STEPS, e.nu_user)


# ---- 2. the advance kernel, exactly ----
@pytest.mark.parametrize("name,B,T", [("two_dof_sea", 5, 1), ("two_dof_sea", 5, 3), ("two_dof_sea", 65, 1),
                                      ("two_dof_sea", 65, 3), ("talos_arm_sea", 3, 2)])
def test_advance_step_is_exact(oracle, name, B, T):
    """One step (three iterations of SolverFDDP from the empty candidate) against a twin handle that runs a plain solve and
    aslr_calc: record, plant, shift and reset bit for bit.  B = 5 and 65 cross a group of four trajectories and a block of 64,
    T = 1 and 3 leave the shift nothing (no control row moves) or almost nothing to move.

    The plant state is compared as x_closed[1] == XNEXT[0] + disturbance, the sum the kernel forms: subtracting the
    disturbance again from a rounded sum does not give XNEXT[0] back bit for bit.  Against the oracle's knot the difference
    x_closed[1] - disturbance is held to 1e-11 of max(1, |x|)."""
    sc = scenarios.SCENARIOS[name](B=B, T=T, seed=1)
    low = scenarios.lower(sc)
    sp = scenarios.solver_params(sc, solver="SolverFDDP", maxiter=3)
    dist = np.random.default_rng(7).uniform(-1e-3, 1e-3, (1, B, low.nx))
    e, twin = gc.engine(low), gc.engine(low)
    for h in (e, twin):
        h.set_candidate(None, None)
    r = e.mpc_run(sp, 1, 3, 3, _dist_bm(dist))
    twin.solve(sp, poll_every=0)
    twin.calc()
    gc.sync()
    X, U, XN = (gc.to_np(twin.region(rid)) for rid in (_abi.R_XS, _abi.R_US, _abi.R_XNEXT))
    xp = XN[0] + dist[0]
    xs_want, us_want = np.concatenate([X[1:], X[-1:]]), np.concatenate([U[1:], U[-1:]])
    xs_want[0] = xp
    same = lambda a, b, what: np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64), err_msg=what)
    same(gc.to_np(e.region(_abi.R_XS)), xs_want, "XS after the shift")
    same(gc.to_np(e.region(_abi.R_US)), us_want, "US after the shift")
    xc = gc.to_np(r.xs_closed)
    same(xc[:, 0], X[0], "x_closed[0]")
    same(gc.to_np(r.us_closed), U[0][:, None], "u_closed[0]")
    same(xc[:, 1], xp, "x_closed[1] = XNEXT[0] + disturbance")
    same(gc.to_np(e.region(_abi.R_X0)), xp, "X0")
    same(gc.to_np(e.region(_abi.R_X0)), gc.to_np(e.region(_abi.R_XS))[0], "X0 = xs[0]")
    knot = np.stack([oracle.knot(low, int(low.node_model[0]), X[0, b], U[0, b], low.frame_ref[b], diff=False)["xnext"] for b in range(B)])
    dk = (np.abs(xc[:, 1] - dist[0] - knot) / np.maximum(1.0, np.abs(knot))).max()
    print("%s B=%d T=%d: plant state against the oracle's knot %.2e" % (name, B, T, dk))
    assert dk < 1e-11
    for rid in (_abi.R_KFF, _abi.R_GAPS, _abi.R_VXXF):
        assert not gc.to_np(e.region(rid)).view(np.int64).any(), "region %d is not all zero" % rid
    np.testing.assert_array_equal(gc.to_np(r.iters)[:, 0], gc.to_np(twin.traj_i(_abi.TI_ITER)))
    same(gc.to_np(r.cost)[:, 0], gc.to_np(twin.traj_f(_abi.TF_COST)), "cost of the step")


# ---- 3. the device loop is the host-driven loop ----
def _table_case(B=64, T=20):
    sc = scenarios.with_traj_params(scenarios.two_dof_vsa_boxddp(B=B, T=T), seed=4, stiffness_floors=(0.0, 0.002))
    rng = np.random.default_rng(5)
    tp = sc["traj_params"]   # random motor inertia already; random boxes: torques +-U(50, 100), stiffness up to U(50, 100)
    tp["u_ub"] = rng.uniform(50.0, 100.0, tp["u_ub"].shape)
    tp["u_lb"][:, :2] = -rng.uniform(50.0, 100.0, (B, 2))
    return sc


def test_device_loop_equals_the_host_driven_loop_bit_for_bit():
    import torch
    sc = _table_case()
    low = scenarios.lower(sc)
    sp = scenarios.solver_params(sc, maxiter=400)
    n, first, per = 4, 6, 2
    dist = np.random.default_rng(7).uniform(-1e-3, 1e-3, (n, low.B, low.nx))
    dev, host = gc.engine(low), gc.engine(low)
    for h in (dev, host):
        h.set_candidate(None, None)
    r = dev.mpc_run(sp, n, first, per, _dist_bm(dist))
    w = _mpc_loop.host_driven_mpc(host, sp, n, first, per, torch.as_tensor(dist, device=host.device))
    gc.sync()
    assert sp.maxiter == 400
    gc.same_bits(r.xs_closed, w["x_closed"].permute(1, 0, 2), "xs_closed")
    gc.same_bits(r.us_closed, w["u_closed"].permute(1, 0, 2), "us_closed")
    for i, k in enumerate(("cost", "stop", "x_reg", "step")):
        gc.same_bits(getattr(r, k), w["stat_f"][:, i].t(), k)
    gc.same_bits(r.iters, w["stat_i"][:, 0].t(), "iters")
    gc.same_bits(r.status, w["stat_i"][:, 1].t(), "status")
    for rid in ext.MPC_REGIONS:
        gc.same_bits(dev.region(rid), host.region(rid), "region %d" % rid)
    # (the comparison is not empty: every trajectory iterates in step 0, some trajectory in every step, the states move.
    #  Not every trajectory iterates in every step: with so few iterations this plant runs away on some of them -- costs of
    #  1e10 .. 1e37 by step 2 -- and their next solve raises its regularisation to the maximum before it completes an
    #  iteration: 0 iterations, status REG_MAX | BACKWARD_ERR.  The oracle loop does the same on the scenario without the
    #  table, on 20 of 64 trajectories; those steps are held to the host-driven loop bit for bit like every other.)
    assert int(r.iters[:, 0].min()) >= 1 and int(r.iters.max(dim=0).values.min()) >= 1
    assert float((r.xs_closed[:, 1:] - r.xs_closed[:, :-1]).abs().max()) > 0.0
    # the table is what the plant used: with the models' constants the closed loop differs
    plain = gc.engine(scenarios.lower(scenarios.two_dof_vsa_boxddp(B=low.B, T=low.T)))
    plain.set_candidate(None, None)
    rp = plain.mpc_run(sp, n, first, per, _dist_bm(dist))
    assert float((rp.xs_closed - r.xs_closed).abs().max()) > 1e-6


# ---- 4. schedule independence ----
def test_results_do_not_depend_on_subshards_or_batch():
    sc = scenarios.two_dof_vsa_boxddp(B=128, T=20)
    sp = scenarios.solver_params(sc, maxiter=400)
    n, first, per = 3, 6, 2
    dist = np.random.default_rng(7).uniform(-1e-3, 1e-3, (n, 128, 8))

    def run(sc, dist, nsub):
        e = gc.engine(scenarios.lower(sc))
        e.set_subshards(nsub)
        e.set_candidate(None, None)
        r = e.mpc_run(sp, n, first, per, _dist_bm(dist))
        return e, r

    e1, r1 = run(sc, dist, 1)
    e2, r2 = run(sc, dist, 2)
    for k, a in _result_arrays(r1).items():
        gc.same_bits(a, _result_arrays(r2)[k], "%s with two sub-shards" % k)
    for rid in ext.SOLVE_REGIONS:
        gc.same_bits(e1.region(rid), e2.region(rid), "region %d with two sub-shards" % rid)
    half = dict(sc)
    half["x0"], half["frame_refs"] = sc["x0"][:64], sc["frame_refs"][:64]
    e3, r3 = run(half, dist[:, :64], 1)
    for k, a in _result_arrays(r1).items():
        gc.same_bits(a[:64], _result_arrays(r3)[k], "%s of the first 64 trajectories in a batch of 64" % k)
    for rid in ext.SOLVE_REGIONS:
        gc.same_bits(e1.region(rid)[:, :64], e3.region(rid), "region %d of the first 64 trajectories" % rid)


# ---- 5. declines ----
def test_declines_leave_the_handle_usable():
    sc = scenarios.two_dof_sea(B=4, T=6)
    sp = scenarios.solver_params(sc, solver="SolverFDDP", maxiter=20)
    # two distinct running models (the terminal model may differ, and does in every scenario)
    mixed = dict(sc)
    mixed["running"] = [sc["running"][0]] * 3 + [copy.copy(sc["running"][0])] * 3
    low = scenarios.lower(mixed)
    assert low.desc.nmodels == 3
    e = gc.engine(low)
    e.set_candidate(None, None)
    with pytest.raises(_abi.AslrError, match="more than one action model"):
        e.mpc_run(sp, 2, 5, 2)
    ext.solve_matches_a_fresh_handle(e, low, sp, ext.SOLVE_REGIONS, AFTER)
    # an iteration log that is set
    low = scenarios.lower(sc)
    e = gc.engine(low)
    e.set_candidate(None, None)
    e.enable_iteration_log(20)
    with pytest.raises(_abi.AslrError, match="an iteration log is set"):
        e.mpc_run(sp, 2, 5, 2)
    ext.solve_matches_a_fresh_handle(e, low, sp, ext.SOLVE_REGIONS, AFTER)
    e.enable_iteration_log(0)
    # n_steps = 0 (and the other counts)
    for args in ((0, 5, 2), (2, 0, 2), (2, 5, 0)):
        with pytest.raises(_abi.AslrError, match="n_steps, first_maxiter and iters_per_step must be >= 1"):
            e.mpc_run(sp, *args)
    ext.solve_matches_a_fresh_handle(e, low, sp, ext.SOLVE_REGIONS, AFTER)
    e.mpc_run(sp, 2, 5, 2)   # (and the same handle runs once the arguments are right)
    # (7, VSA) with SolverDDP
    sc7 = scenarios.talos_arm_vsa(B=2, T=4)
    low7 = scenarios.lower(sc7)
    e7 = gc.engine(low7)
    e7.set_candidate(None, None)
    with pytest.raises(_abi.AslrError, match="built for SolverBoxDDP only"):
        e7.mpc_run(scenarios.solver_params(sc7, solver="SolverDDP", maxiter=5), 2, 5, 2)
    ext.solve_matches_a_fresh_handle(e7, low7, scenarios.solver_params(sc7, maxiter=10), ext.SOLVE_REGIONS, AFTER)
