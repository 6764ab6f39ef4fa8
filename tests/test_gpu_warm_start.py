"""Full solves from a real starting guess against the CPU oracle started from the same arrays.  From Crocoddyl's empty
candidate the gaps close with the first accepted full step; from a guess they persist: non-zero gaps at every knot, the
gap-tolerance switch of the calc sweep, the gap terms of the backward sweeps, SolverBoxDDP's plain gains while infeasible
and its QP once feasible, and SolverFDDP steps that are accepted at alpha < 1 and stay infeasible.

The guess: xs = x0 + U(-0.1, 0.1) at every knot, us = U(-0.2, 0.2), stiffness commands of the VSA models U(1, 5) (inside
their boxes), drawn time-major from default_rng(seed); is_feasible = 0.  Tolerances are north_star's, as
test_gpu_parity.test_c5_horizon_full_solves_match_oracle applies them: iteration counts and decision bits exactly, xs /
us within 1e-6 of the size of the trajectory's iterates, the cost within 1e-4 of max(1, |cost|); on top, the accepted
step index, the feasibility flag and the regularisation of every iteration exactly."""
import numpy as np
import pytest

from aslr_to_amd import _abi, scenarios

import _gpu_case as gc
import _parity

pytestmark = pytest.mark.gpu


def _guess(sc, low, seed=3):
    """-> xs [T+1, B, nx], us [T, B, nu] (time-major, the oracle's layout; Engine.set_candidate takes [B, T+1, nx])"""
    rng = np.random.default_rng(seed)
    xs = np.atleast_2d(sc["x0"])[None] + rng.uniform(-0.1, 0.1, (low.T + 1, low.B, low.nx))
    us = rng.uniform(-0.2, 0.2, (low.T, low.B, low.nu))
    if low.dam == _abi.DAM_VSA:
        us[..., low.nu // 2:] = rng.uniform(1.0, 5.0, (low.T, low.B, low.nu // 2))
    return xs, us


def _solve(oracle, low, sp, xs, us, nthreads=8):
    """The oracle and the GPU from the same candidate (None: the empty one), both with their iteration logs
    -> the engine, gc.solution of it, the oracle's result"""
    ref = oracle.solve(low, sp, xs=xs, us=us, nthreads=nthreads, log_cap=sp.maxiter)
    return gc.solve_gpu(low, sp, xs, us, log_cap=sp.maxiter) + (ref,)


def _compare(gpu, ref, label, sel=None):
    """Iteration counts, status words and the logged decisions exactly; iterates and costs within north_star's
    tolerances -- on the trajectories in `sel` (a mask; default: all of them)."""
    it_r, st_r = ref["traj_i"][_abi.TI_ITER], ref["traj_i"][_abi.TI_STATUS]
    sel = np.ones(it_r.shape, dtype=bool) if sel is None else sel
    np.testing.assert_array_equal(gpu["traj_i"][_abi.TI_ITER][sel], it_r[sel])
    _parity.assert_status_words_match(gpu["traj_i"][_abi.TI_STATUS][sel], st_r[sel])
    lg, lr = gpu["log"], ref["log"]
    for row, what in ((_abi.LOG_ACCEPTED, "accepted step index"), (_abi.LOG_FEASIBLE, "feasibility"), (_abi.LOG_XREG, "x_reg")):
        np.testing.assert_array_equal(lg[:, row][:, sel], lr[:, row][:, sel], err_msg="per-iteration %s (rows: iterations)" % what)
    scale = np.maximum(1.0, np.maximum(np.abs(ref["xs"]).max(axis=(0, 2)), np.abs(ref["us"]).max(axis=(0, 2))))
    dx = (np.abs(gpu["xs"] - ref["xs"]).max(axis=(0, 2)) / scale)[sel].max()
    du = (np.abs(gpu["us"] - ref["us"]).max(axis=(0, 2)) / scale)[sel].max()
    cost = ref["traj_f"][_abi.TF_COST]
    dc = (np.abs(gpu["traj_f"][_abi.TF_COST] - cost) / np.maximum(1.0, np.abs(cost)))[sel].max()
    print("%s: iterations %d..%d, max rel |dx| %.2e |du| %.2e |dcost| %.2e"
          % (label, it_r[sel].min(), it_r[sel].max(), dx, du, dc))
    assert dx < 1e-6 and du < 1e-6, (dx, du)
    assert dc < 1e-4, dc


def _persistent_gap_iterations(log):
    """per trajectory: iterations that accepted a step shorter than 1 and left the trajectory infeasible"""
    return ((log[:, _abi.LOG_ACCEPTED] > 0) & (log[:, _abi.LOG_FEASIBLE] == 0)).sum(axis=0)


# (scenario, solver, B, T, seed of the guess, must the oracle's log show persistent gaps).  With the guess of seed 3 the
# oracle alone converges on every trajectory of every row (13 - 56, 13 - 56, 8 - 31, 10 - 32, 20 - 43 iterations).
# 2-DoF SEA at T = 40 accepts the full step in its first iteration whatever the draw (no seed in 0..299 does otherwise on
# the oracle), which closes the gaps at once; at T = 100 trajectories of the same recipe do accept shorter steps first, so
# that row -- the second below, an addition to the five the issue lists -- is what holds the planar kernels to the
# persistent-gap path.
ROWS = [("two_dof_sea", "SolverFDDP", 16, 40, 3, False),
        ("two_dof_sea", "SolverFDDP", 16, 100, 0, True),
        ("two_dof_sea", "SolverDDP", 16, 40, 3, False),
        ("talos_arm_sea", "SolverFDDP", 4, 30, 3, True),
        ("talos_arm_sea", "SolverDDP", 4, 30, 3, False),
        ("talos_arm_vsa", "SolverBoxDDP", 4, 20, 3, False)]


@pytest.mark.parametrize("name,solver,B,T,seed,persistent", ROWS, ids=["%s-%s-T%d" % (r[0], r[1], r[3]) for r in ROWS])
def test_warm_started_solve_matches_oracle(oracle, name, solver, B, T, seed, persistent):
    sc = scenarios.SCENARIOS[name](B=B, T=T)
    low = scenarios.lower(sc)
    sp = scenarios.solver_params(sc, solver=solver, maxiter=100)
    assert sp.is_feasible == 0
    xs, us = _guess(sc, low, seed)
    _, gpu, ref = _solve(oracle, low, sp, xs, us)
    assert ((ref["traj_i"][_abi.TI_STATUS] & _abi.ST_CONVERGED) != 0).all()
    if persistent:   # (a condition on the guess: change the seed, not this line)
        n = _persistent_gap_iterations(ref["log"])
        print("iterations that keep their gaps, per trajectory: %s" % n)
        assert n.max() >= 1
    _compare(gpu, ref, "%s %s B=%d T=%d from a guess" % (name, solver, B, T))


def test_boxddp_first_iterations_from_a_guess_take_the_oracles_decisions(oracle):
    """2-DoF VSA from the guess is not well behaved on the oracle itself (every trajectory notes a forward error in its
    first iterations, 5 of 16 converge within 100 iterations, and under SolverFDDP the iterates reach 1e27), so no
    converged values are compared on it: six iterations under SolverBoxDDP, on iteration counts, status words and the
    regularisation.  Some trajectories reject every step length and stay infeasible (plain gains throughout), the
    others turn feasible after the first iteration and go on with the QP; x_reg ends between 1e-9 and 1e-3."""
    sc = scenarios.two_dof_vsa_boxddp(B=16, T=40)
    low = scenarios.lower(sc)
    sp = scenarios.solver_params(sc, solver="SolverBoxDDP", maxiter=6)
    xs, us = _guess(sc, low)
    _, gpu, ref = _solve(oracle, low, sp, xs, us)
    np.testing.assert_array_equal(gpu["traj_i"][_abi.TI_ITER], ref["traj_i"][_abi.TI_ITER])
    _parity.assert_status_words_match(gpu["traj_i"][_abi.TI_STATUS], ref["traj_i"][_abi.TI_STATUS])
    np.testing.assert_array_equal(gpu["traj_f"][_abi.TF_XREG], ref["traj_f"][_abi.TF_XREG])
    print("2-DoF VSA BoxDDP, 6 iterations from a guess: status %s, x_reg %s"
          % (sorted(set(ref["traj_i"][_abi.TI_STATUS].tolist())), sorted(set(ref["traj_f"][_abi.TF_XREG].tolist()))))


def test_boxddp_from_a_perturbed_iterate_switches_to_the_qp_like_the_oracle(oracle):
    """SolverBoxDDP computes plain gains while the candidate is infeasible and solves the box QP once it is feasible: a
    full solve from the oracle's cold iterate after 5 iterations with U(-1e-3, 1e-3) added to xs (default_rng(1)) and
    is_feasible = 0.  The oracle alone converges on all 16 trajectories from it, in 33 - 378 iterations, with no
    backward error.

    One of them cannot be compared to the end, for a reason that shows on the oracle alone: a relative perturbation of
    1e-14 of the guess changes the oracle's own iteration count of trajectory 7 (133 -> 187, 138, 245 with the three draws
    below; its accepted step index first differs at iterations 19 - 22), while the other 15 keep theirs to the end.  On
    the MI355X that trajectory took 364 iterations against the oracle's 133 and the other 15 matched exactly.  So the
    trajectories whose count the oracle itself keeps under these perturbations are compared in full, and the others
    on the decisions of their first 12 iterations (a difference of 1e-14 needs ~20 iterations to flip a decision, i.e.
    grows ~5x per iteration; kernel outputs differ from the oracle's by 1e-13 .. 1e-12, two or three iterations' worth)."""
    sc = scenarios.two_dof_vsa_boxddp(B=16, T=40)
    low = scenarios.lower(sc)
    cold = oracle.solve(low, scenarios.solver_params(sc, solver="SolverBoxDDP", maxiter=5))
    xs = cold["xs"] + np.random.default_rng(1).uniform(-1e-3, 1e-3, cold["xs"].shape)
    sp = scenarios.solver_params(sc, solver="SolverBoxDDP")
    _, gpu, ref = _solve(oracle, low, sp, xs, cold["us"])
    st, it = ref["traj_i"][_abi.TI_STATUS], ref["traj_i"][_abi.TI_ITER]
    conv = (st & _abi.ST_CONVERGED) != 0
    assert conv.sum() >= 12 and (st & _abi.ST_BACKWARD_ERR == 0).all()
    feas = ref["log"][:, _abi.LOG_FEASIBLE]
    assert (feas[0] == 1).all()        # infeasible into the first iteration (is_feasible = 0), feasible out of it
    m = sc["running"][0]
    assert ((ref["us"] == m.u_lb) | (ref["us"] == m.u_ub)).any()      # the QP's box is active in the solution
    stable = np.ones(low.B, dtype=bool)
    for k in range(3):
        wiggle = 1.0 + np.random.default_rng(100 + k).uniform(-1e-14, 1e-14, xs.shape)
        stable &= oracle.solve(low, sp, xs=xs * wiggle, us=cold["us"], nthreads=8)["traj_i"][_abi.TI_ITER] == it
    print("trajectories whose iteration count the oracle keeps under 1e-14 perturbations: %d of %d" % (stable.sum(), low.B))
    # Pinned, so that a change that widens this set is looked at.  The set is a property of the ORACLE build alone (its
    # rounding under the three perturbations above); the GPU code has no part in it.  If this line fails after the oracle
    # was built with another compiler or OpenMP runtime, derive the set again on the oracle; it is no kernel defect.
    assert list(np.nonzero(~stable)[0]) == [7]
    _compare(gpu, ref, "2-DoF VSA BoxDDP from a perturbed iterate", sel=stable & conv)
    lg = gpu["log"]
    for row in (_abi.LOG_ACCEPTED, _abi.LOG_FEASIBLE, _abi.LOG_XREG):
        np.testing.assert_array_equal(lg[:12, row][:, ~stable], ref["log"][:12, row][:, ~stable])


@pytest.mark.parametrize("solver", ["SolverDDP", "SolverFDDP"])
def test_feasible_warm_start_matches_oracle(oracle, solver):
    """The GPU's own iterate after three cold iterations, declared feasible (is_feasible = 1: no gap terms anywhere),
    solved again on the GPU and by the oracle from the same arrays."""
    sc = scenarios.two_dof_sea(B=16, T=40)
    low = scenarios.lower(sc)
    _, third = gc.solve_gpu(low, scenarios.solver_params(sc, solver="SolverDDP", maxiter=3), poll_every=0)
    xs, us = third["xs"], third["us"]
    sp = scenarios.solver_params(sc, solver=solver, is_feasible=1)
    _, gpu, ref = _solve(oracle, low, sp, xs, us)
    assert ((ref["traj_i"][_abi.TI_STATUS] & _abi.ST_CONVERGED) != 0).all()
    assert (ref["log"][0, _abi.LOG_FEASIBLE] == 1).all()
    np.testing.assert_array_equal(gpu["traj_i"][_abi.TI_STATUS], ref["traj_i"][_abi.TI_STATUS])
    _compare(gpu, ref, "2-DoF SEA %s from the GPU's third iterate, feasible" % solver)


def test_cold_and_warm_trajectories_in_one_batch(oracle):
    """B = 70 under SolverFDDP: even trajectories start from the empty candidate, odd ones from the guess, so every wave
    holds both.  Against the oracle, and bit for bit against the same trajectories in an all-cold and an all-warm batch
    (no arithmetic crosses trajectories)."""
    import torch
    sc = scenarios.two_dof_sea(B=70, T=40)
    low = scenarios.lower(sc)
    sp = scenarios.solver_params(sc, solver="SolverFDDP", maxiter=100)
    xs, us = _guess(sc, low)
    odd = np.arange(low.B) % 2 == 1
    xs_mix, us_mix = np.where(odd[None, :, None], xs, 0.0), np.where(odd[None, :, None], us, 0.0)
    e, gpu, ref = _solve(oracle, low, sp, xs_mix, us_mix)
    _compare(gpu, ref, "2-DoF SEA FDDP, cold and warm trajectories mixed")
    regions = (_abi.R_XS, _abi.R_US, _abi.R_TRAJ_F, _abi.R_TRAJ_I)
    mixed = [e.region(r).clone() for r in regions]
    for which, cand in ((~odd, (None, None)), (odd, (xs, us))):
        h, _ = gc.solve_gpu(low, sp, *cand)
        sel = torch.as_tensor(which, device=h.device)
        for r, m in zip(regions, mixed):
            gc.same_bits(h.region(r)[:, sel], m[:, sel], "region %d of the %s trajectories" % (r, "warm" if which is odd else "cold"))
