"""GPU parity on geometry the synthetic scenarios do not have: the general 3-D recursion at nj = 2 (axes other than +z,
rotated joint / inertial / frame origins, gravity with a z component) for SEA and VSA, and frame-placement costs whose
references are rotated, with residual rotations in every branch of the SE(3) log.  The oracle is the checker (it is pinned
to a 40-digit reference on the same chains and log bands by tests/test_oracle_geometry.py); tolerances are those of
tests/test_gpu_parity.py: 1e-11 on xnext and cost, 1e-9 on the DERIV record and on forward-pass outputs."""
import numpy as np
import pytest

from aslr_to_amd import _abi, scenarios

import _geometry_chains as chains
import _gpu_case as gc
import _parity

pytestmark = pytest.mark.gpu

TAYLOR = 2.0 ** -13


def _check_forward(oracle, low, solver, seed=5):
    """Rollout + trial costs of every step length against the oracle (FDDP: infeasible start, the gaps are closed by
    the rollout)."""
    sp = _abi.default_solver_params(gc.SOLVERS[solver])
    fddp = solver == "SolverFDDP"
    xs, us, K, k, gaps = gc.forward_inputs(oracle, low, sp, seed, fddp)
    feasible = 0 if fddp else 1
    e = gc.run_forward(low, sp, xs, us, K, k, gaps, feasible)
    oks, _ = gc.assert_forward_matches(*gc.forward_outputs(e), lambda alpha: oracle.forward_pass(
        low, sp, alpha, xs, us, K, k, gaps if fddp else None, feasible if fddp else None))
    assert all(ok.mean() > 0.5 for ok in oks)
    return e


# ---------------------------------------------------------------------------------------------
# the general recursion at nj = 2
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [70, 130])
@pytest.mark.parametrize("actuator", ["sea", "vsa"])
@pytest.mark.parametrize("chain", chains.CHAINS)
def test_calc_and_calcdiff_on_non_planar_two_joint_chains(oracle, chain, actuator, B):
    """calc_kernel<2, SEA / VSA, *, false, ...> (the planar detector declines all three chains) at batches that leave a
    partial wave, T = 5, both sweeps."""
    low = scenarios.lower(chains.problem(chain, actuator, B=B, T=5, seed=B))
    gc.check_calc_and_calc_diff(oracle, low)


@pytest.mark.parametrize("actuator", ["sea", "vsa"])
def test_model_level_entry_points_on_the_general_chain(oracle, actuator):
    """dam_eval, dam_residuals, frame_placement (every frame, the welded end effector with its rotated origin included)
    and quasi_static through the general path, running and terminal models, against the oracle point by point."""
    import torch
    sc = chains.problem("general", actuator, B=70, T=3, seed=2)
    sc["frame_refs"][0, :9] = chains.random_rotation(np.random.default_rng(3)).reshape(9)
    low = scenarios.lower(sc)
    fref = low.frame_ref[0]       # (the point evaluators take trajectory 0's reference for every point)
    e = gc.engine(low)
    n = 70
    xs, us = gc.random_candidate(low, 9)
    x, u = xs[0], us[0]
    for mi in range(low.desc.nmodels):
        got = e.dam_eval(mi, x, u)
        res = e.dam_residuals(mi, x, u)
        for b in range(n):
            ref = oracle.dam(low, mi, x[b], u[b], frame_ref=fref)
            for key in ("xout", "cost"):
                assert gc.relerr(got[key][b], ref[key]) < 1e-11, (mi, b, key)
            for key in ("Fx", "Fu", "Lx", "Lu", "Lxx", "Lxu", "Luu"):
                assert gc.relerr(got[key][b], ref[key]) < 1e-9, (mi, b, key)
            assert gc.relerr(res[b], oracle.dam_residuals(low, mi, x[b], u[b], frame_ref=fref)) < 1e-11, (mi, b)
    model = sc["terminal"].state.pinocchio
    xd = torch.as_tensor(x, device=e.device)
    for fr in model.frames[1:]:
        R, p = e.frame_placement(fr.parent, fr.placement.rotation, fr.placement.translation, xd)
        R, p = gc.to_np(R), gc.to_np(p)
        for b in range(n):
            Rr, pr = oracle.frame_placement(low.desc.chain, x[b, :2], fr.parent, fr.placement.rotation,
                                            fr.placement.translation)
            np.testing.assert_allclose(R[b], Rr, rtol=0, atol=1e-13)
            np.testing.assert_allclose(p[b], pr, rtol=0, atol=1e-13)
    # quasi-static controls of the states in XS (Gauss-Newton on the Euler step), knot by knot
    xs[..., 4:] *= 0.25
    e.region(_abi.R_XS).copy_(torch.as_tensor(xs))
    iters = gc.to_np(e.quasi_static())
    gc.sync()
    U = gc.to_np(e.region(_abi.R_US))
    assert (iters >= 0).all()
    for t in range(low.T):
        for b in range(0, n, 7):
            u_ref, it = oracle.quasi_static(low, int(low.node_model[t]), xs[t, b], frame_ref=low.frame_ref[b])
            assert it >= 0
            np.testing.assert_allclose(U[t, b], u_ref, rtol=1e-8, atol=1e-10)


@pytest.mark.parametrize("solver", ["SolverDDP", "SolverFDDP"])
@pytest.mark.parametrize("actuator", ["sea", "vsa"])
def test_forward_pass_on_the_general_chain_for_every_alpha(oracle, actuator, solver):
    """rollout_kernel<2, *, false, *> and trial_cost_kernel<2, *, false, false>: the non-planar forward pass."""
    low = scenarios.lower(chains.problem("general", actuator, B=70, T=20, seed=4))
    _check_forward(oracle, low, solver)


@pytest.mark.parametrize("actuator,solver", [("sea", "SolverDDP"), ("sea", "SolverFDDP"), ("vsa", "SolverBoxDDP")])
def test_short_solves_on_the_general_chain(oracle, actuator, solver):
    """Full solves, B = 16, T = 40, through every kernel of the general path: the oracle's iteration counts exactly,
    decision bits of the status words exactly, xs / us within 1e-6 of the size of the iterates."""
    sc = chains.problem("general", actuator, B=16, T=40, seed=3)
    low = scenarios.lower(sc)
    sp = scenarios.solver_params(sc, solver=solver)
    ref = oracle.solve(low, sp, nthreads=8)
    _, g = gc.solve_gpu(low, sp, poll_every=4)
    st_r = ref["traj_i"][_abi.TI_STATUS]
    assert ((st_r & _abi.ST_CONVERGED) != 0).all()
    np.testing.assert_array_equal(g["traj_i"][_abi.TI_ITER], ref["traj_i"][_abi.TI_ITER])
    _parity.assert_status_words_match(g["traj_i"][_abi.TI_STATUS], st_r)
    scale = np.maximum(1.0, np.maximum(np.abs(ref["xs"]).max(axis=(0, 2)), np.abs(ref["us"]).max(axis=(0, 2))))
    dx = np.abs(g["xs"] - ref["xs"]).max(axis=(0, 2)) / scale
    du = np.abs(g["us"] - ref["us"]).max(axis=(0, 2)) / scale
    dc = np.abs(g["traj_f"][_abi.TF_COST] - ref["traj_f"][_abi.TF_COST])
    print("general %s %s: iterations %s, max rel |dx| %.2e |du| %.2e, |dcost| %.2e"
          % (actuator, solver, ref["traj_i"][_abi.TI_ITER], dx.max(), du.max(), dc.max()))
    assert dx.max() < 1e-6 and du.max() < 1e-6
    assert (dc < 1e-4 * np.maximum(1.0, np.abs(ref["traj_f"][_abi.TF_COST]))).all()


# ---------------------------------------------------------------------------------------------
# rotated references
# ---------------------------------------------------------------------------------------------
# residual rotations rMf = Mref^-1 oMf of the evaluated state, one per SE(3) log branch: the Taylor band (far inside it
# and just under its edge 2^-13, where Pinocchio's alpha = 1 - t^2/12 differs from 1 - t^2/6 by 1e-9), 1e-3, a generic
# angle, and pi - 1e-3 (the near-pi branch)
BAND_ANGLES = (1e-6, TAYLOR * (1 - 2e-3), 1e-3, 1.3, np.pi - 1e-3)


def _rotated_refs(oracle, low, sc, xs, seed):
    """Per-trajectory references: a random SO(3) rotation and a random target for most trajectories; for trajectories
    b = 0, 1, ..., one per band, the placement of the cost frame at the evaluated terminal state composed with a rotation
    by that band's angle about a random axis and a translation of ~0.05, so that rMf at knot T has that angle."""
    rng = np.random.default_rng(seed)
    B, T = low.B, low.T
    refs = np.zeros((B, 12))
    for b in range(B):
        refs[b, :9] = chains.random_rotation(rng).reshape(9)
        refs[b, 9:] = sc["frame_refs"][b, 9:] + rng.uniform(-0.05, 0.05, 3)
    model = sc["terminal"].state.pinocchio
    fr = model.frames[model.getFrameId("EE")]
    for b, angle in enumerate(BAND_ANGLES):
        R, p = oracle.frame_placement(low.desc.chain, xs[T, b, :2], fr.parent, fr.placement.rotation, fr.placement.translation)
        dR, dp = chains.random_rotation(rng, angle), rng.uniform(-0.05, 0.05, 3)
        # Mref = oMf * (dR, dp)^-1  =>  rMf = (dR, dp)
        refs[b, :9] = R.dot(dR.T).reshape(9)
        refs[b, 9:] = p - R.dot(dR.T).dot(dp)
    return refs


def _with_refs(sc, refs):
    sc = dict(sc)
    sc["frame_refs"] = refs
    return sc


@pytest.mark.parametrize("chain,actuator", [("planar", "sea"), ("planar", "vsa"), ("general", "sea"), ("general", "vsa")])
def test_calc_and_calcdiff_with_rotated_references_in_every_log_band(oracle, chain, actuator):
    """frame_refs with random rotations, and references that put the terminal residual's rotation in each band of the
    log (checked on the oracle's log6 of rMf); on the planar arm of C2 / C3 and on the general chain, whose cost frame is
    itself rotated on its joint.  Both sweeps against the oracle."""
    if chain == "planar":
        sc = scenarios.SCENARIOS["two_dof_sea" if actuator == "sea" else "two_dof_vsa_boxddp"](B=70, T=5, seed=3)
    else:
        sc = chains.problem(chain, actuator, B=70, T=5, seed=3)
    low0 = scenarios.lower(sc)
    xs, us = gc.random_candidate(low0, 1)
    refs = _rotated_refs(oracle, low0, sc, xs, seed=6)
    low = scenarios.lower(_with_refs(sc, refs))
    # the residual rotation of knot T really lies in each band
    model = sc["terminal"].state.pinocchio
    fr = model.frames[model.getFrameId("EE")]
    for b, angle in enumerate(BAND_ANGLES):
        R, p = oracle.frame_placement(low.desc.chain, xs[low.T, b, :2], fr.parent, fr.placement.rotation,
                                      fr.placement.translation)
        Rr = refs[b, :9].reshape(3, 3)
        th = np.linalg.norm(oracle.log6(Rr.T.dot(R), Rr.T.dot(p - refs[b, 9:]))[3:])
        assert abs(th - angle) < 1e-6 * max(angle, 1e-3), (b, th, angle)
    e = gc.engine(low)
    ref = oracle.calc_diff(low, xs, us)
    gc.assert_records_match(*gc.run_calc_diff(e, xs, us), ref=ref)   # (a mismatch is reported with its (t, b))
    gc.assert_records_match(None, gc.run_calc(e)[1], None, ref=ref)


def test_residual_rotation_of_exactly_pi_gives_the_oracles_cost(oracle):
    """References turned by exactly pi against the frame, about one of the reference frame's own axes: log3 has two
    answers there (w and -w), and which one either side takes depends on the last bit of R's off-diagonal pairs, so
    residuals and derivatives are not comparable; only the cost is.  1/2 |r|^2 is the same for both (|w| = pi, and
    V(-w) = V(w)^T keeps |v|).  (About a general axis it is not even that: the near-pi branch picks the sign of each
    component of w on its own, and two sides that round R differently can return different sign patterns, which are
    not logs of R -- tests/test_oracle_geometry.py shows the tie.)  Compared to 1e-7 relative: theta = acos((tr - 1) / 2)
    at a trace within a few eps of -1 is pi to ~sqrt(eps), and so are the square roots of the near-zero diagonal terms."""
    import torch
    sc = chains.problem("general", "sea", B=70, T=2, seed=8)
    low0 = scenarios.lower(sc)
    xs, us = gc.random_candidate(low0, 2)
    rng = np.random.default_rng(12)
    model = sc["terminal"].state.pinocchio
    fr = model.frames[model.getFrameId("EE")]
    refs = np.array(sc["frame_refs"], dtype=float)
    for b in range(low0.B):
        R, p = oracle.frame_placement(low0.desc.chain, xs[low0.T, b, :2], fr.parent, fr.placement.rotation,
                                      fr.placement.translation)
        dR = -np.eye(3)
        dR[b % 3, b % 3] = 1.0                      # a half turn about axis b % 3 (its own inverse)
        refs[b, :9] = R.dot(dR).reshape(9)
        refs[b, 9:] = p + rng.uniform(-0.05, 0.05, 3)
    low = scenarios.lower(_with_refs(sc, refs))
    e = gc.engine(low)
    e.region(_abi.R_XS).copy_(torch.as_tensor(xs))
    e.region(_abi.R_US).copy_(torch.as_tensor(us))
    e.calc()
    gc.sync()
    _, cost, _ = oracle.calc_diff(low, xs, us, diff=False)
    got = gc.to_np(e.region(_abi.R_COST))[low.T]
    err = np.abs(got - cost[low.T]) / np.abs(cost[low.T])
    assert err.max() < 1e-7, "cost at a half turn: %.3e relative (trajectory %d)" % (err.max(), err.argmax())


@pytest.mark.parametrize("actuator", ["sea", "vsa"])
def test_closed_form_reach_switch_falls_back_with_rotated_references(oracle, monkeypatch, actuator):
    """ASLR_PLANAR_REACH=1 asks for the closed-form planar reach residual, which needs identity reference rotations:
    with rotated frame_refs fill_planar_reach declines, so calc / calcDiff and the forward pass give the same bits as
    with the switch off (and match the oracle)."""
    sc = scenarios.SCENARIOS["two_dof_sea" if actuator == "sea" else "two_dof_vsa_boxddp"](B=70, T=20, seed=5)
    low0 = scenarios.lower(sc)
    xs, _ = gc.random_candidate(low0, 5)      # the candidate gc.forward_inputs draws below
    low = scenarios.lower(_with_refs(sc, _rotated_refs(oracle, low0, sc, xs, seed=9)))
    sp = scenarios.solver_params(sc)
    xs, us, K, k, gaps = gc.forward_inputs(oracle, low, sp, 5, False)
    out = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("ASLR_PLANAR_REACH", flag)   # (read when the handle is created)
        e = gc.run_forward(low, sp, xs, us, K, k, gaps, 1)
        fwd = [e.region(r).clone() for r in (_abi.R_XS_TRY, _abi.R_US_TRY, _abi.R_TRAJ_F)]
        gc.run_calc_diff(e, xs, us)
        out[flag] = fwd + [e.region(r).clone() for r in (_abi.R_XNEXT, _abi.R_COST, _abi.R_DERIV)]
    for a, b in zip(out["0"], out["1"]):
        gc.same_bits(a, b, "ASLR_PLANAR_REACH / ASLR_NO_PLANAR = 0 and = 1")
    _, cost, deriv = oracle.calc_diff(low, xs, us)
    assert gc.relerr(gc.to_np(out["1"][4]), cost) < 1e-11
    assert gc.relerr(gc.to_np(out["1"][5]), deriv) < 1e-9
    for a in range(_abi.NALPHA):
        _, _, cost_try, fail = oracle.forward_pass(low, sp, 0.5 ** a, xs, us, K, k)
        got = gc.to_np(out["1"][2][_abi.TF_COST_TRY0 + a])
        ok = fail == 0
        assert ok.mean() > 0.5 and gc.relerr(got[ok], cost_try[ok]) < 1e-9


# ---------------------------------------------------------------------------------------------
# planar against general on the same problem
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["two_dof_sea", "two_dof_vsa_boxddp"])
def test_general_path_on_the_planar_scenarios_matches_oracle(oracle, monkeypatch, name):
    """ASLR_NO_PLANAR=1 (read when the handle is created) sends the default C2 / C3 problems through the general 3-D
    recursion: calc / calcDiff and the forward pass of every step length against the oracle."""
    monkeypatch.setenv("ASLR_NO_PLANAR", "1")
    sc = scenarios.SCENARIOS[name](B=70, T=20, seed=1)
    low = scenarios.lower(sc)
    gc.check_calc_and_calc_diff(oracle, low)
    _check_forward(oracle, low, "SolverDDP")


@pytest.mark.parametrize("actuator", ["sea", "vsa"])
@pytest.mark.parametrize("chain", ["flipped", "tilted"])
def test_planar_switch_changes_nothing_where_the_detector_declines(monkeypatch, chain, actuator):
    """On the flipped (axes -z) and tilted (1e-3 rad) arms the planar detector declines, so ASLR_NO_PLANAR=0 and =1 run
    the same kernels: calc / calcDiff and forward-pass outputs must be the same bits."""
    import torch
    sc = chains.problem(chain, actuator, B=70, T=20, seed=7)
    low = scenarios.lower(sc)
    sp = scenarios.solver_params(sc, solver="SolverFDDP")
    xs, us = gc.random_candidate(low, 4)
    rng = np.random.default_rng(4)
    K = rng.uniform(-0.05, 0.05, (low.T, low.B, low.nu, low.nx))
    k = rng.uniform(-0.05, 0.05, (low.T, low.B, low.nu))
    gaps = rng.uniform(-0.05, 0.05, (low.T + 1, low.B, low.nx))
    out = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("ASLR_NO_PLANAR", flag)
        e = gc.run_forward(low, sp, xs, us, K, k, gaps, 0)
        res = [e.region(r).clone() for r in (_abi.R_XS_TRY, _abi.R_US_TRY, _abi.R_TRAJ_F)]
        gc.run_calc_diff(e, xs, us)
        out[flag] = res + [e.region(r).clone() for r in (_abi.R_XNEXT, _abi.R_COST, _abi.R_DERIV)]
    assert torch.isfinite(out["0"][4]).all()
    for a, b in zip(out["0"], out["1"]):
        gc.same_bits(a, b, "ASLR_PLANAR_REACH / ASLR_NO_PLANAR = 0 and = 1")
