"""Kernel-level forward pass on the path the 2-DoF workloads take by default: the horizon of a planar chain with T >= 16 is
rolled out in 2 - 4 launches (launch_forward, aslr_forward.inc.hpp; ASLR_PIPELINE picks the number), and a continuing
launch re-reads its state from XS_TRY and its dv / failure flag from the per-trajectory slots, skipping at the seam knot
what the launch before has already done there.  Every step length against the oracle's forwardPass on the inputs of
tests/_gpu_case.py, at the smallest split horizon (16), an odd one (17) and one where T / nseg truncates (37), with a
partial last wave (B = 70); and the FDDP terms no other test reads: the per-step-length dv (TF_DVTRY0..) with waves that
mix feasible and infeasible trajectories, and `Vxx f` (R_VXXF) of the backward sweeps.  The 7-joint team rollout does
not split; it is here for the FDDP terms.

What the seam handling is worth to these tests, measured by taking `!seam` out of one guard of rollout_body at a time: twelve
tests fail either way, and only they can (SolverDDP / SolverBoxDDP carry no gap terms) -- the nine two_dof_sea SolverFDDP
cases of test_split_forward_pass_matches_oracle_for_every_alpha that split (ASLR_PIPELINE unset, 3, 4) and the three of
test_number_of_segments_changes_no_bit.  Gaps contracted twice at the seam: xs_try off by 3.0 - 6.0 (relerr), us_try
0.17 - 1.2, trial costs 0.14 - 0.41, XS_TRY bits differ.  The seam knot's dv term counted twice: dv off by 1.1e-3 - 1.6e-2
of its bound's scale against the 1e-9 allowed, DVTRY bits differ, everything else unchanged.

Tolerances: 1e-9 relative on forward-pass outputs and 1e-8 on backward-pass outputs, as in tests/test_gpu_parity.py.
dv and Vxx f are sums with cancellation, so they are held to the same factors times the absolute sum of their terms:
what inputs that agree to that factor can move them by."""
import numpy as np
import pytest

from aslr_to_amd import _abi, scenarios

import _gpu_case as gc

pytestmark = pytest.mark.gpu

HORIZONS = (16, 17, 37)
PIPELINES = (None, "0", "3", "4")      # unset (two segments), the plain sequence, three segments, four
SEED = 5                               # (on the oracle alone no rollout of any case below fails or exceeds |x| = 3e3 with it)
# (scenario, its arguments, solver, control box of the running model or None)
PLANAR = [("two_dof_sea", dict(B=70), "SolverDDP", None),
          ("two_dof_sea", dict(B=70), "SolverFDDP", None),
          # torques boxed to +-0.5 and stiffness to [0.5, 4].  The candidate's torques are U(-1, 1) and its stiffness commands
          # U(0.1, 5), and the mild gains move them little: half of the torques and 1.4 / 4.9 of the stiffness commands lie
          # outside the box, so about 40 % of the rolled-out controls sit on a bound (0.37 - 0.41 on the oracle)
          ("two_dof_vsa_boxddp", dict(B=70), "SolverBoxDDP", ((-0.5, -0.5, 0.5, 0.5), (0.5, 0.5, 4.0, 4.0))),
          # double_pendulum turns about +y, so fill_planar (aslr_abi.hip) leaves it on the general 3-D chain and the launcher
          # rolls it out in ONE launch whatever ASLR_PIPELINE says: these two are the general-chain rollout at the same
          # horizons (B = 1: a wave with one team), not cases of the seam
          ("double_pendulum", dict(), "SolverDDP", None),
          ("double_pendulum", dict(), "SolverFDDP", None)]
TEAM = ("talos_arm_sea", dict(B=5), "SolverFDDP", None)


def _set_pipeline(monkeypatch, pl):
    # the launcher splits only planar chains with the closed-form reach off: neither switch may come from outside
    monkeypatch.delenv("ASLR_PLANAR_REACH", raising=False)
    monkeypatch.delenv("ASLR_NO_PLANAR", raising=False)
    if pl is None:
        monkeypatch.delenv("ASLR_PIPELINE", raising=False)
    else:
        monkeypatch.setenv("ASLR_PIPELINE", pl)      # (read when the handle is created)


_CASES = {}


def _case(oracle, name, kw, solver, box, T):
    """Inputs and the oracle's answers of one case, computed once and shared (read-only) by the tests below."""
    key = (name, tuple(sorted(kw.items())), solver, box, T)
    if key in _CASES:
        return _CASES[key]
    sc = scenarios.SCENARIOS[name](T=T, **kw)
    if box is not None:
        sc["running"][0].u_lb, sc["running"][0].u_ub = np.array(box[0]), np.array(box[1])
    low = scenarios.lower(sc)
    sp = _abi.default_solver_params(gc.SOLVERS[solver])
    fddp = solver == "SolverFDDP"
    # FDDP: odd trajectories feasible, even ones not -- every wave of 4 teams mixes the two kinds
    feasible = (np.arange(low.B) % 2).astype(np.int32) if fddp else 1
    xs, us, K, k, gaps, ref_b = gc.forward_inputs(oracle, low, sp, SEED, fddp, feasible=feasible if fddp else None, full=True)
    c = dict(low=low, sp=sp, fddp=fddp, feasible=feasible, xs=xs, us=us, K=K, k=k, gaps=gaps, box=box,
             vxxf=np.einsum("tbij,tbj->tbi", ref_b["Vxx"], gaps), ref=[])
    for a in range(_abi.NALPHA):
        c["ref"].append(oracle.forward_pass(low, sp, 0.5 ** a, xs, us, K, k, gaps if fddp else None,
                                            feasible if fddp else None))
    if fddp:   # dv = -sum_t f_t . Vxx_t (xs_t - xs_try_t) in extended precision, and the absolute sum of its terms
        f, V = gaps.astype(np.longdouble), ref_b["Vxx"].astype(np.longdouble)
        infeasible = (feasible == 0)
        c["dv"], c["dv_abs"] = [], []
        for a in range(_abi.NALPHA):
            d = xs.astype(np.longdouble) - c["ref"][a][0].astype(np.longdouble)
            c["dv"].append(np.where(infeasible, -np.einsum("tbi,tbij,tbj->b", f, V, d), 0.0).astype(np.float64))
            c["dv_abs"].append(np.where(infeasible, np.einsum("tbi,tbij,tbj->b", np.abs(f), np.abs(V), np.abs(d)),
                                        0.0).astype(np.float64))
    _CASES[key] = c
    return c


def _run(c):
    return gc.run_forward(c["low"], c["sp"], c["xs"], c["us"], c["K"], c["k"], c["gaps"], c["feasible"],
                          vxxf=c["vxxf"] if c["fddp"] else None)


def _check_against_oracle(c, e, label):
    low = c["low"]
    oks, _ = gc.assert_forward_matches(*gc.forward_outputs(e), c["ref"])
    worst_dv = 0.0
    clamped = []
    for a, ok in enumerate(oks):
        us_try = c["ref"][a][1]
        assert ok.mean() > 0.9, (a, ok.mean())       # a condition on the inputs: the oracle alone meets it
        got = gc.to_np(e.traj_f(_abi.TF_COST_TRY0 + a))
        np.testing.assert_array_equal(np.isnan(got), ~ok, err_msg="NaN pattern of the trial costs, alpha index %d" % a)
        np.testing.assert_array_equal(gc.to_np(e.traj_i(_abi.TI_TRYFAIL0 + a))[ok], 0)
        if c["box"] is not None:   # share of the controls of the LAST segment of any split that sit on a bound
            late = us_try[low.T - low.T // 4:, ok]
            clamped.append(((late == np.array(c["box"][0])) | (late == np.array(c["box"][1]))).mean())
        if c["fddp"]:
            dv = gc.to_np(e.traj_f(_abi.TF_DVTRY0 + a))
            worst_dv = max(worst_dv, (np.abs(dv - c["dv"][a])[ok] / (1.0 + c["dv_abs"][a][ok])).max())
            assert (dv[c["feasible"] == 1] == 0.0).all()
            assert (np.abs(c["dv"][a][ok & (c["feasible"] == 0)]) > 0.0).all()
    print("%s: dv error over (1 + sum |f|'|Vxx||dx|) %.2e" % (label, worst_dv))
    assert worst_dv < 1e-9
    if clamped:
        print("%s: share of the controls past the last seam that sit on a bound %.3f .. %.3f" % (label, min(clamped), max(clamped)))
        # the clamp really binds after the last seam: (1/2 + 1.4/4.9) / 2 = 0.39 is what the recipe of the box gives; the
        # last quarter of the smallest case holds 4 knots x 70 trajectories x 4 controls, a sampling error of 0.015
        assert min(clamped) > 0.3, clamped


@pytest.mark.parametrize("pl", PIPELINES, ids=lambda p: "pipeline-%s" % (p or "unset"))
@pytest.mark.parametrize("T", HORIZONS)
@pytest.mark.parametrize("name,kw,solver,box", PLANAR, ids=["%s-%s" % (c[0], c[2]) for c in PLANAR])
def test_split_forward_pass_matches_oracle_for_every_alpha(oracle, monkeypatch, name, kw, solver, box, T, pl):
    """xs_try, us_try, the trial costs with their NaN pattern and (SolverFDDP) dv of all NALPHA step lengths."""
    c = _case(oracle, name, kw, solver, box, T)
    _set_pipeline(monkeypatch, pl)
    _check_against_oracle(c, _run(c), "%s %s T=%d ASLR_PIPELINE=%s" % (name, solver, T, pl))


def test_team_rollout_fddp_terms_match_oracle(oracle, monkeypatch):
    """rollout_team_kernel<7, FDDP> at B = 5, T = 17, feasible and infeasible trajectories side by side: the gap
    contraction and dv, which the 7-joint rollout otherwise runs inside full solves only."""
    name, kw, solver, box = TEAM
    c = _case(oracle, name, kw, solver, box, 17)
    _set_pipeline(monkeypatch, None)
    _check_against_oracle(c, _run(c), "%s %s T=17" % (name, solver))


@pytest.mark.parametrize("T", HORIZONS)
@pytest.mark.parametrize("name,kw,solver,box", PLANAR, ids=["%s-%s" % (c[0], c[2]) for c in PLANAR])
def test_number_of_segments_changes_no_bit(oracle, monkeypatch, name, kw, solver, box, T):
    """One, two, three and four launches over the horizon: XS_TRY, US_TRY, the trial costs, dv and the failure flags are
    the same bits (a continuing launch resumes from what the one before stored, and repeats nothing at the seam)."""
    c = _case(oracle, name, kw, solver, box, T)
    out = {}
    for pl in PIPELINES:
        _set_pipeline(monkeypatch, pl)
        e = _run(c)
        tf, ti = e.region(_abi.R_TRAJ_F), e.region(_abi.R_TRAJ_I)
        out[pl] = [e.region(_abi.R_XS_TRY).clone(), e.region(_abi.R_US_TRY).clone(),
                   tf[_abi.TF_COST_TRY0:_abi.TF_COST_TRY0 + _abi.NALPHA].clone(),
                   tf[_abi.TF_DVTRY0:_abi.TF_DVTRY0 + _abi.NALPHA].clone(),
                   ti[_abi.TI_TRYFAIL0:_abi.TI_TRYFAIL0 + _abi.NALPHA].clone(), e.region(_abi.R_COST_TRY).clone()]
    for pl in PIPELINES[1:]:
        for what, a, b in zip(("XS_TRY", "US_TRY", "COST_TRY", "DVTRY", "TRYFAIL", "node costs"), out[None], out[pl]):
            gc.same_bits(a, b, "%s differs between ASLR_PIPELINE unset and %s" % (what, pl))


@pytest.mark.parametrize("pl", PIPELINES, ids=lambda p: "pipeline-%s" % (p or "unset"))
def test_failure_before_the_seam_is_carried_across_it(oracle, monkeypatch, pl):
    """tests/test_gpu_parity.py::test_forward_error_is_skipped_like_crocoddyl with the overflow in the FIRST segment only
    (T = 40, k = -1e200 on knots 0..5, zero after) and launches that continue from it.  This pins the NaN pattern of the
    trial costs and the failure flags at the end of the pass; it cannot tell a flag carried across the seam from one set
    again, because the state a continuing launch resumes from is itself out of range."""
    sc = scenarios.two_dof_sea(B=4, T=40)
    low = scenarios.lower(sc)
    sp = scenarios.solver_params(sc)
    xs = np.zeros((low.T + 1, low.B, low.nx))
    us = np.zeros((low.T, low.B, low.nu))
    K = np.zeros((low.T, low.B, low.nu, low.nx))
    k = np.zeros((low.T, low.B, low.nu))
    k[:6] = -1e200
    _set_pipeline(monkeypatch, pl)
    e = gc.run_forward(low, sp, xs, us, K, k, np.zeros_like(xs), 1)
    failed = 0
    for a in range(_abi.NALPHA):
        _, _, _, fail = oracle.forward_pass(low, sp, 0.5 ** a, xs, us, K, k)
        np.testing.assert_array_equal(np.isnan(gc.to_np(e.traj_f(_abi.TF_COST_TRY0 + a))), fail != 0)
        np.testing.assert_array_equal(gc.to_np(e.traj_i(_abi.TI_TRYFAIL0 + a)) != 0, fail != 0)
        failed += int((fail != 0).sum())
    assert failed > 0


VXXF_CASES = [("two_dof_sea", dict(B=70, T=5), hs) for hs in (0, 1, 2, 4)] + [("talos_arm_sea", dict(B=5, T=3), 0)]


@pytest.mark.parametrize("name,kw,hs", VXXF_CASES)
def test_backward_pass_stores_vxx_times_gap_and_dg_dq_for_fddp(oracle, monkeypatch, name, kw, hs):
    """R_VXXF, what the FDDP rollout reads for dv: Vxx f of every knot from an infeasible candidate, through each
    decomposition of the backward sweep (ASLR_BWD_HS; 0: the default of the size), against the oracle's Vxx times the
    input gaps.  Inputs and the factor 1e-8 of test_gpu_parity.test_backward_pass_matches_oracle."""
    if hs:
        monkeypatch.setenv("ASLR_BWD_HS", str(hs))
    else:
        monkeypatch.delenv("ASLR_BWD_HS", raising=False)
    sc = scenarios.SCENARIOS[name](**kw)
    low = scenarios.lower(sc)
    sp = scenarios.solver_params(sc, solver="SolverFDDP")
    xs, us, deriv, gaps = gc.backward_inputs(oracle, low, 3)
    xreg = 1e-3
    e = gc.engine(low)
    e.region(_abi.R_VXXF).fill_(float("nan"))
    out = gc.run_backward(e, sp, us, deriv, gaps, xreg, 0)
    ref = oracle.backward_pass(low, sp, deriv, gaps, us, xreg, 0)
    gc.assert_backward_matches(out, ref, 1e-8, fields=())     # (no failure on either side; test_gpu_parity.py compares the fields)
    V = ref["Vxx"].astype(np.longdouble)
    want = np.einsum("tbij,tbj->tbi", V, gaps.astype(np.longdouble)).astype(np.float64)
    sens = np.einsum("tbij,tbj->tbi", np.abs(V), np.abs(gaps).astype(np.longdouble)).astype(np.float64)
    got = gc.to_np(e.region(_abi.R_VXXF))
    assert np.isfinite(got).all()
    err = (np.abs(got - want) / (1.0 + sens)).max()
    print("%s hs=%d: Vxx f error over (1 + |Vxx||f|) %.2e" % (name, hs, err))
    assert err < 1e-8, "R_VXXF: %g" % err
    # the same sweep's dg = sum Qu.k - sum Vx.f and dq = -sum k.Quu k + sum f.Vxx f (TF_DG / TF_DQ), which select_kernel
    # adds dv to: against the oracle's, over the absolute sum of their terms (-k.Quu k has one sign: no cancellation in it)
    f = gaps.astype(np.longdouble)
    fvf = np.einsum("tbi,tbij,tbj->b", f, V, f)
    dg_abs = (np.abs(ref["Qu"]) * np.abs(ref["k"])).sum(axis=(0, 2)) + (np.abs(ref["Vx"]) * np.abs(gaps)).sum(axis=(0, 2))
    dq_abs = np.abs(ref["d2"] - fvf).astype(np.float64) + np.einsum("tbi,tbij,tbj->b", np.abs(f), np.abs(V), np.abs(f)).astype(np.float64)
    err_g = (np.abs(gc.to_np(e.traj_f(_abi.TF_DG)) - ref["d1"]) / (1.0 + dg_abs)).max()
    err_q = (np.abs(gc.to_np(e.traj_f(_abi.TF_DQ)) - ref["d2"]) / (1.0 + dq_abs)).max()
    print("%s hs=%d: dg error over its absolute sum %.2e, dq %.2e" % (name, hs, err_g, err_q))
    assert err_g < 1e-8, "TF_DG: %g" % err_g
    assert err_q < 1e-8, "TF_DQ: %g" % err_q
