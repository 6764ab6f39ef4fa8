"""The per-knot action-model switch of every sweep kernel, kernel by kernel, against the CPU oracle on horizons of THREE
distinct running models (tests/_model_switch.py: they differ in dt, presence of a control box, box values, cost weights, K
and B; SEQ7 has a switch after the first knot, a repeat, a return to model 0 and a switch into the last running knot,
SEQ_CYCLE a switch at every knot).  tests/test_model_switch_host.py holds, on the oracle alone, every condition relied on
here: the box binds per model, the clamp binds, the rollouts stay bounded, and each compared output moves by more than 1e-6
under a node table that is one knot off -- a thousand times the loosest tolerance below.

Shapes: B = 5, T = 7 at 7 joints (a block per trajectory; idle teams in the rollout block), B = 70, T = 7 at 2 joints (a
partial last wave), B = 70, T = 17 for the 2-joint rollout split over 2 - 4 launches.  Tolerances are the project's own, from
the helpers: gc.assert_records_match (1e-11 on states and costs, 1e-9 on records), gc.assert_backward_matches at 1e-8,
gc.assert_forward_matches (1e-9), 1e-9 for the extension kernels, 1e-6 on xs / us and 1e-4 on the cost for solves.

What an off-by-one in the model index is worth to these tests, shown once by hand in a scratch build (not committed):
 - `pre_m = node_model_at(a, tt + 1 < T ? tt + 1 : tt)` in the prefetch of the block backward kernel (aslr_backward_blk.inc.hpp):
   the two feasible SolverBoxDDP cases of test_backward_pass_takes_each_knots_box that run it fail (talos_arm_sea: K off by
   56 in relerr; talos_arm_vsa: 50) and so do both solves of test_cold_solves_with_a_switch_at_every_knot_match_oracle
   (iteration counts); every other backward case passes, as it must: the kernel uses the index for the box alone;
 - `m_loaded` never reset in rollout_team_kernel (aslr_forward_team.inc.hpp: `if (m_loaded < 0)`), so that the constants of
   the first model stay loaded: all four cases of test_team_rollout_reloads_what_it_caches_per_model fail (xs_try of step
   length 1 off by 3.7 - 7.5) and both solves."""
import numpy as np
import pytest

import _ext_call as ext
import _gpu_case as gc
import _model_switch as ms
import _parity
import _plant_sens as ps
import _policy as pol
import _sensitivity as sens
from aslr_to_amd import _abi

pytestmark = pytest.mark.gpu

BWD_SWITCHES = ("ASLR_BWD_HS", "ASLR_BLK_MFMA")
PIPELINES = (None, "0", "3", "4")      # unset (two segments), the plain sequence, three segments, four


# ---------------------------------------------------------------------------------------------
# (a) calc / calcDiff
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B,table", ms.CALC_CASES)
def test_calc_and_calcdiff_take_each_knots_model(oracle, name, B, table):
    """calcDiff, calc alone and calcDiff at a second point (whose sweep does not rewrite the model-only record chunks: with
    weights that differ per knot they must have been written per knot); with a table against tests/_traj_oracle.py"""
    _, low = ms.problem(name, B, 7, ms.SEQ7, table)
    gc.check_calc_and_calc_diff(ms.oracle_for(oracle, low), low)


# ---------------------------------------------------------------------------------------------
# (b) backward pass
# ---------------------------------------------------------------------------------------------
_MFMA = ({"ASLR_BLK_MFMA": "1"}, {"ASLR_BLK_MFMA": "0"})
# (scenario, B, solver, the launch switches of each run; two runs: bit-equal to each other)
BACKWARD = [
    ("talos_arm_sea", 5, "SolverBoxDDP", _MFMA),                      # block kernel, per-lane gains
    ("talos_arm_sea", 5, "SolverBoxDDP", ({"ASLR_BWD_HS": "2"},)),    # register-column sweep, limL and the team QP
    ("talos_arm_sea", 5, "SolverDDP", ({},)),
    ("talos_arm_vsa", 5, "SolverBoxDDP", _MFMA),                      # block kernel, wave_gains
    ("two_dof_vsa_boxddp", 70, "SolverBoxDDP", ({},)),
    ("two_dof_vsa_boxddp", 70, "SolverBoxDDP", ({"ASLR_BWD_HS": "1"},)),
    ("two_dof_vsa_boxddp", 70, "SolverBoxDDP", ({"ASLR_BWD_HS": "2"},)),
    ("two_dof_vsa_boxddp", 70, "SolverBoxDDP", ({"ASLR_BWD_HS": "4"},)),
    ("two_dof_sea", 70, "SolverFDDP", ({},)),
]


def _switches(runs):
    return "+".join(",".join("%s=%s" % kv for kv in env.items()) or "default" for env in runs)


@pytest.mark.parametrize("feasible", [0, 1])
@pytest.mark.parametrize("name,B,solver,runs", BACKWARD, ids=["%s-%s-%s" % (c[0], c[2], _switches(c[3])) for c in BACKWARD])
def test_backward_pass_takes_each_knots_box(oracle, monkeypatch, name, B, solver, runs, feasible):
    """K, k, Qu, Vx, Vxx, d1, d2 and the stopping measure against the oracle; from a feasible candidate under SolverBoxDDP the
    clamped set is the oracle's knot by knot: none on the knots of the model without limits, and C's narrower box clamps
    where A's does not.  (SolverFDDP: d1 / d2 of the oracle are the sweep's dg / dq, which tests/test_gpu_forward_seam.py
    holds to their own measure.)"""
    c = ms.backward_case(oracle, name, B, solver, feasible)
    low, ref = c["low"], c["ref"]
    fields = ("K", "k", "Qu", "Vx", "Vxx", "stop") if solver == "SolverFDDP" else gc.BACKWARD_FIELDS
    outs = []
    for env in runs:
        for sw in BWD_SWITCHES:
            monkeypatch.delenv(sw, raising=False)
        for sw, v in env.items():
            monkeypatch.setenv(sw, v)       # (read when the handle is created)
        out = gc.run_backward(gc.engine(low), c["sp"], c["us"], c["deriv"], c["gaps"], ms.XREG, feasible, k0=c["k0"])
        gc.assert_backward_matches(out, ref, 1e-8, fields=fields)
        if c["boxed"]:
            np.testing.assert_array_equal(out["Qu"] == 0.0, ref["Qu"] == 0.0)
            assert not (out["Qu"][ms.knots_of(low, 1)] == 0.0).any()
        outs.append(out)
    if len(outs) == 2:
        for f in gc.BACKWARD_FIELDS:
            np.testing.assert_array_equal(outs[0][f], outs[1][f], err_msg=f)


# ---------------------------------------------------------------------------------------------
# (c) forward pass
# ---------------------------------------------------------------------------------------------
def _set_pipeline(monkeypatch, pl):
    # the launcher splits only planar chains with the closed-form reach off: neither switch may come from outside
    monkeypatch.delenv("ASLR_PLANAR_REACH", raising=False)
    monkeypatch.delenv("ASLR_NO_PLANAR", raising=False)
    if pl is None:
        monkeypatch.delenv("ASLR_PIPELINE", raising=False)
    else:
        monkeypatch.setenv("ASLR_PIPELINE", pl)      # (read when the handle is created)


def _check_forward(c):
    """every step length on the trajectories of c["keep"] (all of them but in ms.UNBOUNDED_FORWARD_CASES); boxed: the controls
    that sit on a bound of their own knot's box are the oracle's, and none on a knot of the model without limits"""
    low, keep = c["low"], c["keep"]
    e = gc.run_forward(low, c["sp"], c["xs"], c["us"], c["K"], c["k"], c["gaps"], c["feasible"], vxxf=c["vxxf"] if c["fddp"] else None)
    XT, UT, costs = gc.forward_outputs(e)
    refs = [(r[0][:, keep], r[1][:, keep], r[2][keep], r[3][keep]) for r in c["ref"]]
    oks, _ = gc.assert_forward_matches(XT[:, :, keep], UT[:, :, keep], costs[:, keep], refs)
    assert all(ok.all() for ok in oks)
    if c["boxed"]:
        lb, ub = (v[:, keep] for v in ms.bounds(low))
        hit = 0
        for a in range(_abi.NALPHA):
            got, want = UT[a][:, keep], refs[a][1]
            np.testing.assert_array_equal((got == lb) | (got == ub), (want == lb) | (want == ub), err_msg="alpha index %d" % a)
            free, beyond = ms.knots_of(low, 1), lambda u: (u < lb[0]) | (u > ub[0])     # (knot 0 is A's: beyond A's box)
            np.testing.assert_array_equal(beyond(got[free]), beyond(want[free]), err_msg="a control on a B knot was clipped")
            hit += int(((got == lb) | (got == ub)).sum())
        assert hit > 0


_TEAM = [c for c in ms.FORWARD_CASES if c[2] == 7]
_SPLIT = [c for c in ms.FORWARD_CASES if c[2] == 17]


@pytest.mark.parametrize("name,B,T,solver,table", _TEAM, ids=["%s-%s%s" % (c[0], c[3], "-table" if c[4] else "") for c in _TEAM])
def test_team_rollout_reloads_what_it_caches_per_model(oracle, monkeypatch, name, B, T, solver, table):
    """rollout_team_kernel on SEQ7: dt, K, 1 / B, has_lim and the box behind `mi != m_loaded`, with a return to model 0; with
    a table the box comes from the table's rows and has_u_limits from the knot's model"""
    _set_pipeline(monkeypatch, None)
    _check_forward(ms.forward_case(oracle, name, B, T, solver, table))


@pytest.mark.parametrize("pl", PIPELINES, ids=lambda p: "pipeline-%s" % (p or "unset"))
@pytest.mark.parametrize("name,B,T,solver,table", _SPLIT, ids=["%s-%s" % (c[0], c[3]) for c in _SPLIT])
def test_split_rollout_enters_every_segment_on_a_switch(oracle, monkeypatch, name, B, T, solver, table, pl):
    """the 2-joint rollout at T = 17 in one to four launches, a switch at every knot: a launch that re-enters mid-horizon
    starts on another model than the one before it ended on"""
    _set_pipeline(monkeypatch, pl)
    _check_forward(ms.forward_case(oracle, name, B, T, solver, table))


# ---------------------------------------------------------------------------------------------
# (d) extension kernels that index the model per knot
# ---------------------------------------------------------------------------------------------
SENS_FIELDS = ("stiffness", "motor_inertia", "x0", "costate")
_SENS_TO_BATCH_MAJOR = {"stiffness": (1, 0), "motor_inertia": (1, 0), "x0": (1, 0), "costate": (1, 0, 2)}
_PS_TO_BATCH_MAJOR = {"dx_dstiffness": (1, 0, 2, 3), "dx_dmotor_inertia": (1, 0, 2, 3), "dxT_dstiffness": (0, 1, 2),
                      "dxT_dmotor_inertia": (0, 1, 2), "dcost_dstiffness": (1, 0), "dcost_dmotor_inertia": (1, 0),
                      "x_var": (1, 0, 2), "u_var": (1, 0, 2)}


def _cost_sensitivity(e):
    """aslr_cost_sensitivity (what Engine.cost_sensitivity calls) through the guarded call -> batch-major arrays"""
    nj = e.nx // 4
    shapes = {"stiffness": (nj, e.B), "motor_inertia": (nj, e.B), "x0": (e.nx, e.B), "costate": (e.T + 1, e.B, e.nx)}
    outs = ext.outputs(e.device, shapes, SENS_FIELDS, perms=_SENS_TO_BATCH_MAJOR)
    return ext.call(e, "aslr_cost_sensitivity", [e.handle] + [outs.get(k) for k in SENS_FIELDS] + [e._stream()], outs)


def _plant_sensitivity(e, vk, vb):
    nj = e.nx // 4
    shapes = {"dx_dstiffness": (e.T + 1, e.B, e.nx, nj), "dx_dmotor_inertia": (e.T + 1, e.B, e.nx, nj),
              "dxT_dstiffness": (e.B, e.nx, nj), "dxT_dmotor_inertia": (e.B, e.nx, nj), "dcost_dstiffness": (nj, e.B),
              "dcost_dmotor_inertia": (nj, e.B), "x_var": (e.T + 1, e.B, e.nx), "u_var": (e.T, e.B, e.nu)}
    outs = ext.outputs(e.device, shapes, ps.OUTPUTS, perms=_PS_TO_BATCH_MAJOR)
    args = [e.handle, ext.dev(e.device, vk, (1, 0)), ext.dev(e.device, vb, (1, 0))]
    return ext.call(e, "aslr_policy_plant_sensitivity", args + [outs.get(k) for k in ps.OUTPUTS] + [e._stream()], outs)


_EXT_IDS = ["%s%s" % (c[0], "-table" if c[2] else "") for c in ms.EXT_CASES]


@pytest.mark.parametrize("name,B,table", ms.EXT_CASES, ids=_EXT_IDS)
def test_adjoint_sweep_takes_each_knots_model(oracle, name, B, table):
    """aslr_cost_sensitivity against tests/_sensitivity.expected: dt, K and 1 / B of each knot's own model in the costates
    and in the gradients"""
    c = ms.ext_case(oracle, name, B, table)
    low = c["low"]
    want = sens.expected(oracle, low, c["xs"], c["us"])
    e = gc.engine(low)
    gc._upload(e, XS=c["xs"], US=c["us"])
    got = _cost_sensitivity(e)
    for k in SENS_FIELDS:
        assert got[k].shape == want[k].shape and np.abs(want[k]).max() > 1e-3, k
        gc._assert_close("%s %s" % (name, k), got[k], want[k], 1e-9)


@pytest.mark.parametrize("name,B,table", ms.EXT_CASES, ids=_EXT_IDS)
def test_plant_sensitivity_takes_each_knots_model(oracle, name, B, table):
    """aslr_policy_plant_sensitivity against tests/_plant_sens.expected, fed the device's own gains"""
    c = ms.ext_case(oracle, name, B, table)
    low = c["low"]
    e, K = ext.with_gains(c)
    vk, vb = ps.variances(low, 37)
    got = _plant_sensitivity(e, vk, vb)
    want = ps.expected(oracle, low, c["xs"], c["us"], K, vk, vb)
    for k in ps.OUTPUTS:
        assert got[k].shape == want[k].shape and np.abs(want[k]).max() > 1e-6, k
        gc._assert_close("%s %s" % (name, k), got[k], want[k], 1e-9)


@pytest.mark.parametrize("table", [False, True], ids=["plain", "table"])
def test_two_joint_policy_rollout_takes_each_knots_model_and_box(oracle, table):
    """aslr_policy_rollout on two_dof_sea with the clamp on, no plant arrays (every knot runs on its own model's K and B),
    against tests/_policy.rollout with the device's own gains"""
    c = ms.ext_case(oracle, "two_dof_sea", 70, table)
    low, S = c["low"], ms.POLICY_S
    e, K = ext.with_gains(c)
    pert = ms.policy_perturbations(low, S)
    got = ext.policy_rollout(e, "aslr_policy_rollout", S, pert, clamp=True)
    want = pol.rollout(oracle, low, c["xs"], c["us"], K, S, clamp=True, **pert)
    assert (want["failed_knot"] == -1).all() and want["bound"].any() and not want["bound"].all()
    np.testing.assert_array_equal(got["failed_knot"], want["failed_knot"])
    for k in pol.OUTPUTS:
        gc._assert_close("policy roll-out %s" % k, got[k], want[k], 1e-9)
    lb, ub = (v.transpose(1, 0, 2)[:, None] for v in ms.bounds(low))     # [B, 1, T, nu]
    np.testing.assert_array_equal((got["us"] == lb) | (got["us"] == ub), (want["us"] == lb) | (want["us"] == ub))


# ---------------------------------------------------------------------------------------------
# (e) full solves
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,solver", ms.SOLVE_CASES)
def test_cold_solves_with_a_switch_at_every_knot_match_oracle(oracle, name, solver):
    """B = 3, T = 30, SEQ_CYCLE, maxiter = 40 from the empty candidate: iteration counts and status words equal, xs / us within
    1e-6 relative to the size of the iterates and the cost within 1e-4, the solution inside each knot's own box and on a bound
    on some A knot and some C knot.  (tests/test_model_switch_host.py: the oracle's own result moves by 1.3e-10 at most when x0
    is scaled by 1 + 1e-14, and no count moves; the 7-joint SEA arm runs to the iteration cap without converging, the
    7-joint VSA arm converges on all three.)"""
    c = ms.solve_case(oracle, name, solver)
    low, ref = c["low"], c["ref"]
    _, g = gc.solve_gpu(low, c["sp"], poll_every=4)
    np.testing.assert_array_equal(g["traj_i"][_abi.TI_ITER], ref["traj_i"][_abi.TI_ITER])
    _parity.assert_status_words_match(g["traj_i"][_abi.TI_STATUS], ref["traj_i"][_abi.TI_STATUS])
    scale = max(1.0, np.abs(ref["xs"]).max(), np.abs(ref["us"]).max())
    dx, du = np.abs(g["xs"] - ref["xs"]).max(), np.abs(g["us"] - ref["us"]).max()
    cost_r = ref["traj_f"][_abi.TF_COST]
    dc = (np.abs(g["traj_f"][_abi.TF_COST] - cost_r) / np.maximum(1.0, np.abs(cost_r))).max()
    print("%s %s: iterations %s, dx %.2e du %.2e (scale %.2e) dcost %.2e" % (name, solver, ref["traj_i"][_abi.TI_ITER], dx, du, scale, dc))
    assert dx < 1e-6 * scale and du < 1e-6 * scale and dc < 1e-4
    lb, ub = ms.bounds(low)
    U = g["us"]
    assert (U >= lb).all() and (U <= ub).all()
    onb = ms.on_bound(low, U)
    assert onb[ms.knots_of(low, 0)].any() and onb[ms.knots_of(low, 2)].any()
