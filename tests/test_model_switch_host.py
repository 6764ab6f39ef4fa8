"""The conditions tests/test_gpu_model_switch.py relies on, on the CPU oracle alone (no GPU): with them met, a failure of a
GPU test there can only be the kernel's.

 - the box binds in the backward sweeps, per boxed model, and never on the knots of the model without limits;
 - the clamp binds in the forward passes, on A's knots and on C's, at their different bounds;
 - no rollout of any forward case fails or grows beyond |x| = 3e3 (the condition by which ms.SEED was chosen);
 - the tests can see an off-by-one: every compared output moves by more than 1e-6 (gc.relerr) when its reference is computed
   with the node table rolled by one knot (ms.shifted) -- a thousand times the loosest per-kernel tolerance, 1e-9;
 - the full-solve cases are conditioned: scaling x0 by (1 + 1e-14) moves no iteration count and the iterates by less than
   the bound of the GPU test.

Measured (printed by each test): clamped shares of Qu on the knots of A / C: talos_arm_sea 0.83 / 0.84, talos_arm_vsa
0.39 / 0.55, two_dof_vsa_boxddp 0.17 / 0.63, and 0 on B's everywhere.  Smallest shift sensitivity per output over the cases:
calc xnext 1.7, cost 3.6e-2, record 1.7; backward K 11, k 11, Qu 1.6, Vx 8.7, Vxx 34; forward xs_try 3.8, us_try 0.27,
cost_try 0.12; adjoint stiffness 6.4, motor inertia 7.7, x0 1.2, costate 8.7; plant sensitivity 1.3 (u_var); policy roll-out
0.21 (cost).  The planar VSA forward case keeps 46 of its 70 trajectories (ms.UNBOUNDED_FORWARD_CASES)."""
import numpy as np
import pytest

import _gpu_case as gc
import _model_switch as ms
import _plant_sens as ps
import _policy as pol
import _sensitivity as sens
from aslr_to_amd import _abi

SHIFT_SEEN = 1e-6


def _moved(label, pairs):
    """pairs: (output name, true reference, shifted reference): each must move by more than SHIFT_SEEN"""
    worst = {}
    for what, true, shift in pairs:
        worst[what] = gc.relerr(shift, true)
    print("%s: shift sensitivity %s" % (label, ", ".join("%s %.1e" % kv for kv in worst.items())))
    for what, v in worst.items():
        assert v > SHIFT_SEEN, "%s: %s moves by %g only under a node table that is one knot off" % (label, what, v)


def test_the_node_table_and_the_models_are_what_the_cases_say():
    sc, low = ms.problem("talos_arm_sea", 5, 7, ms.SEQ7)
    assert list(low.node_model) == [0, 1, 1, 2, 0, 2, 1, 3]
    assert list(ms.shifted(low).node_model) == [1, 0, 1, 1, 2, 0, 2, 3]
    m = [low.desc.models[i] for i in range(4)]
    assert m[1].dt == 0.5 * m[0].dt and m[2].dt == 2.0 * m[0].dt
    assert m[1].K[0] == 1.5 * m[0].K[0] and m[1].B[0] == 0.8 * m[0].B[0] and m[2].K[0] == m[0].K[0]
    assert m[0].u_ub[0] == 0.6 and m[2].u_ub[0] == 0.3 and not m[1].has_u_limits
    lb, ub = ms.bounds(low)
    assert np.isinf(ub[1]).all() and (ub[0] == 0.6).all() and (lb[3] == -0.3).all()
    sc, low = ms.problem("talos_arm_sea", 5, 7, ms.SEQ7, True)   # a table: K and B are the models' own, the box the table's
    m = [low.desc.models[i] for i in range(4)]
    assert m[1].K[0] == m[0].K[0] and m[1].B[0] == m[0].B[0] and m[1].dt == 0.5 * m[0].dt
    lb, ub = ms.bounds(low)
    assert (ub[0] == low.traj_params["u_ub"]).all() and (ub[3] == ub[0]).all() and np.isinf(ub[2]).all() and (ub[0] < 0.6).all()
    assert ms.SEQ_CYCLE(5) == (0, 1, 2, 0, 1)
    _, low = ms.problem("talos_arm_vsa", 5, 7, ms.SEQ7)
    m = low.desc.models
    assert (m[0].u_ub[0], m[0].u_lb[7], m[2].u_ub[0], m[2].u_lb[7], m[2].u_ub[13]) == (1.0, 1.0, 0.3, 2.0, 20.0)


@pytest.mark.parametrize("name,B,table", ms.CALC_CASES)
def test_calc_records_move_under_a_shifted_node_table(oracle, name, B, table):
    _, low = ms.problem(name, B, 7, ms.SEQ7, table)
    orc = ms.oracle_for(oracle, low)
    xs, us = gc.random_candidate(low, 1)     # the candidate of gc.check_calc_and_calc_diff
    true, shift = orc.calc_diff(low, xs, us), orc.calc_diff(ms.shifted(low), xs, us)
    _moved("%s table=%s" % (name, table), [("xnext", true[0], shift[0]), ("cost", true[1], shift[1]), ("record", true[2], shift[2])])


@pytest.mark.parametrize("feasible", [0, 1])
@pytest.mark.parametrize("name,B,solver", ms.BACKWARD_CASES)
def test_backward_cases_bind_the_box_per_model_and_see_a_shift(oracle, name, B, solver, feasible):
    """Boxed, feasible cases: the share of clamped (knot, control) pairs lies in (0.05, 0.95) on A's knots and on C's and is
    zero on B's; the backward pass of the SAME records with the node table one knot off moves K, k, Qu, Vx and Vxx.  The
    other cases (SolverDDP, SolverFDDP, SolverBoxDDP from an infeasible candidate) read the model through the records alone:
    the same shift moves nothing there, and the records are what moves -- they come from the calc sweep, whose shift
    sensitivity is asserted above, so here the whole chain is shifted."""
    c = ms.backward_case(oracle, name, B, solver, feasible)
    low, ref, sh = c["low"], c["ref"], ms.shifted(c["low"])
    assert not ref["fail"].any()
    label = "%s %s feasible=%d" % (name, solver, feasible)
    deriv = c["deriv"]
    if c["boxed"]:
        shares = [ms.clamped_share(low, ref["Qu"], mi) for mi in range(3)]
        print("%s: clamped share of Qu on the knots of A %.3f, B %.3f, C %.3f" % ((label,) + tuple(shares)))
        assert 0.05 < shares[0] < 0.95 and 0.05 < shares[2] < 0.95 and shares[1] == 0.0, shares
    else:
        same = oracle.backward_pass(sh, c["sp"], deriv, c["gaps"], c["us"], ms.XREG, feasible, kff0=c["k0"])
        for what in ("K", "k", "Qu", "Vx", "Vxx"):
            np.testing.assert_array_equal(same[what], ref[what], err_msg=what)
        deriv = oracle.calc_diff(sh, c["xs"], c["us"])[2]
    shift = oracle.backward_pass(sh, c["sp"], deriv, c["gaps"], c["us"], ms.XREG, feasible, kff0=c["k0"])
    assert not shift["fail"].any()
    _moved(label, [(what, ref[what], shift[what]) for what in ("K", "k", "Qu", "Vx", "Vxx")])


@pytest.mark.parametrize("name,B,T,solver,table", ms.FORWARD_CASES)
def test_forward_cases_roll_out_bind_the_clamp_and_see_a_shift(oracle, name, B, T, solver, table):
    c = ms.forward_case(oracle, name, B, T, solver, table)
    low = c["low"]
    label = "%s %s T=%d table=%s" % (name, solver, T, table)
    worst = 0.0
    hit = {0: set(), 2: set()}
    keep = c["keep"]
    floor = ms.UNBOUNDED_FORWARD_CASES.get((name, B, T, solver, table))
    print("%s: %d of %d trajectories stay within |x| = %g at every step length" % (label, keep.sum(), keep.size, ms.X_BOUND))
    if floor is None:
        assert keep.all()
    else:   # (why: ms.UNBOUNDED_FORWARD_CASES) enough of them, and some in the partial last wave
        assert floor < keep.mean() < 1.0 and keep[64:].any() and not keep[64:].all()
    for a, (xs_try, us_try, cost_try, fail) in enumerate(c["ref"]):
        xs_try, us_try = xs_try[:, keep], us_try[:, keep]
        assert not fail[keep].any(), "%s: a rollout fails at alpha index %d" % (label, a)
        worst = max(worst, np.abs(xs_try).max())
        if c["boxed"]:
            lb, ub = (v[:, keep] for v in ms.bounds(low))
            assert (us_try >= lb).all() and (us_try <= ub).all()
            onb = (us_try == lb) | (us_try == ub)
            assert not onb[ms.knots_of(low, 1)].any()
            free = us_try[ms.knots_of(low, 1)]
            assert ((free < lb[0]) | (free > ub[0])).any()     # on B's knots controls go where A's box would have clipped them
            for mi in (0, 2):
                hit[mi] |= set(np.unique(us_try[ms.knots_of(low, mi)][onb[ms.knots_of(low, mi)]]).tolist())
    print("%s: max |xs_try| %.2e" % (label, worst))
    assert worst < ms.X_BOUND
    if c["boxed"]:
        print("%s: controls on a bound: %d distinct values on A's knots, %d on C's" % (label, len(hit[0]), len(hit[2])))
        assert hit[0] and hit[2] and hit[0] != hit[2]
    true, shift = c["ref"][0], ms.forward_ref(ms.oracle_for(oracle, low), c, ms.shifted(low), 1.0)
    assert not shift[3][keep].any()
    _moved(label, [("xs_try", true[0][:, keep], shift[0][:, keep]), ("us_try", true[1][:, keep], shift[1][:, keep]),
                   ("cost_try", true[2][keep], shift[2][keep])])


@pytest.mark.parametrize("name,B,table", ms.EXT_CASES)
def test_extension_references_move_under_a_shifted_node_table(oracle, name, B, table):
    """the adjoint sweep, the plant sensitivity and (2 joints) the clamped policy roll-out, each reference against the one of
    the shifted node table, with the oracle's own gains"""
    c = ms.ext_case(oracle, name, B, table)
    low, sh = c["low"], ms.shifted(c["low"])
    label = "%s table=%s" % (name, table)
    xs, us = c["xs"], c["us"]
    true, shift = sens.expected(oracle, low, xs, us), sens.expected(oracle, sh, xs, us)
    _moved(label + " adjoint", [(k, true[k], shift[k]) for k in ("stiffness", "motor_inertia", "x0", "costate")])
    K = pol.oracle_gains(oracle, low, c["sp"], xs, us)
    vk, vb = ps.variances(low, 37)
    true, shift = ps.expected(oracle, low, xs, us, K, vk, vb), ps.expected(oracle, sh, xs, us, K, vk, vb)
    _moved(label + " plant sensitivity", [(k, true[k], shift[k]) for k in ps.OUTPUTS])
    if low.nj == 2:
        pert = ms.policy_perturbations(low, ms.POLICY_S)
        true = pol.rollout(oracle, low, xs, us, K, ms.POLICY_S, clamp=True, **pert)
        shift = pol.rollout(oracle, sh, xs, us, K, ms.POLICY_S, clamp=True, **pert)
        assert (true["failed_knot"] == -1).all()
        print("%s: samples whose controls the clamp moved: %d of %d" % (label, true["bound"].sum(), true["bound"].size))
        assert true["bound"].any() and not true["bound"].all()
        _moved(label + " policy roll-out", [(k, true[k], shift[k]) for k in pol.OUTPUTS])


@pytest.mark.parametrize("name,solver", ms.SOLVE_CASES)
def test_oracle_is_stable_on_the_full_solve_cases(oracle, name, solver):
    """the check of tests/test_ref_path_host.py: scaling x0 by (1 + 1e-14) moves no iteration count or status word and the
    iterates by less than the 1e-6 (relative to their size) the GPU is held to; the solution rides a bound on some A knot and
    some C knot and stays inside each knot's own box"""
    c = ms.solve_case(oracle, name, solver)
    low, ref = c["low"], c["ref"]
    per = ms.perturbed_solve(oracle, c, 1e-14)
    it, st = ref["traj_i"][_abi.TI_ITER], ref["traj_i"][_abi.TI_STATUS]
    scale = max(1.0, np.abs(ref["xs"]).max(), np.abs(ref["us"]).max())
    dx, du = np.abs(per["xs"] - ref["xs"]).max(), np.abs(per["us"] - ref["us"]).max()
    dc = (np.abs(per["traj_f"][_abi.TF_COST] - ref["traj_f"][_abi.TF_COST]) / np.maximum(1.0, np.abs(ref["traj_f"][_abi.TF_COST]))).max()
    print("%s %s: iterations %s, status %s, converged %d of %d, scale %.2e; under x0 (1 + 1e-14): counts changed %d, dx %.1e du %.1e dcost %.1e"
          % (name, solver, it, st, ((st & _abi.ST_CONVERGED) != 0).sum(), st.size, scale,
             int((per["traj_i"][_abi.TI_ITER] != it).sum()), dx, du, dc))
    np.testing.assert_array_equal(per["traj_i"][_abi.TI_ITER], it)
    np.testing.assert_array_equal(per["traj_i"][_abi.TI_STATUS], st)
    assert dx < 1e-6 * scale and du < 1e-6 * scale and dc < 1e-4
    lb, ub = ms.bounds(low)
    U = ref["us"]
    assert (U >= lb).all() and (U <= ub).all()
    onb = ms.on_bound(low, U)
    assert onb[ms.knots_of(low, 0)].any() and onb[ms.knots_of(low, 2)].any()
