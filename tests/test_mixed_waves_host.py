"""The inputs of tests/test_gpu_mixed_waves.py on the CPU oracle alone (tests/_mixed_waves.py makes them): the kernel-level
records fail on exactly the intended trajectories, far from the edge, in every pattern for every wave width, at the first and
at the last knot of the sweep; the solve-level cases really part inside a wave and are stable under a perturbation of the
reference's own size."""
import numpy as np
import pytest

import _mixed_waves as mw
from aslr_to_amd import _abi


def test_the_masks_hold_every_pattern_for_every_wave_width():
    for tpw in mw.TPWS:
        found = set().union(*(mw.patterns(m, tpw) for m in mw.MASKS.values()))
        assert found == mw.PATTERNS, (tpw, mw.PATTERNS - found)
    # the detector itself: one group of four, each pattern alone
    assert mw.patterns([1, 0, 0, 0], 4) == {"only the first"}
    assert mw.patterns([0, 0, 0, 1], 4) == {"only the last"}
    assert mw.patterns([1, 1, 0, 1], 4) == {"all but one"}
    assert mw.patterns([0, 1, 0, 1], 4) == {"alternating"}
    assert mw.patterns([0, 0, 0, 0], 4) == set() and mw.patterns([1, 1, 1, 1], 4) == set()
    assert mw.patterns([0, 1, 1, 0, 1, 0], 4) == {"next to the partial last wave"}
    assert mw.patterns([1, 1, 1, 1, 1, 1], 4) == set()
    for m in mw.MASKS.values():
        tb = mw.fail_knots(m)
        assert ((tb >= 0) == m).all() and (tb == 0).any() and (tb == mw.T - 1).any()
    # x_reg and the feasibility flags are mixed inside every full group of 4 and of 8, and inside two pairs of every three
    for v in (mw.xregs(), mw.feasible_flags("a"), mw.feasible_flags("b")):
        for t in mw.TPWS:
            mixed = [len(set(v[g])) == 2 for g in mw.groups(t) if g.stop - g.start == t]
            assert all(mixed) if t > 2 else sum(mixed) == 6, (t, mixed)


@pytest.mark.parametrize("scen,solver", mw.KERNEL_CASES)
@pytest.mark.parametrize("flags", ["a", "b"])
@pytest.mark.parametrize("mask_name", sorted(mw.MASKS))
def test_kernel_level_records_fail_where_intended_and_far_from_the_edge(oracle, scen, solver, flags, mask_name):
    c = mw.kernel_case(oracle, scen, solver, flags, mask_name)
    fail = c["ref"]["fail"] != 0
    np.testing.assert_array_equal(fail, mw.MASKS[mask_name])
    assert not c["clean"]["fail"].any()
    for factor in (0.5, 2.0):     # no trajectory near the edge
        r = oracle.backward_pass(c["low"], c["sp"], c["deriv"], c["gaps"], c["us"], factor * c["xreg"], c["feasible"], kff0=c["k0"])
        np.testing.assert_array_equal(r["fail"] != 0, fail)
    # the survivors' records are untouched, so the oracle computes on them what it computes without any failure ...
    for name in ("K", "k", "Qu", "Vx", "Vxx"):
        np.testing.assert_array_equal(c["ref"][name][:, ~fail], c["clean"][name][:, ~fail], err_msg=name)
    # ... and a failing trajectory fails AT its knot t_b: the rows above are those of the untouched records
    for b in np.nonzero(fail)[0]:
        tb = c["tb"][b]
        for name in ("K", "k", "Qu"):
            np.testing.assert_array_equal(c["ref"][name][tb + 1:, b], c["clean"][name][tb + 1:, b], err_msg=name)
        for name in ("Vx", "Vxx"):
            np.testing.assert_array_equal(c["ref"][name][tb + 1:, b], c["clean"][name][tb + 1:, b], err_msg=name)
    if solver == "SolverBoxDDP":  # the box is active on the feasible survivors
        feas = (c["feasible"] != 0) & ~fail
        clamped = (c["ref"]["Qu"][:, feas] == 0.0).mean()
        assert 0.05 < clamped < 0.95, clamped


@pytest.mark.parametrize("vsa", [False, True])
def test_seven_joint_records_fail_on_the_middle_trajectory_alone(oracle, vsa):
    c = mw.arm_case(oracle, vsa)
    assert (c["ref"]["fail"] != 0).tolist() == [False, True, False] and not c["clean"]["fail"].any()
    for factor in (0.5, 2.0):
        r = oracle.backward_pass(c["low"], c["sp"], c["deriv"], c["gaps"], c["us"], factor * c["xreg"], c["feasible"], kff0=c["k0"])
        assert (r["fail"] != 0).tolist() == [False, True, False]


@pytest.mark.parametrize("name", sorted(mw.SOLVE_CASES))
def test_solve_cases_part_inside_a_wave_and_are_stable(oracle, name):
    ref = mw.solve_ref(oracle, name)
    st, it = ref["traj_i"][_abi.TI_STATUS], ref["traj_i"][_abi.TI_ITER]
    assert mw.SOLVE_CASES[name][4] <= 6
    assert ((st & _abi.ST_BACKWARD_ERR) != 0).all()              # every trajectory took the retry path
    for tpw in mw.TPWS:
        parts = mw.xreg_parts_in_groups(ref["log"], tpw)
        print("%s: x_reg parts inside a group of %d in iterations %s" % (name, tpw, parts))
        assert parts, tpw
    if name == "vsa_boxddp":   # a trajectory at the ceiling beside one that goes on (see SOLVE_CASES for the SEA cases)
        for tpw in mw.TPWS:
            pairs = mw.reg_max_beside_a_running_neighbour(ref, tpw)
            print("%s: (stopped at reg_max, running neighbour, iterations) in groups of %d: %s" % (name, tpw, pairs))
            assert pairs, tpw
        assert (12, 13, 2) in mw.reg_max_beside_a_running_neighbour(ref, 2)   # the one test (d) follows
    # a 1e-14 relative perturbation of x0 moves no iteration count, no status word and no logged x_reg
    per = mw.solve_ref(oracle, name, 1.0 + 1e-14)
    np.testing.assert_array_equal(per["traj_i"][_abi.TI_ITER], it)
    np.testing.assert_array_equal(per["traj_i"][_abi.TI_STATUS], st)
    np.testing.assert_array_equal(per["log"][:, _abi.LOG_XREG], ref["log"][:, _abi.LOG_XREG])
    mag = np.maximum(np.abs(ref["xs"]).max(axis=(0, 2)), np.abs(ref["us"]).max(axis=(0, 2)))
    assert (mag < 1e6).sum() >= 10                             # enough tame trajectories to compare values on
