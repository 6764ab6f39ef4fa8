"""The comparison layer of tests/_gpu_case.py on a CPU: a shared assertion that cannot fail would disarm every GPU test built
on it.  The "GPU" side is a copy of the oracle's own results (two_dof_vsa_boxddp, B = 3, T = 4): the exact copy must pass,
one entry off by 1e-6 relative -- far outside every tolerance the GPU tests use, 1e-8 at the widest -- must raise with the
name of what differs."""
import numpy as np
import pytest

import _gpu_case as gc
from aslr_to_amd import _abi, scenarios

SEED = 3


@pytest.fixture(scope="module")
def case(oracle):
    """Inputs and the oracle's results, computed once and left unchanged (the tests perturb copies)."""
    sc = scenarios.two_dof_vsa_boxddp(B=3, T=4)
    low = scenarios.lower(sc)
    sp = scenarios.solver_params(sc)
    xs, us, K, k, gaps, ref_b = gc.forward_inputs(oracle, low, sp, SEED, False, full=True)
    forward = [oracle.forward_pass(low, sp, 0.5 ** a, xs, us, K, k) for a in range(_abi.NALPHA)]
    assert not ref_b["fail"].any() and all((f[3] == 0).all() for f in forward)
    return dict(records=oracle.calc_diff(low, xs, us), backward=ref_b, forward=forward)


def _off(a, index=None):
    """a copy of `a` with one entry (the largest, or the one at `index`) moved by 1e-6 relative"""
    a = np.array(a, dtype=float)
    index = np.unravel_index(np.abs(a).argmax(), a.shape) if index is None else index
    a[index] += 1e-6 * (1.0 + abs(a[index]))
    return a


def _backward_copy(ref):
    out = {name: np.array(ref[name]) for name in gc.BACKWARD_FIELDS}
    out["status"] = np.zeros(3, dtype=np.int32)
    return out


def test_backward_comparison_passes_on_an_exact_copy(case):
    gc.assert_backward_matches(_backward_copy(case["backward"]), case["backward"], 1e-8)


@pytest.mark.parametrize("field", gc.BACKWARD_FIELDS)
def test_backward_comparison_names_the_field_that_differs(case, field):
    out = _backward_copy(case["backward"])
    out[field] = _off(out[field])
    with pytest.raises(AssertionError, match=r"^%s mismatch" % field):
        gc.assert_backward_matches(out, case["backward"], 1e-8)
    gc.assert_backward_matches(out, case["backward"], 1e-8, fields=[f for f in gc.BACKWARD_FIELDS if f != field])


def test_backward_comparison_refuses_a_backward_error_on_either_side(case):
    out = _backward_copy(case["backward"])
    out["status"][1] = _abi.ST_BACKWARD_ERR | _abi.ST_CONVERGED
    with pytest.raises(AssertionError, match="ST_BACKWARD_ERR"):
        gc.assert_backward_matches(out, case["backward"], 1e-8)
    failed = dict(case["backward"], fail=np.array([0, 0, 1]))
    with pytest.raises(AssertionError, match="oracle"):
        gc.assert_backward_matches(_backward_copy(case["backward"]), failed, 1e-8)


def _forward_copy(forward):
    return (np.stack([f[0] for f in forward]), np.stack([f[1] for f in forward]), np.stack([f[2] for f in forward]))


def test_forward_comparison_passes_on_an_exact_copy_and_returns_the_masks(case):
    XT, UT, costs = _forward_copy(case["forward"])
    oks, refs = gc.assert_forward_matches(XT, UT, costs, case["forward"])
    assert len(oks) == _abi.NALPHA and all(ok.all() for ok in oks)
    assert all(r is f for r, f in zip(refs, case["forward"]))
    # the same through a callable of the step length, as the tests give it
    seen = []
    gc.assert_forward_matches(XT, UT, costs, lambda alpha: (seen.append(alpha), case["forward"][len(seen) - 1])[1])
    assert seen == [0.5 ** a for a in range(_abi.NALPHA)]


@pytest.mark.parametrize("a", [0, _abi.NALPHA - 1])
@pytest.mark.parametrize("which", ["xs_try", "us_try", "cost_try"])
def test_forward_comparison_names_the_output_and_step_length_that_differ(case, which, a):
    got = list(_forward_copy(case["forward"]))
    i = ["xs_try", "us_try", "cost_try"].index(which)
    got[i][a] = _off(got[i][a])
    with pytest.raises(AssertionError, match=r"^%s\[%d\] mismatch" % (which, a)):
        gc.assert_forward_matches(*got, case["forward"])


def test_forward_comparison_with_a_trajectory_the_oracle_fails_on(case):
    """fail set by hand on trajectory 1 at every step length: its candidates are not compared, its cost must be NaN."""
    XT, UT, costs = _forward_copy(case["forward"])
    failing = [f[:3] + (np.array([0, 1, 0]),) for f in case["forward"]]
    with pytest.raises(AssertionError, match="finite trial cost"):
        gc.assert_forward_matches(XT, UT, costs, failing)
    costs[:, 1] = np.nan
    XT[:, :, 1], UT[:, :, 1] = np.nan, 7.0        # (whatever a failed rollout left behind)
    oks, _ = gc.assert_forward_matches(XT, UT, costs, failing)
    assert all(ok.tolist() == [True, False, True] for ok in oks)
    # ... one entry off on a trajectory that succeeded still raises
    XT[2] = _off(XT[2], (3, 2, 0))
    with pytest.raises(AssertionError, match=r"^xs_try\[2\] mismatch"):
        gc.assert_forward_matches(XT, UT, costs, failing)
    # ... as does a NaN cost where the oracle succeeded, and a reference that fails everywhere
    costs[4, 0] = np.nan
    with pytest.raises(AssertionError, match=r"^cost_try\[4\] mismatch"):
        gc.assert_forward_matches(_forward_copy(case["forward"])[0], UT, costs, failing)
    with pytest.raises(AssertionError, match="fails on every trajectory"):
        gc.assert_forward_matches(XT, UT, costs, [f[:3] + (np.ones(3, dtype=int),) for f in case["forward"]])


def test_records_comparison(case):
    xnext, cost, deriv = (np.array(v) for v in case["records"])
    gc.assert_records_match(xnext, cost, deriv, ref=case["records"])
    gc.assert_records_match(xnext, cost, None, ref=case["records"])
    for what, args in (("xnext", (_off(xnext), cost, deriv)), ("cost", (xnext, _off(cost), deriv)),
                       ("DERIV record", (xnext, cost, _off(deriv)))):
        with pytest.raises(AssertionError, match="^%s mismatch" % what):
            gc.assert_records_match(*args, ref=case["records"])
    # the two tolerances are apart: 1e-10 relative passes on the record and fails on the state
    small = lambda a: a + 1e-10 * (1.0 + np.abs(a))
    gc.assert_records_match(xnext, cost, small(deriv), ref=case["records"])
    with pytest.raises(AssertionError, match="^xnext mismatch"):
        gc.assert_records_match(small(xnext), cost, deriv, ref=case["records"])
    gc.assert_records_match(small(xnext), cost, deriv, ref=case["records"], tol_state=1e-9)
    with pytest.raises(AssertionError, match="^cost mismatch"):
        gc.assert_records_match(xnext, np.where(np.arange(cost.size).reshape(cost.shape) == 5, np.nan, cost), deriv,
                                ref=case["records"])


def test_relerr_and_owned_copies():
    assert gc.relerr(np.zeros((0, 3)), np.zeros((0, 3))) == 0.0
    assert gc.relerr([1.0, 3.0], [1.0, 1.0]) == 1.0
    import torch
    for src in (np.arange(6.0).reshape(2, 3), torch.arange(6.0, dtype=torch.float64).reshape(2, 3)):
        got = gc.to_np(src)
        assert isinstance(got, np.ndarray) and got.flags.owndata
        assert not np.shares_memory(got, src if isinstance(src, np.ndarray) else src.numpy())
        np.testing.assert_array_equal(got, np.arange(6.0).reshape(2, 3))
        got[0, 0] = -1.0
        assert float(src[0, 0]) == 0.0
    view = np.arange(12.0).reshape(3, 4).T           # a permuted view comes back as an array of its own too
    assert not np.shares_memory(gc.to_np(view), view)


def _mixed(case):
    """the oracle's result with trajectory 1 declared failed (whatever its rows hold), and a "GPU" copy that says the same"""
    ref = dict(case["backward"], fail=np.array([0, 1, 0]))
    out = _backward_copy(case["backward"])
    out["status"][1] = _abi.ST_BACKWARD_ERR
    for name in gc.BACKWARD_FIELDS:        # (a failed sweep's leftovers are not compared)
        if out[name].ndim == 1:
            out[name][1] = np.nan
        else:
            out[name][:, 1] = -7.0
    return out, ref


def test_mixed_backward_comparison_passes_on_a_copy_and_ignores_the_failed_trajectory(case):
    out, ref = _mixed(case)
    ok = gc.assert_backward_matches_where_ok(out, ref, 1e-8)
    assert ok.tolist() == [True, False, True]


@pytest.mark.parametrize("field", gc.BACKWARD_FIELDS)
@pytest.mark.parametrize("b", [0, 2])
def test_mixed_backward_comparison_fails_on_one_wrong_entry_of_a_surviving_trajectory(case, field, b):
    out, ref = _mixed(case)
    index = (b,) if out[field].ndim == 1 else (out[field].shape[0] - 1, b) + (0,) * (out[field].ndim - 2)
    out[field] = _off(out[field], index)
    with pytest.raises(AssertionError, match=r"^%s mismatch" % field):
        gc.assert_backward_matches_where_ok(out, ref, 1e-8)
    out[field][index] = np.nan             # (what a sentinel left behind looks like)
    with pytest.raises(AssertionError, match=r"^%s mismatch" % field):
        gc.assert_backward_matches_where_ok(out, ref, 1e-8)


def test_mixed_backward_comparison_holds_the_status_bits_to_the_oracles_fail_mask(case):
    out, ref = _mixed(case)
    out["status"][1] = _abi.ST_CONVERGED                       # missing on the failed one
    with pytest.raises(AssertionError, match=r"ST_BACKWARD_ERR is missing on trajectories \[1\]"):
        gc.assert_backward_matches_where_ok(out, ref, 1e-8)
    out, ref = _mixed(case)
    out["status"][2] = _abi.ST_BACKWARD_ERR                    # present on a surviving one
    with pytest.raises(AssertionError, match=r"ST_BACKWARD_ERR is set on trajectories \[2\]"):
        gc.assert_backward_matches_where_ok(out, ref, 1e-8)


def test_mixed_backward_comparison_refuses_a_reference_that_is_not_mixed(case):
    out, ref = _mixed(case)
    out["status"][:] = _abi.ST_BACKWARD_ERR
    with pytest.raises(AssertionError, match="fails on every trajectory"):
        gc.assert_backward_matches_where_ok(out, dict(ref, fail=np.ones(3, dtype=np.int32)), 1e-8)
    with pytest.raises(AssertionError, match="fails on no trajectory"):
        gc.assert_backward_matches_where_ok(_backward_copy(case["backward"]), case["backward"], 1e-8)


def test_wrote_tells_a_prefill_from_any_other_bits():
    import _mixed_waves as mw
    a = np.full((2, 3), mw.SENTINEL)
    assert np.isnan(mw.SENTINEL) and not gc.wrote(a, mw.SENTINEL).any()
    a[0, 1], a[1, 2] = np.nan, 0.0                             # another NaN counts as written
    assert gc.wrote(a, mw.SENTINEL).tolist() == [[False, True, False], [False, False, True]]
