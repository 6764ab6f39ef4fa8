"""Closed-loop policy roll-outs (aslr_policy_rollout, include/aslr_to_amd_policy.h) on a CPU: the contract of the extension
header, the reference of tests/_policy.py pinned on the oracle alone, and the conditioning of the inputs the GPU cases use
(tests/test_gpu_policy.py)."""
import ctypes as C

import numpy as np
import pytest

import _gpu_case as gc
import _policy as pol
from aslr_to_amd import _abi, scenarios


def test_a_null_handle_is_refused_by_name():
    lib = _abi.load_library()
    assert lib.aslr_workspace_bytes(None) < 0     # some other message is in the buffer first
    buf = C.cast((C.c_double * 64)(), C.c_void_p)   # stands where a device pointer goes; never dereferenced
    assert lib.aslr_policy_rollout(None, 4, None, None, None, None, 0, buf, None, None, None, None, None) == _abi.E_INVALID
    msg = lib.aslr_last_error().decode()
    assert msg.startswith("aslr_policy_rollout:") and "handle" in msg, msg


@pytest.mark.parametrize("name, solver", [("two_dof_sea", "SolverDDP"), ("two_dof_vsa_boxddp", "SolverBoxDDP")])
def test_the_reference_is_the_oracles_forward_pass_where_the_two_overlap(oracle, name, solver):
    """No disturbance, plant = model, k = 0 and dx0 folded into the problem's x0: the reference must be oracle.forward_pass
    at alpha = 1 (clamp on under SolverBoxDDP), states, controls and costs within 1e-13 relative.  B = 3, T = 6, the mild
    gains of gc.forward_inputs."""
    B, T = 3, 6
    sc = scenarios.SCENARIOS[name](B=B, T=T, seed=4)
    dx0 = np.random.default_rng(8).uniform(-1e-2, 1e-2, (B, 8))
    moved = dict(sc, x0=np.asarray(sc["x0"]) + dx0)
    low, low_moved = scenarios.lower(sc), scenarios.lower(moved)
    sp = scenarios.solver_params(sc, solver=solver)
    xs, us, K, _, _ = gc.forward_inputs(oracle, low, sp, 5, False)
    xs_try, us_try, cost_try, fail = oracle.forward_pass(low_moved, sp, 1.0, xs, us, K, np.zeros_like(us))
    assert not fail.any()
    got = pol.rollout(oracle, low, xs, us, K, 1, dx0=dx0[:, None, :], clamp=solver == "SolverBoxDDP")
    assert (got["failed_knot"] == -1).all()
    assert np.abs(xs_try - xs).max() > 1e-3     # a closed loop that moved
    for what, a, b in (("xs", got["xs"][:, 0].transpose(1, 0, 2), xs_try), ("us", got["us"][:, 0].transpose(1, 0, 2), us_try),
                       ("cost", got["cost"][:, 0], cost_try)):
        err = pol.relerr(a, b)
        print("%s %s: %.2e" % (name, what, err))
        assert err < 1e-13, (what, err)


@pytest.mark.parametrize("key", sorted(pol.CASES))
def test_the_gpu_cases_are_well_conditioned(oracle, key):
    """x0 and K moved by 1e-13 relative (seeded signs): every output of the reference must move by less than 1e-11 in the
    measure of the GPU tests, max |a - b| / (1 + |b|), so that 1e-9 there is a statement about the kernel.  A condition on
    the choice of inputs.  What was chosen: T and the perturbation ranges stay at the issue's values (T <= 5, +-30 %, 1e-2,
    1e-3); the seeded candidate is seeded controls with their own open-loop roll-out as xs.  With gc.random_candidate's
    unrelated random xs the loop starts at |x0 - xs_0| ~ 1 under the stiff gains of one backward sweep, and the movement
    was 1.0e-11 .. 5.7e-11 (six of eight cases over the bound); with the roll-out it is 0 .. 6.5e-12 (worst: vsa_box)."""
    c = pol.case(oracle, key)
    low, xs, us, S = c["low"], c["xs"], c["us"], c["S"]
    K = pol.oracle_gains(oracle, low, c["sp"], xs, us)
    base = pol.rollout(oracle, low, xs, us, K, S, clamp=c["clamp"], **c["pert"])
    assert (base["failed_knot"] == -1).all() and np.isfinite(base["cost"]).all()
    rng = np.random.default_rng(23)
    K2 = K * (1.0 + 1e-13 * rng.choice([-1.0, 1.0], K.shape))
    x0 = np.array(low.x0)
    try:
        low.x0[:] = x0 * (1.0 + 1e-13 * rng.choice([-1.0, 1.0], x0.shape))
        moved = pol.rollout(oracle, low, xs, us, K2, S, clamp=c["clamp"], **c["pert"])
    finally:
        low.x0[:] = x0
    worst = max(pol.relerr(moved[k], base[k]) for k in pol.OUTPUTS)
    print("%s: worst movement %.2e" % (key, worst))
    assert worst < 1e-11, worst
    if c["clamp"]:
        print("%s: the box binds on %d of %d samples" % (key, base["bound"].sum(), base["bound"].size))
        assert base["bound"].any() and not base["bound"].all()
