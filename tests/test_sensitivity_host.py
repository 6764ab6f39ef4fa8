"""Cost sensitivities (aslr_cost_sensitivity, include/aslr_to_amd_sens.h) on a CPU: the formula the kernel implements against
finite differences of the oracle's own rollouts and solves, and the contract of the extension header.  The expected values
come from tests/_sensitivity.py, which uses the definition of the gradients and none of the kernel's closed-form identities.

Finite-difference error is not rounding error and has no a-priori bound, so the tolerances of the two finite-difference
tests were fixed by the procedure of their docstrings: the disagreement measured over a few relative steps on the oracle
alone, the step where it is smallest, ten times that value.  Disagreement: max |a - b| / (1 + |b|) (_sensitivity.relerr)."""
import ctypes as C

import numpy as np
import pytest

import _sensitivity as sens
import _traj_oracle
from aslr_to_amd import _abi, scenarios


# scenario -> (relative step, disagreement measured at it); the bound is ten times the measured value
ROLLOUT_FD = {"two_dof_sea": (1e-5, 8.2e-8), "talos_arm_sea": (1e-4, 8.2e-8)}


@pytest.mark.parametrize("name", sorted(ROLLOUT_FD))
def test_the_adjoint_gradients_match_finite_differences_of_the_rollout_cost(oracle, name):
    """B = 3, T = 6, a seeded per-trajectory table; the candidate is the oracle's open-loop rollout of random controls (zero
    gaps: the adjoint gradient is exact there).  dJ/dK_j, dJ/dB_j and dJ/dx0_i from the oracle's records against central
    differences of the rollout's total cost.

    Measured (worst of the three gradients, per relative step 1e-4 / 1e-5 / 1e-6 / 1e-7):
      two_dof_sea    5.1e-7 / 8.2e-8 / 1.5e-7 / 1.2e-6   -> step 1e-5, bound 8.2e-7
      talos_arm_sea  8.1e-8 / 5.5e-7 / 5.5e-6 / 8.0e-5   -> step 1e-4, bound 8.2e-7
    (gradient magnitudes: up to 1.2e3 for two_dof_sea, 4.9e4 for talos_arm_sea)."""
    rel, measured = ROLLOUT_FD[name]
    sc = scenarios.with_traj_params(scenarios.SCENARIOS[name](B=3, T=6, seed=4), seed=5)
    low = scenarios.lower(sc)
    us = np.random.default_rng(11).uniform(-1.0, 1.0, (low.T, low.B, low.nu))
    xs = sens.rollout(oracle, low, us)
    want = sens.expected(oracle, low, xs, us)
    fd = sens.fd_rollout(oracle, low, us, rel)
    for k in ("stiffness", "motor_inertia", "x0"):
        err = sens.relerr(want[k], fd[k])
        print("%s d%s: disagreement %.2e at step %.0e (bound %.1e)" % (name, k, err, rel, 10 * measured))
        assert np.abs(fd[k]).max() > 1.0      # a gradient worth the name
        assert err < 10 * measured, (k, err)


def test_at_an_optimum_the_adjoint_gradient_is_the_gradient_of_the_optimal_cost(oracle):
    """The oracle's converged SolverDDP solves (all 4 must converge); dJ/dK_j and dJ/dB_j at the solution against central
    differences of the CONVERGED cost of re-solved, perturbed problems (envelope theorem).

    The solves run to th_stop = 1e-16, not the script's 1e-7: away from exact stationarity the adjoint gradient is off by a
    term of first order in Lu + Fu^T lambda, whatever the step.  Measured on the oracle, worst of the two gradients:
      th_stop 1e-7 (14-27 iterations): 5.7e-2 at every step 1e-2 .. 1e-7;  1e-10: 2.4e-3;  1e-13: 7.3e-5;
      th_stop 1e-16 (29-56 iterations): 5.1e-5 / 2.2e-6 / 2.2e-6 / 2.2e-6 / 2.2e-6 at steps 1e-2 / 1e-3 / 1e-4 / 1e-5 / 1e-6
    -> step 1e-3, bound 2.2e-5 (gradient magnitudes 0.56 in K, 72 in B)."""
    sc, sp = sens.optimum_case()
    low = scenarios.lower(sc)
    ref = _traj_oracle.solve(oracle, low, sp)
    assert ((ref["traj_i"][_abi.TI_STATUS] & _abi.ST_CONVERGED) != 0).all()
    want = sens.expected(oracle, low, ref["xs"], ref["us"])
    fd = sens.optimum_fd(oracle)
    for k in ("stiffness", "motor_inertia"):
        err = sens.relerr(want[k], fd[k])
        print("d%s: disagreement %.2e at step %.0e (bound %.1e)" % (k, err, sens.OPT_FD[0], 10 * sens.OPT_FD[1]))
        assert err < 10 * sens.OPT_FD[1], (k, err)


def test_a_null_handle_is_refused_by_name():
    lib = _abi.load_library()
    assert lib.aslr_workspace_bytes(None) < 0     # some other message is in the buffer first
    buf = C.cast((C.c_double * 64)(), C.c_void_p)   # stands where a device pointer goes; never dereferenced
    assert lib.aslr_cost_sensitivity(None, buf, buf, buf, buf, None) == _abi.E_INVALID
    msg = lib.aslr_last_error().decode()
    assert msg.startswith("aslr_cost_sensitivity:") and "handle" in msg, msg
