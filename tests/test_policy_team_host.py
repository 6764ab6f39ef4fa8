"""Closed-loop policy roll-outs for every model size (aslr_policy_rollout_all, include/aslr_to_amd_policy_all.h) on a CPU: the
contract of the extension header, and the conditioning of the 7-joint cases the GPU tests use (tests/_policy_team.py,
tests/test_gpu_policy_team.py) on the oracle alone, with the reference of tests/_policy.py as it stands."""
import ctypes as C

import numpy as np
import pytest

import _policy as pol
import _policy_team as pt
from aslr_to_amd import _abi


def test_a_null_handle_is_refused_by_name():
    lib = _abi.load_library()
    assert lib.aslr_workspace_bytes(None) < 0     # some other message is in the buffer first
    buf = C.cast((C.c_double * 64)(), C.c_void_p)   # stands where a device pointer goes; never dereferenced
    assert lib.aslr_policy_rollout_all(None, 4, None, None, None, None, 0, buf, None, None, None, None, None) == _abi.E_INVALID
    msg = lib.aslr_last_error().decode()
    assert msg.startswith("aslr_policy_rollout_all:") and "handle" in msg, msg


@pytest.mark.parametrize("key", sorted(pt.CASES))
def test_the_gpu_cases_are_well_conditioned(oracle, key):
    """On the oracle alone: no sample fails; the closed loops leave the candidate by more than 1e-3; the gains moved by
    1e-13 relative (seeded signs) move every output of the reference by less than 1e-10 in the measure of the GPU tests,
    max |a - b| / (1 + |b|) -- an amplification below 1e3, which is what makes 1e-9 there a statement about the kernel and
    not about the inputs.  arm_vsa_box: the narrowed box binds on some samples and not on all, and the clamped controls
    differ from the free ones by more than 1e-3."""
    c = pt.case(oracle, key)
    low, xs, us, S = c["low"], c["xs"], c["us"], c["S"]
    K = pol.oracle_gains(oracle, low, c["sp"], xs, us)
    base = pol.rollout(oracle, low, xs, us, K, S, clamp=c["clamp"], **c["pert"])
    assert (base["failed_knot"] == -1).all() and np.isfinite(base["cost"]).all()
    moved_by = np.abs(base["xs"] - xs.transpose(1, 0, 2)[:, None]).max()
    print("%s: the loops leave the candidate by %.2e" % (key, moved_by))
    assert moved_by > 1e-3
    rng = np.random.default_rng(23)
    K2 = K * (1.0 + 1e-13 * rng.choice([-1.0, 1.0], K.shape))
    moved = pol.rollout(oracle, low, xs, us, K2, S, clamp=c["clamp"], **c["pert"])
    worst = max(pol.relerr(moved[k], base[k]) for k in pol.OUTPUTS)
    print("%s: worst movement %.2e" % (key, worst))
    assert worst < 1e-10, worst
    if c["clamp"]:
        print("%s: the box binds on %d of %d samples" % (key, base["bound"].sum(), base["bound"].size))
        assert base["bound"].any() and not base["bound"].all()
        free = pol.rollout(oracle, low, xs, us, K, S, clamp=False, **c["pert"])
        diff = pol.relerr(free["us"], base["us"])
        print("%s: clamped against free controls %.2e" % (key, diff))
        assert diff > 1e-3
