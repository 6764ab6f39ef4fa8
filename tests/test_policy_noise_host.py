"""Monte-Carlo policy roll-outs that draw their noise on the device (aslr_policy_rollout_noise,
include/aslr_to_amd_policy_noise.h) on a CPU: the numpy generator of tests/_policy_noise.py against the known answers of the
definition, the contract of the extension header, and the conditioning of the cases the GPU tests use
(tests/test_gpu_policy_noise.py) on the oracle alone.

Sigmas: tests/_policy_noise.SIGMAS as the issue gives them (3e-4, 3e-3, 0.05 relative); the oracle diverges for no case,
so none was lowered and no sample is skipped."""
import ctypes as C

import numpy as np
import pytest

import _policy as pol
import _policy_noise as pn
from aslr_to_amd import _abi

NAME = "aslr_policy_rollout_noise"

KNOWN = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


@pytest.mark.parametrize("counter, key, want", KNOWN)
def test_philox_known_answers(counter, key, want):
    got = tuple(int(v) for v in pn.philox4x32_10(counter, key))
    assert got == want, [hex(v) for v in got]


def test_philox_is_elementwise():
    """the three known answers as one call on arrays: what the draws rely on"""
    c = [np.array([k[0][i] for k in KNOWN]) for i in range(4)]
    key = [np.array([k[1][i] for k in KNOWN]) for i in range(2)]
    got = np.stack(pn.philox4x32_10(c, key), axis=-1)
    np.testing.assert_array_equal(got, np.array([k[2] for k in KNOWN], dtype=np.uint32))


def test_uniform_extremes():
    """words all ones -> u = 1 and r = 0 (a finite normal); words zero -> u = 2^-53, the largest r: |z| <= 8.58"""
    ones, zero = np.uint32(0xffffffff), np.uint32(0)
    assert pn.uniform(ones, ones) == 1.0 and pn.uniform(zero, zero) == 2.0 ** -53
    za, zb, r, ua, ub = pn.box_muller([ones] * 4)
    assert ua == 1.0 and ub == 1.0 and r == 0.0 and za == 0.0 and zb == 0.0
    za, zb, r, ua, ub = pn.box_muller([zero] * 4)
    assert ua == 2.0 ** -53 and np.isfinite(r) and 8.57 < r < 8.58
    # the reduced argument: exact at the quarter turns
    s, c = pn.sincospi(np.array([0.5, 1.0, 1.5, 2.0]))
    np.testing.assert_array_equal(np.abs(s), [1.0, 0.0, 1.0, 0.0])
    np.testing.assert_array_equal(np.abs(c), [0.0, 1.0, 0.0, 1.0])


def test_moments_of_the_normals():
    """2e5 normals (kind 0, 25 knots x 1000 samples x 8 entries): |mean| < 0.01, |std - 1| < 0.01, fourth moment within 0.1 of 3"""
    z = pn.normals(pn.SEED, pn.DISTURBANCE, np.arange(25)[:, None], np.arange(1000)[None, :], 7, 8).ravel()
    assert z.size == 200000
    mean, std, m4 = z.mean(), z.std(), ((z - z.mean()) ** 4).mean() / z.var() ** 2
    print("mean %.2e, std %.4f, fourth moment %.3f, max |z| %.2f" % (mean, std, m4, np.abs(z).max()))
    assert abs(mean) < 0.01 and abs(std - 1.0) < 0.01 and abs(m4 - 3.0) < 0.1
    assert np.abs(z).max() <= 8.58


def test_a_draw_depends_on_its_counter_alone():
    """entries of a pair share a block, an odd count discards the last sine, offsets shift the counter, kinds and seeds differ"""
    z8 = pn.normals(5, pn.DX0, 0, np.arange(4)[:, None], np.arange(3)[None, :], 8)
    z7 = pn.normals(5, pn.DX0, 0, np.arange(4)[:, None], np.arange(3)[None, :], 7)
    np.testing.assert_array_equal(z7, z8[..., :7])
    np.testing.assert_array_equal(pn.normals(5, pn.DX0, 0, 2 + np.arange(2)[:, None], 1 + np.arange(2)[None, :], 8), z8[2:, 1:])
    assert not (pn.normals(5, pn.STIFFNESS, 0, np.arange(4)[:, None], np.arange(3)[None, :], 8) == z8).any()
    assert not (pn.normals(5 + (1 << 32), pn.DX0, 0, np.arange(4)[:, None], np.arange(3)[None, :], 8) == z8).any()


def test_a_null_handle_is_refused_by_name():
    lib = _abi.load_library()
    assert lib.aslr_workspace_bytes(None) < 0     # some other message is in the buffer first
    buf = C.cast((C.c_double * 64)(), C.c_void_p)   # stands where a device pointer goes; never dereferenced
    assert lib.aslr_policy_rollout_noise(None, 4, 0, 0, 1, buf, None, None, None, 0, buf, *([None] * 9)) == _abi.E_INVALID
    msg = lib.aslr_last_error().decode()
    assert msg.startswith(NAME + ":") and "handle" in msg, msg


@pytest.mark.parametrize("key", pn.KEYS)
def test_no_sample_of_the_gpu_cases_diverges(oracle, key):
    """On the oracle alone, with the host-drawn arrays of the definition: failed_knot == -1 for every sample of every
    trajectory, and the closed loops leave the candidate (the draws are not too small to matter)"""
    c = pn.case(oracle, key)
    low, xs, us, S = c["low"], c["xs"], c["us"], c["S"]
    K = pol.oracle_gains(oracle, low, c["sp"], xs, us)
    pert = pn.draws(low, S, pn.SEED, **pn.sigmas(low))
    assert (pert["plant_stiffness"] is None) == (low.dam == _abi.DAM_VSA)
    for k, v in pert.items():
        assert v is None or np.isfinite(v).all(), k
    assert (pert["plant_motor_inertia"] > 0).all()
    got = pol.rollout(oracle, low, xs, us, K, S, clamp=c["clamp"], **pert)
    assert (got["failed_knot"] == -1).all() and np.isfinite(got["cost"]).all(), got["failed_knot"]
    moved_by = np.abs(got["xs"] - xs.transpose(1, 0, 2)[:, None]).max()
    print("%s: the loops leave the candidate by %.2e" % (key, moved_by))
    assert moved_by > 1e-4
