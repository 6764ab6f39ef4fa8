"""Shared by tests/test_policy_noise_host.py and tests/test_gpu_policy_noise.py: the generator of aslr_policy_rollout_noise
(include/aslr_to_amd_policy_noise.h) in numpy -- Philox4x32-10, the two 53-bit uniforms of a block, the
Box-Muller pair, and the four draws in the batch-major shapes of tests/_policy.py -- and the cases of the two suites.

Nothing here is taken from the library: the block function is written from its definition and held to the three known
answers by the host suite."""
import numpy as np

import _policy as pol
import _policy_team as pt
from aslr_to_amd import _abi

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
DISTURBANCE, DX0, STIFFNESS, MOTOR_INERTIA = 0, 1, 2, 3
MASK = np.uint64(0xFFFFFFFF)

# the sigmas of the suites: inside the +-1e-3 / +-1e-2 / +-30 % ranges of tests/_policy.perturbations at typical |z|.  No case
# needed a lower one: tests/test_policy_noise_host.py finds no diverging sample on the oracle with these.
SIGMAS = dict(noise_std=3e-4, dx0_std=3e-3, stiffness_rel_std=0.05, motor_inertia_rel_std=0.05)
SEED = 0x9E3779B97F4A7C15   # (both key words in use)
# the two-joint cases of tests/_policy.py and the arm cases of tests/_policy_team.py, at their shapes
TWO_JOINT = ("sea_table", "sea_one", "vsa_box", "pendulum_3d")
ARMS = tuple(sorted(pt.CASES))
KEYS = TWO_JOINT + ARMS


def philox4x32_10(c, k):
    """c: four arrays (or integers) of counter words, k: two of key words -> four uint32 arrays of output words"""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in np.broadcast_arrays(*c)]
    k = [np.asarray(v, dtype=np.uint64) & MASK for v in k]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]   # (32 x 32 bits: exact in 64)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return [v.astype(np.uint32) for v in c]


def uniform(hi, lo):
    """((hi >> 5) 2^26 + (lo >> 6) + 1) 2^-53: exact in double, in (0, 1]"""
    hi, lo = np.asarray(hi, dtype=np.uint32), np.asarray(lo, dtype=np.uint32)
    return ((hi >> np.uint32(5)).astype(np.float64) * 67108864.0 + (lo >> np.uint32(6)).astype(np.float64) + 1.0) * 2.0 ** -53


def sincospi(x):
    """sin(pi x), cos(pi x) for x in (0, 2] with the argument reduced exactly: x = n / 2 + f, |f| <= 1 / 4"""
    x = np.asarray(x, dtype=np.float64)
    n = np.rint(2.0 * x)
    f = x - 0.5 * n
    q = n.astype(np.int64) % 4
    s, c = np.sin(np.pi * f), np.cos(np.pi * f)
    return np.choose(q, [s, c, -s, -c]), np.choose(q, [c, -s, -c, s])


def box_muller(w):
    """the output words of a block -> (z_a, z_b, r, u_a, u_b)"""
    ua, ub = uniform(w[0], w[1]), uniform(w[2], w[3])
    r = np.sqrt(-2.0 * np.log(ua))
    sn, cs = sincospi(2.0 * ub)
    return r * cs, r * sn, r, ua, ub


def normals(seed, kind, t, s, b, n):
    """z(kind; t, s, b, i) for i < n: t, s, b integer arrays that broadcast against each other -> [..., n]"""
    t, s, b = np.broadcast_arrays(np.asarray(t), np.asarray(s), np.asarray(b))
    pair = np.arange((n + 1) // 2)
    w = philox4x32_10((t[..., None], s[..., None], b[..., None], (kind << 16) | pair), (seed & 0xFFFFFFFF, seed >> 32))
    za, zb = box_muller(w)[:2]
    return np.stack([za, zb], axis=-1).reshape(t.shape + (-1,))[..., :n]   # (an odd n discards the last sine)


def _sigma(v, B, n):
    return None if v is None else np.broadcast_to(np.asarray(v, dtype=np.float64), (B, n))


def nominal(low, field):
    """[B, nj]: the trajectory's own diagonal as the kernel has it -- its row of the table, else the models' constant.  The
    table holds 1 / B (formed on the host), so with a table the nominal B is the reciprocal of that reciprocal."""
    v = np.array([pol.nominal_diag(low, b, field) for b in range(low.B)])
    return 1.0 / (1.0 / v) if field == "B" and low.traj_params else v


def draws(low, S, seed, noise_std=None, dx0_std=None, stiffness_rel_std=None, motor_inertia_rel_std=None, sample0=0,
          trajectory0=0):
    """the four draws of the definition, batch-major as tests/_policy.perturbations gives them (None: source absent)"""
    B, T, nx, nj = low.B, low.T, low.nx, low.nj
    s, b = sample0 + np.arange(S)[None, :], trajectory0 + np.arange(B)[:, None]
    out = dict(plant_stiffness=None, plant_motor_inertia=None, dx0=None, disturbance=None)
    if noise_std is not None:
        z = normals(seed, DISTURBANCE, np.arange(T)[None, None, :], s[..., None], b[..., None], nx)
        out["disturbance"] = _sigma(noise_std, B, nx)[:, None, None, :] * z
    if dx0_std is not None:
        out["dx0"] = _sigma(dx0_std, B, nx)[:, None, :] * normals(seed, DX0, 0, s, b, nx)
    if stiffness_rel_std is not None:
        out["plant_stiffness"] = nominal(low, "K")[:, None, :] * np.exp(_sigma(stiffness_rel_std, B, nj)[:, None, :] * normals(seed, STIFFNESS, 0, s, b, nj))
    if motor_inertia_rel_std is not None:
        out["plant_motor_inertia"] = nominal(low, "B")[:, None, :] * np.exp(_sigma(motor_inertia_rel_std, B, nj)[:, None, :] * normals(seed, MOTOR_INERTIA, 0, s, b, nj))
    return out


def case(oracle, key):
    """the case of tests/_policy.py or tests/_policy_team.py with that name"""
    return pt.case(oracle, key) if key in pt.CASES else pol.case(oracle, key)


def sigmas(low):
    """SIGMAS for this model: no stiffness sigma on a VSA model"""
    return {k: (None if k == "stiffness_rel_std" and low.dam == _abi.DAM_VSA else v) for k, v in SIGMAS.items()}


def scale(low, sg):
    """what a difference in each draw is measured against: sigma for the additive draws, the nominal for the plant's"""
    B = low.B
    return dict(disturbance=None if sg["noise_std"] is None else _sigma(sg["noise_std"], B, low.nx)[:, None, None, :],
                dx0=None if sg["dx0_std"] is None else _sigma(sg["dx0_std"], B, low.nx)[:, None, :],
                plant_stiffness=nominal(low, "K")[:, None, :], plant_motor_inertia=nominal(low, "B")[:, None, :])
