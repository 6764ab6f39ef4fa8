"""Shared by tests/test_covariance_host.py and tests/test_gpu_covariance.py: what the CPU oracle says about
aslr_policy_covariance (include/aslr_to_amd_cov.h), without changing the oracle.

 - expected(): the DEFINITION in numpy with full matrices on the oracle's records (oracle.calc_diff, or the per-trajectory
   and reference-path sweeps of _traj_oracle / _ref_path where a table or a path is set) and a given K:
     A_t = Fx_t - Fu_t K_t,   Sigma_{t+1} = A_t Sigma_t A_t^T + diag(noise_var_t),   U_t = K_t Sigma_t K_t^T,
     cost_increase = 1/2 sum_{t<T} [tr(Lxx_t Sigma_t) - 2 tr(Lxu_t K_t Sigma_t) + tr(Luu_t U_t)] + 1/2 tr(Lxx_T Sigma_T).
   It takes xs, us and K as inputs: the GPU tests pass the device's own gains, so that only this sweep is compared.
 - inputs(): seeded sigma0 = M M^T + 0.1 I with M ~ U(-1, 1) and noise_var ~ U(0.1, 1), both of order 1 on purpose, so that
   a relative measure says something.
 - case(): the seeded scenario and candidate of the GPU cases -- seeded controls (clipped to the box where there is one) and
   the oracle's open-loop roll-out of them from x0, the recipe of tests/_policy.case.
 - traj_relerr(): per output array and trajectory max |a - b| / max |b|; the worst trajectory is returned.

Everything is time-major going in (the oracle's layout) and batch-major coming out, like Engine.policy_covariance: x_var
[B, T+1, nx], u_var [B, T, nu] (the device's nu), cov_final [B, nx, nx], cov [B, T+1, nx, nx], cost_increase [B]."""
import numpy as np

import _policy as pol
import _ref_path
import _traj_oracle
from aslr_to_amd import _abi, scenarios

OUTPUTS = ("x_var", "u_var", "cov_final", "cov", "cost_increase")

# key -> (scenario, table, path, B, T): the smallest shapes that leave a partial wave of teams (nx = 8: 8 teams per wave + 1;
# nx = 28: 2 per wave + 1) and the smallest problem there is
CASES = {
    "sea": ("two_dof_sea", True, False, 9, 5),
    "sea_path": ("two_dof_sea", True, True, 9, 5),
    "sea_one": ("two_dof_sea", False, False, 1, 1),
    "vsa_box": ("two_dof_vsa_boxddp", True, False, 9, 5),     # the narrowed box of _policy: some gain rows are zero
    "nu1": ("double_pendulum_nu1", False, False, 3, 3),        # padded control
    "arm_sea": ("talos_arm_sea", False, False, 3, 4),
    "arm_vsa": ("talos_arm_vsa", False, False, 3, 4),          # tight = True, SolverBoxDDP gains, (28, 14)
}
# the three input combinations every parity and conditioning check covers
COMBOS = {"sigma0": (True, False), "noise": (False, True), "both": (True, True)}
ARM_VSA_LB, ARM_VSA_UB = (-1.0,) * 7 + (1.0,) * 7, (1.0,) * 7 + (50.0,) * 7   # the box of talos_arm_vsa(tight=True)


def scenario(key):
    name, table, path, B, T = CASES[key]
    if name == "talos_arm_vsa":
        return scenarios.talos_arm_vsa(B=B, T=T, seed=4, tight=True)
    return pol.scenario(name, B, T, table, path)


def candidate(oracle, low, x0=None):
    """seeded controls (tests/_policy.case's recipe, seed 3) and their open-loop roll-out from x0 (default: the problem's)
    -> xs [T+1, B, nx], us [T, B, nu]"""
    T, B = low.T, low.B
    rng = np.random.default_rng(3)
    us = rng.uniform(-1.0, 1.0, (T, B, low.nu))
    if low.dam == _abi.DAM_VSA:
        if low.nj == 2:
            us[..., 2:] = rng.uniform(0.1, 5.0, (T, B, 2))
            us = np.clip(us, pol.BOX_LB, pol.BOX_UB)
        else:   # torques and stiffnesses drawn past the box on both sides, then clipped: some commands sit on a bound
            us[..., :7] = rng.uniform(-1.3, 1.3, (T, B, 7))
            us[..., 7:] = rng.uniform(0.5, 5.0, (T, B, 7))
            us = np.clip(us, ARM_VSA_LB, ARM_VSA_UB)
    if low.nu_user < low.nu:
        us[..., low.nu_user:] = 0.0   # padded commands
    zx, zk = np.zeros((T + 1, low.nx)), np.zeros((T, low.nu, low.nx))
    xs = np.stack([pol.rollout_one(oracle, low, b, zx, us[:, b], zk, x0=None if x0 is None else x0[b])["xs"]
                   for b in range(B)], axis=1)
    return xs, us


def case(oracle, key):
    """-> dict(key, sc, low, xs, us, sp, sigma0, noise_var)"""
    sc = scenario(key)
    low = scenarios.lower(sc)
    xs, us = candidate(oracle, low)
    sigma0, noise_var = inputs(low, 31)
    return dict(key=key, sc=sc, low=low, xs=xs, us=us, sp=scenarios.solver_params(sc), sigma0=sigma0, noise_var=noise_var)


def inputs(low, seed):
    """seeded, batch-major: sigma0 [B, nx, nx] = M M^T + 0.1 I with M ~ U(-1, 1) (symmetrised so that it is symmetric bit
    for bit), noise_var [B, T, nx] ~ U(0.1, 1)"""
    rng = np.random.default_rng(seed)
    M = rng.uniform(-1.0, 1.0, (low.B, low.nx, low.nx))
    s0 = M @ M.transpose(0, 2, 1) + 0.1 * np.eye(low.nx)
    s0 = 0.5 * (s0 + s0.transpose(0, 2, 1))
    return s0, rng.uniform(0.1, 1.0, (low.B, low.T, low.nx))


def combo(c, which):
    """(sigma0, noise_var) of the case with the ones `which` leaves out set to None"""
    use_s, use_w = COMBOS[which]
    return (c["sigma0"] if use_s else None), (c["noise_var"] if use_w else None)


def records(oracle, low, xs, us):
    """DERIV [T+1, B, rec] of the candidate from the oracle, through the sweep that honours what the problem has set"""
    path = getattr(low, "ref_path", None)
    if path is not None:
        return _ref_path.sweep(oracle, low, xs, us, path[0], path[1])[2]
    if low.traj_params:
        return _traj_oracle.calc_diff(oracle, low, xs, us)[2]
    return oracle.calc_diff(low, xs, us)[2]


def blocks(low, deriv):
    """-> dict of [T+1, B, rows, cols] views of the record blocks"""
    nx, nu = low.nx, low.nu
    o = _abi.record_offsets(nx, nu)
    shp = {"Fx": (nx, nx), "Fu": (nx, nu), "Lxx": (nx, nx), "Lxu": (nx, nu), "Luu": (nu, nu)}
    return {k: deriv[:, :, o[k]:o[k] + r * c].reshape(low.T + 1, low.B, r, c) for k, (r, c) in shp.items()}


def closed_loop(low, deriv, K):
    """A [T, B, nx, nx] = Fx - Fu K"""
    blk = blocks(low, deriv)
    return blk["Fx"][:low.T] - blk["Fu"][:low.T] @ K


def propagate(low, deriv, K, sigma0=None, noise_var=None):
    """the definition on given records; sigma0 [B, nx, nx], noise_var [B, T, nx] batch-major, None = 0"""
    T, B, nx, nu = low.T, low.B, low.nx, low.nu
    blk = blocks(low, deriv)
    A = closed_loop(low, deriv, K)
    cov = np.zeros((B, T + 1, nx, nx))
    u_var, cost = np.zeros((B, T, nu)), np.zeros(B)
    for b in range(B):
        S = np.zeros((nx, nx)) if sigma0 is None else np.array(sigma0[b], dtype=np.float64)
        for t in range(T):
            cov[b, t] = S
            Kt = K[t, b]
            U = Kt @ S @ Kt.T
            u_var[b, t] = np.diag(U)
            cost[b] += 0.5 * (np.trace(blk["Lxx"][t, b] @ S) - 2.0 * np.trace(blk["Lxu"][t, b] @ Kt @ S)
                              + np.trace(blk["Luu"][t, b] @ U))
            S = A[t, b] @ S @ A[t, b].T
            if noise_var is not None:
                S = S + np.diag(noise_var[b, t])
        cov[b, T] = S
        cost[b] += 0.5 * np.trace(blk["Lxx"][T, b] @ S)
    return dict(x_var=np.einsum("btii->bti", cov).copy(), u_var=u_var, cov_final=cov[:, T].copy(), cov=cov, cost_increase=cost)


def expected(oracle, low, xs, us, K, sigma0=None, noise_var=None):
    return propagate(low, records(oracle, low, xs, us), K, sigma0, noise_var)


def traj_relerr(a, b):
    """max over the trajectories (axis 0) of max |a - b| / max |b|; a trajectory whose reference is all zero must match
    exactly (-> 0.0, else inf)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    worst = 0.0
    for i in range(b.shape[0]):
        num, den = np.abs(a[i] - b[i]).max(), np.abs(b[i]).max()
        if not np.isfinite(num):
            return float("inf")
        worst = max(worst, (0.0 if num == 0.0 else float("inf")) if den == 0.0 else float(num / den))
    return worst
