"""Shared by tests/test_lqg_host.py and tests/test_gpu_lqg.py: what the CPU oracle says about aslr_policy_lqg
(include/aslr_to_amd_lqg.h), without changing the oracle.

 - propagate(): the DEFINITION in numpy with full matrices on given records (tests/_covariance.records / blocks) and a given K:
     Pm_0 = sigma0, Xm_0 = 0
     update (t = 0 .. T)   G = Pm[:, m],  S = Pm[m, m] + diag(meas_var),  L = G S^-1 (Cholesky of S),  D = L G^T,
                           P = Pm - D,  Xh = Xm + D
     outputs               Sigma = Xh + P,  U = K Xh K^T (t < T)
     predict (t < T)       Pm' = Fx P Fx^T + diag(noise_var_t),  Xm' = A Xh A^T,  A = Fx - Fu K
     cost_increase = 1/2 sum_{t<T} [tr(Lxx Sigma) - 2 tr(Lxu K Xh) + tr(Luu U)] + 1/2 tr(Lxx_T Sigma_T), in knot order.
   Beside the seven outputs of the call it returns the full matrices (Sigma, Xh, P, Pm, U), for the host tests.
 - augmented(): the 2 nx x 2 nx covariance of [e; eh] propagated directly with GIVEN filter gains, the prior / posterior steps
   written out with (I - L C) and L R L^T: no orthogonality of estimate and error is assumed.  The host tests hold
   propagate() to it.
 - measured sets and seeded meas_var ~ U(0.1, 1), of order 1 like tests/_covariance.inputs (MEAS_SCALE: two cases scale it).

Batch-major like Engine.policy_lqg: x_var, est_var [B, T+1, nx], u_var [B, T, nu] (the device's nu), cov_final, est_cov_final
[B, nx, nx], kalman_gain [B, T+1, nx, ny], cost_increase [B]."""
import numpy as np

import _covariance as cv

OUTPUTS = ("x_var", "u_var", "est_var", "cov_final", "est_cov_final", "kalman_gain", "cost_increase")
SETS = ("default", "one", "all", "odd")
_ODD = {8: [5, 0, 6], 28: [20, 3, 27, 9, 14]}


def measured(nx, which):
    """the measured state entries of the set `which`: the positions; the last entry alone; a seeded permutation of all nx; a
    short unsorted list"""
    if which == "default":
        return list(range(nx // 2))
    if which == "one":
        return [nx - 1]
    if which == "all":
        return [int(i) for i in np.random.default_rng(61).permutation(nx)]
    return list(_ODD[nx])


# The two VSA cases of tests/_covariance.CASES spread to variances of 1e5 within their few knots (max |Fx| 168 and 50).  A
# measurement of variance 1 is exact on that scale: P = Pm - D then cancels five digits, and the filter's outputs move by up
# to 9e-11 under the 1e-13 of the conditioning test (tests/test_lqg_host.py).  Their meas_var is scaled to the spread instead.
MEAS_SCALE = {"vsa_box": 1e4, "arm_vsa": 1e4}


def meas_var(B, ny, key=None, seed=67):
    """seeded [B, ny] ~ U(0.1, 1), times MEAS_SCALE of the case `key`"""
    return MEAS_SCALE.get(key, 1.0) * np.random.default_rng(seed).uniform(0.1, 1.0, (B, ny))


def gain(Pm, m, r):
    """L = Pm[:, m] (Pm[m, m] + diag(r))^-1 through the Cholesky factor -> L [nx, ny], G [nx, ny]"""
    G = Pm[:, m]
    c = np.linalg.cholesky(Pm[np.ix_(m, m)] + np.diag(r))
    return np.linalg.solve(c.T, np.linalg.solve(c, G.T)).T, G


def propagate(low, deriv, K, m, r, sigma0=None, noise_var=None):
    """the definition on given records.  m: the measured entries; r [B, ny]; sigma0 [B, nx, nx], noise_var [B, T, nx]
    batch-major, None = 0"""
    T, B, nx, nu = low.T, low.B, low.nx, low.nu
    m = list(m)
    blk = cv.blocks(low, deriv)
    Sig, Xhs, Ps, Pms = (np.zeros((B, T + 1, nx, nx)) for _ in range(4))
    Ls, Us, cost = np.zeros((B, T + 1, nx, len(m))), np.zeros((B, T, nu, nu)), np.zeros(B)
    for b in range(B):
        Pm = np.zeros((nx, nx)) if sigma0 is None else np.array(sigma0[b], dtype=np.float64)
        Xm = np.zeros((nx, nx))
        for t in range(T + 1):
            L, G = gain(Pm, m, r[b])
            D = L @ G.T
            P, Xh = Pm - D, Xm + D
            S = Xh + P
            Pms[b, t], Ps[b, t], Xhs[b, t], Sig[b, t], Ls[b, t] = Pm, P, Xh, S, L
            if t == T:
                cost[b] += 0.5 * np.trace(blk["Lxx"][T, b] @ S)
                break
            Kt, Fx, Fu = K[t, b], blk["Fx"][t, b], blk["Fu"][t, b]
            U = Kt @ Xh @ Kt.T
            Us[b, t] = U
            cost[b] += 0.5 * (np.trace(blk["Lxx"][t, b] @ S) - 2.0 * np.trace(blk["Lxu"][t, b] @ Kt @ Xh) + np.trace(blk["Luu"][t, b] @ U))
            A = Fx - Fu @ Kt
            Pm = Fx @ P @ Fx.T
            if noise_var is not None:
                Pm = Pm + np.diag(noise_var[b, t])
            Xm = A @ Xh @ A.T
    diag = lambda M: np.einsum("btii->bti", M).copy()
    return dict(x_var=diag(Sig), u_var=diag(Us), est_var=diag(Ps), cov_final=Sig[:, T].copy(), est_cov_final=Ps[:, T].copy(),
                kalman_gain=Ls, cost_increase=cost, Sigma=Sig, Xh=Xhs, P=Ps, Pm=Pms, U=Us)


def expected(oracle, low, xs, us, K, m, r, sigma0=None, noise_var=None):
    return propagate(low, cv.records(oracle, low, xs, us), K, m, r, sigma0, noise_var)


def augmented(low, deriv, K, m, r, gains, sigma0=None, noise_var=None):
    """the covariance Z of [e; eh] under plant, measurement, a filter with the GIVEN gains [B, T+1, nx, ny] and the controller
    du = -K eh, propagated directly:
      update   [e; eh] = M [e; eh-] + [0; L] v,   M = [[I, 0], [L C, I - L C]]          Z = M Z- M^T + [0; L] R [0; L]^T
      predict  [e; eh-]' = N [e; eh] + [w; 0],    N = [[Fx, -Fu K], [0, Fx - Fu K]]     Z-' = N Z N^T + diag(W, 0)
    -> Sigma [B, T+1, nx, nx] (cov e), U [B, T, nu, nu] (cov du), cost_increase [B] (the expectation of the quadratic model,
    with E[eh e^T] read off Z), err [B, T+1, nx, nx] (cov of e - eh after the update)"""
    T, B, nx, nu = low.T, low.B, low.nx, low.nu
    m = list(m)
    blk = cv.blocks(low, deriv)
    C = np.zeros((len(m), nx))
    C[np.arange(len(m)), m] = 1.0
    I, O = np.eye(nx), np.zeros((nx, nx))
    Sig, err = np.zeros((B, T + 1, nx, nx)), np.zeros((B, T + 1, nx, nx))
    Us, cost = np.zeros((B, T, nu, nu)), np.zeros(B)
    for b in range(B):
        Z = np.block([[O if sigma0 is None else np.array(sigma0[b], dtype=np.float64), O], [O, O]])
        for t in range(T + 1):
            L = gains[b, t]
            M = np.block([[I, O], [L @ C, I - L @ C]])
            V = np.vstack([np.zeros((nx, len(m))), L])
            Z = M @ Z @ M.T + V @ np.diag(r[b]) @ V.T
            See, Shh, She = Z[:nx, :nx], Z[nx:, nx:], Z[nx:, :nx]
            Sig[b, t] = See
            err[b, t] = See - She - She.T + Shh
            if t == T:
                cost[b] += 0.5 * np.trace(blk["Lxx"][T, b] @ See)
                break
            Kt, Fx, Fu = K[t, b], blk["Fx"][t, b], blk["Fu"][t, b]
            Us[b, t] = Kt @ Shh @ Kt.T
            cost[b] += 0.5 * (np.trace(blk["Lxx"][t, b] @ See) - 2.0 * np.trace(blk["Lxu"][t, b] @ Kt @ She) + np.trace(blk["Luu"][t, b] @ Us[b, t]))
            N = np.block([[Fx, -Fu @ Kt], [O, Fx - Fu @ Kt]])
            Z = N @ Z @ N.T
            if noise_var is not None:
                Z[:nx, :nx] += np.diag(noise_var[b, t])
    return dict(Sigma=Sig, U=Us, cost_increase=cost, err=err)
