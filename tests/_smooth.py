"""Shared by tests/test_smooth_host.py and tests/test_gpu_smooth.py: what the CPU oracle says about aslr_state_smooth
(include/aslr_to_amd_smooth.h), without changing the oracle.

 - once(): ONE iteration of the DEFINITION in numpy with full matrices on given records (tests/_covariance.blocks) and the
   oracle's xnext, about the nominal xb:
     filter (t = 0 .. T), from m^-_0 = x0_mean, Pm_0 = sigma0
       G = Pm[:, m],  S = Pm[m, m] + diag(meas_var) = C C^T,  L = G S^-1,  nu = y - m^-[m],  w = S^-1 nu,  mf = m^- + L nu,
       P = Pm - L G^T (symmetrised, (a + b) / 2),  nis = nu^T w,
       m^-' = xnext + Fx (mf - xb),  Pm' = Fx P Fx^T + diag(noise_var_t)                                            (t < T)
       nll = 1/2 sum_t (nis_t + 2 sum_a log C_t[a][a]), in knot order
     adjoint (t = T .. 0), from q^+_T = 0
       q = q^+, and q[m_a] = q^+[m_a] + w[a] - L[:, a] . q^+;   xs = m^- + Pm q;   q^+_{t-1} = Fx_{t-1}^T q
     step = max |xs - xb|
   A factor that does not exist (a pivot <= 0) makes the trajectory NaN from that knot on, as the header says.
 - iterate(): n_iters of them, the nominal re-evaluated through the oracle each time (sweep(): the sweep that honours what
   the problem has set) and moved by relax (xs - xb).
 - inputs(): the seeded data of a case -- the true run is tests/_covariance.candidate's roll-out, ys its measured entries plus
   sqrt(meas_var) z, the nominal the true run plus 1e-2 z', x0_mean the true x0 plus 1e-2 z''.  Measured sets, meas_var and its
   per-case scaling are those of tests/_lqg.py.

Time-major going in (the oracle's layout) for xs, us; everything the call takes or returns is batch-major, like
Engine.estimate_states: ys [B, T+1, ny], xs_smooth, x_filt, est_var [B, T+1, nx], nis [B, T+1], neg_log_lik, step_norm
[B, n_iters]."""
import numpy as np

import _covariance as cv
import _lqg as lq
import _ref_path
import _traj_oracle

OUTPUTS = ("xs_smooth", "x_filt", "est_var", "nis", "neg_log_lik", "step_norm")

# On top of tests/_lqg.MEAS_SCALE.  nu1 is the double pendulum with one control and T = 3.  With meas_var ~ U(0.1, 1) against a
# prior that its |Fx| spreads to variances of 1e3 within three knots, P = Pm - D cancels three to four digits and nis and
# step_norm moved by 1.04e-11 under the 1e-13 of the conditioning test (tests/test_smooth_host.py); a factor 10 still gave
# 1.1e-11, a factor 100 gives 4.2e-12.  As in tests/_lqg.py the measurement noise is scaled to the spread, not the bound.
MEAS_SCALE = {"nu1": 1e2}


def sweep(oracle, low, xs, us):
    """-> xnext [T+1, B, nx], DERIV [T+1, B, rec] of the nominal from the oracle (the choice of tests/_covariance.records)"""
    path = getattr(low, "ref_path", None)
    if path is not None:
        out = _ref_path.sweep(oracle, low, xs, us, path[0], path[1])
    elif low.traj_params:
        out = _traj_oracle.calc_diff(oracle, low, xs, us)
    else:
        out = oracle.calc_diff(low, xs, us)
    return out[0], out[2]


def inputs(c, which="default", seed=71, noise=True):
    """the seeded data of the case c (tests/_covariance.case) for the measured set `which` -> dict(m, r [B, ny], ys
    [B, T+1, ny], nominal [T+1, B, nx], x0_mean [B, nx]); noise False: exact measurements, the nominal and x0_mean still moved"""
    low = c["low"]
    m = lq.measured(low.nx, which)
    r = MEAS_SCALE.get(c["key"], 1.0) * lq.meas_var(low.B, len(m), c["key"])
    rng = np.random.default_rng(seed)
    true = c["xs"].transpose(1, 0, 2)
    z = rng.standard_normal((low.B, low.T + 1, len(m)))
    ys = true[:, :, m] + (np.sqrt(r)[:, None, :] * z if noise else 0.0)
    nominal = c["xs"] + 1e-2 * rng.standard_normal(c["xs"].shape)
    x0_mean = true[:, 0] + 1e-2 * rng.standard_normal((low.B, low.nx))
    return dict(m=m, r=r, ys=ys, nominal=nominal, x0_mean=x0_mean)


def once(low, deriv, xnext, xb, ys, m, r, x0_mean, sigma0=None, noise_var=None):
    """one iteration on given records.  xnext, xb [T+1, B, nx] time-major; the rest batch-major, None = 0 -> batch-major dict:
    the per-knot outputs, nll [B], step [B], and the full Pm, P, L, w, mm (m^-) for the host tests"""
    T, B, nx = low.T, low.B, low.nx
    m = list(m)
    ny = len(m)
    Fx = cv.blocks(low, deriv)["Fx"]
    xs, xf, mms = (np.zeros((B, T + 1, nx)) for _ in range(3))
    Pms, Ps = np.zeros((B, T + 1, nx, nx)), np.zeros((B, T + 1, nx, nx))
    Ls, ws, nus = np.zeros((B, T + 1, nx, ny)), np.zeros((B, T + 1, ny)), np.zeros((B, T + 1, ny))
    nis, nll, step = np.zeros((B, T + 1)), np.zeros(B), np.zeros(B)
    for b in range(B):
        Pm = np.zeros((nx, nx)) if sigma0 is None else np.array(sigma0[b], dtype=np.float64)
        mm = np.array(x0_mean[b], dtype=np.float64)
        for t in range(T + 1):
            G = Pm[:, m]
            S = Pm[np.ix_(m, m)] + np.diag(r[b])
            try:
                if not np.isfinite(S).all():
                    raise np.linalg.LinAlgError
                C = np.linalg.cholesky(S)
            except np.linalg.LinAlgError:
                C = np.full((ny, ny), np.nan)
            solve = lambda rhs: np.linalg.solve(C.T, np.linalg.solve(C, rhs)) if np.isfinite(C).all() else np.full(np.shape(rhs), np.nan)
            L = solve(G.T).T
            nu = ys[b, t] - mm[m]
            w = solve(nu)
            mf = mm + L @ nu
            P = Pm - L @ G.T
            P = 0.5 * (P + P.T)
            nis[b, t] = nu @ w
            nll[b] = nll[b] + 0.5 * (nis[b, t] + 2.0 * np.log(np.diag(C)).sum())
            Pms[b, t], Ps[b, t], Ls[b, t], ws[b, t], nus[b, t], mms[b, t], xf[b, t] = Pm, P, L, w, nu, mm, mf
            if t < T:
                mm = xnext[t, b] + Fx[t, b] @ (mf - xb[t, b])
                Pm = Fx[t, b] @ P @ Fx[t, b].T
                if noise_var is not None:
                    Pm = Pm + np.diag(noise_var[b, t])
        qp = np.zeros(nx)
        for t in range(T, -1, -1):
            q = qp.copy()
            q[m] = qp[m] + ws[b, t] - Ls[b, t].T @ qp
            xs[b, t] = mms[b, t] + Pms[b, t] @ q
            if t > 0:
                qp = Fx[t - 1, b].T @ q
        step[b] = np.abs(xs[b] - xb[:, b]).max()
    return dict(xs_smooth=xs, x_filt=xf, est_var=np.einsum("btii->bti", Ps).copy(), nis=nis, nll=nll, step=step,
                Pm=Pms, P=Ps, L=Ls, w=ws, nu=nus, mm=mms)


def iterate(oracle, low, xs0, us, ys, m, r, x0_mean, sigma0=None, noise_var=None, n_iters=1, relax=1.0):
    """the definition: n_iters iterations from the nominal xs0 [T+1, B, nx] -> the six outputs of the call, batch-major, and
    XS [T+1, B, nx]: what the handle's XS holds afterwards"""
    xb = np.array(xs0, dtype=np.float64)
    nll, step = np.zeros((low.B, n_iters)), np.zeros((low.B, n_iters))
    with np.errstate(invalid="ignore"):
        for s in range(n_iters):
            xnext, deriv = sweep(oracle, low, xb, us)
            last = once(low, deriv, xnext, xb, ys, m, r, x0_mean, sigma0, noise_var)
            nll[:, s], step[:, s] = last["nll"], last["step"]
            xs_tm = last["xs_smooth"].transpose(1, 0, 2)
            xb = xb + relax * (xs_tm - xb)
    return dict(xs_smooth=last["xs_smooth"], x_filt=last["x_filt"], est_var=last["est_var"], nis=last["nis"], neg_log_lik=nll,
                step_norm=step, XS=xb)
