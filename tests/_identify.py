"""Shared by tests/test_identify_host.py and tests/test_gpu_identify.py: what the CPU oracle says about aslr_plant_identify
(include/aslr_to_amd_identify.h), without changing the oracle.

 - definition(): sse, g and H of a candidate from the DEFINITION -- r_t = y_{t+1} - xnext_t with the oracle's own knot
   evaluation on the B = 1 problem of trajectory b whose models carry the candidate (tests/_policy.plant_problem), and
   Jz_t = dxnext_t / dlog theta as central differences of that evaluation with the parameter moved, as
   tests/_sensitivity.expected forms them: xnext is linear in K_j and in 1 / B_j, so the differences are exact up to rounding
   whatever the step.  The kernel's two closed forms appear nowhere in this file.
 - step(): identify_step_kernel in numpy, operation by operation on float64 scalars (every product, sum and quotient rounded
   on its own, which is what the kernel does with contraction off), so the two agree bit for bit; run(): the loop around it,
   driven through a `normal(theta)` callable -- definition() here, the GPU kernel in tests/test_gpu_identify.py.
 - case(): the seeded data.  The policy is the oracle's solve of the scenario and the gains of one backward sweep on its
   solution; Y and U are its closed-loop run (tests/_policy.rollout_one) on a plant whose K and B lie within +-20 % of the
   model's.  Every joint is excited by dx0 and by a seeded dither on the policy's feed-forward controls, which U records; a
   disturbance on the STATE would be a one-step prediction error at the true parameters, i.e. noise, and the data of the
   recovery tests are noise-free.

theta is [np][B] like the call's rows: the fitted fields' entries, stiffness first.  `fields`: "KB", "K" or "B"."""
import numpy as np

import _policy as pol
import _traj_oracle
from aslr_to_amd import _abi, scenarios

DEFAULTS = dict(mu0=1e-3, mu_min=1e-12, mu_max=1e12, grow=10.0, shrink=0.1, max_rel=0.5, min_curv=1e-12)

# name -> (scenario, B, T, fields, n_steps, mu0, max_rel).  Shapes: nx = 8 runs 8 trajectories per wave, B = 11 is a full wave
# and a partial one; nx = 28 runs 2 per wave, B = 3 is a full wave and a lone trajectory; T = 7 is odd.  mu0 and max_rel were
# picked on the reference alone so that every case accepts and rejects (tests/test_identify_host.py): from the poor guess of
# case() a step damped by mu = 0.1 overshoots and max_rel = 0.9 lets it; n_steps so that at least two thirds of the steps
# lie before the reference has converged (compared_steps).
CASES = {
    "sea": ("two_dof_sea", 11, 7, "KB", 10, 1.0, 0.9),
    "vsa": ("two_dof_vsa_boxddp", 11, 7, "B", 10, 1.0, 0.9),
    "arm_sea": ("talos_arm_sea", 3, 7, "KB", 12, 1.0, 0.9),
    "arm_vsa": ("talos_arm_vsa", 3, 7, "B", 12, 1.0, 0.9),
}
GUESS = 2.6
FLOOR = 1e-20
MARGIN = 1e-6      # a compared decision has |sse_try - sse_acc| > MARGIN sse_acc
# Recovery of the true plant, max |theta_acc / theta_true - 1| after N_RECOVER steps of the reference loop on noise-free data,
# measured on the oracle alone (tests/test_identify_host.py prints and pins it): (the data of case(): Y, U; the same run
# without the dither: Y_plain, U_plain, the CPU twin of the data tests/test_gpu_identify.py makes on the device with
# aslr_policy_rollout[_all]).  N_RECOVER is past the convergence of every trajectory of every case, so the figures are the
# rounding of the fit, not where a loop happened to stop.  A figure below ULP4 = 4 ulp of theta is recorded as ULP4: so close
# to the format's resolution the measured value says which way the last bits of theta fell on this machine, not how well the
# reference recovers.  The GPU bound is 16 times the recorded figure.
N_RECOVER = 16
ULP4 = 4 * 2.0 ** -52
# measured: sea 4.4e-16 / 2.2e-16, vsa 2.2e-16 / 7.8e-16, arm_sea 1.78e-15 / 2.89e-15, arm_vsa 2.2e-16 / 2.2e-16
RECOVERY = {"sea": (ULP4, ULP4), "vsa": (ULP4, ULP4), "arm_sea": (1.8e-15, 2.9e-15), "arm_vsa": (ULP4, ULP4)}
assert _abi.IDENTIFY_SYMBOLS == ["aslr_plant_identify"]   # (the suites of this file are about that call: no call, no suite)


def n_params(nj, fields):
    return len(fields) * nj


def split(theta, nj, fields):
    """theta [np][B] -> (K [nj][B] or None, B [nj][B] or None)"""
    k = theta[:nj] if "K" in fields else None
    b = theta[(nj if "K" in fields else 0):][:nj] if "B" in fields else None
    return k, b


def full_diag(c, theta, b):
    """(diag K, diag B) of trajectory b under theta: the fitted entries from theta, the others the model's"""
    k, bm = split(theta, c["low"].nj, c["fields"])
    return (c["model_k"][:, b] if k is None else k[:, b]), (c["model_b"][:, b] if bm is None else bm[:, b])


def pack(M):
    """symmetric [np][np] -> packed lower [np (np+1)/2]"""
    return M[np.tril_indices(M.shape[0])]


def unpack(h, npar):
    M = np.zeros((npar, npar) + h.shape[1:])
    p, q = np.tril_indices(npar)
    M[p, q] = h
    M[q, p] = h
    return M


def jacobian(oracle, c, theta, b, t):
    """(r_t [nx], Jz_t [nx][np]) of trajectory b at knot t under theta, from the definition"""
    low, Y, U, fields = c["low"], c["Y"], c["U"], c["fields"]
    nj = low.nj
    mi = int(low.node_model[t])
    k, bm = full_diag(c, theta, b)
    xn = lambda kk, bb: oracle.knot(pol.plant_problem(low, b, kk, bb), mi, Y[t, b], U[t, b], diff=False)["xnext"]
    r = Y[t + 1, b] - xn(k, bm)
    cols = []
    if "K" in fields:
        for j in range(nj):
            h = 0.25 * abs(k[j])
            kp, km = k.copy(), k.copy()
            kp[j] += h
            km[j] -= h
            cols.append(k[j] * (xn(kp, bm) - xn(km, bm)) / (2 * h))
    if "B" in fields:
        for j in range(nj):
            ri = 1.0 / bm[j]
            h = 0.25 * ri
            bp, bn = bm.copy(), bm.copy()
            bp[j] = 1.0 / (ri + h)
            bn[j] = 1.0 / (ri - h)
            d = (xn(k, bp) - xn(k, bn)) / (2 * h)   # dxnext / d(1 / B_j);  dxnext / dlog B_j = -(1 / B_j) of it
            cols.append(-ri * d)
    return r, np.stack(cols, axis=1)


def definition(oracle, c, theta, weights=None):
    """-> sse [B], g [np][B], H [np (np+1)/2][B] of the candidate theta [np][B]"""
    low = c["low"]
    B, T, nx = low.B, low.T, low.nx
    npar = theta.shape[0]
    sse, g, H = np.zeros(B), np.zeros((npar, B)), np.zeros((npar * (npar + 1) // 2, B))
    for b in range(B):
        w = np.ones(nx) if weights is None else weights[b]
        Hb = np.zeros((npar, npar))
        for t in range(T):
            r, J = jacobian(oracle, c, theta, b, t)
            sse[b] += np.sum(w * r * r)
            g[:, b] -= J.T @ (w * r)
            Hb += J.T @ (w[:, None] * J)
        H[:, b] = pack(Hb)
    return sse, g, H


# ---------------------------------------------------------------------------------------------
# the step, bit for bit
# ---------------------------------------------------------------------------------------------
def new_state(theta0):
    npar, B = theta0.shape
    nh = npar * (npar + 1) // 2
    return dict(theta=np.array(theta0, dtype=np.float64), sse=np.zeros(B), grad=np.zeros((npar, B)), info=np.zeros((nh, B)),
                mu=np.zeros(B), identifiable=np.zeros((npar, B), dtype=np.int32), n_accepted=np.zeros(B, dtype=np.int32),
                theta_try=np.array(theta0, dtype=np.float64))


def _at(p, q):
    return p * (p + 1) // 2 + q


def _solve(H, g, msk, mu, mu_max, grow):
    """A = H + mu diag(H) = L D L^T on the masked block, dz = -A^-1 g -> (dz or None, mu): the kernel's loop"""
    f = np.float64
    npar = len(g)
    tries = 0
    while True:
        A = [f(0.0)] * len(H)
        for p in range(npar):
            for q in range(p + 1):
                h = H[_at(p, q)]
                if p == q:
                    A[_at(p, q)] = (h + mu * h) if msk[p] else f(1.0)
                else:
                    A[_at(p, q)] = h if (msk[p] and msk[q]) else f(0.0)
        D = [f(0.0)] * npar
        ok = True
        for p in range(npar):
            d = A[_at(p, p)]
            for k in range(p):
                d = d - (A[_at(p, k)] * A[_at(p, k)]) * D[k]
            if not (d > 0.0) or not np.isfinite(d):
                ok = False
                break
            D[p] = d
            for i in range(p + 1, npar):
                v = A[_at(i, p)]
                for k in range(p):
                    v = v - (A[_at(i, k)] * A[_at(p, k)]) * D[k]
                A[_at(i, p)] = v / d
        if ok:
            break
        if not (mu < mu_max) or tries == 63:
            return None, mu
        mu = mu * grow
        if mu > mu_max:
            mu = mu_max
        tries += 1
    x = [f(0.0)] * npar
    for p in range(npar):
        v = -g[p] if msk[p] else f(0.0)
        for k in range(p):
            v = v - A[_at(p, k)] * x[k]
        x[p] = v
    for p in range(npar):
        x[p] = x[p] / D[p]
    for p in range(npar - 1, -1, -1):
        v = x[p]
        for k in range(p + 1, npar):
            v = v - A[_at(k, p)] * x[k]
        x[p] = v
    return x, mu


def step(st, s, last, sse_try, g_try, h_try, lo, hi, mu0, mu_min, mu_max, grow, shrink, max_rel, min_curv):
    """One launch of identify_step_kernel: st (new_state) is updated in place; st["theta_try"] holds the candidate that was
    evaluated and takes the next one.  -> dict(decision [B], theta_eval [np][B], sse_eval [B], next [np][B]: the candidate
    written to the table (K and B themselves), margin [B]: |sse_try - sse_acc| / sse_acc where the comparison decided)"""
    f = np.float64
    npar, B = st["theta"].shape
    nh = npar * (npar + 1) // 2
    out = dict(decision=np.zeros(B, dtype=np.int32), theta_eval=st["theta_try"].copy(), sse_eval=np.array(sse_try, dtype=f),
               next=np.zeros((npar, B)), margin=np.full(B, np.nan))
    with np.errstate(all="ignore"):
        for b in range(B):
            sse_t = f(sse_try[b])
            mu_in = f(mu0) if s == 0 else f(st["mu"][b])
            frozen = s > 0 and mu_in < 0.0
            evaluable = bool(np.isfinite(sse_t))
            accept = evaluable if s == 0 else (not frozen and evaluable and bool(sse_t < st["sse"][b]))
            freeze = frozen or (s == 0 and not evaluable)
            take = accept or s == 0
            if s > 0 and not frozen and evaluable:
                out["margin"][b] = abs(sse_t - st["sse"][b]) / st["sse"][b]
            out["decision"][b] = -1 if (freeze or not evaluable) else int(accept)
            if take:
                st["theta"][:, b] = st["theta_try"][:, b]
                st["grad"][:, b] = g_try[:, b]
                st["info"][:, b] = h_try[:, b]
                st["sse"][b] = sse_t
            st["n_accepted"][b] = (0 if s == 0 else st["n_accepted"][b]) + int(accept)
            if freeze:
                mu = f(-1.0)
            elif accept:
                mu = mu_in * f(shrink)
                mu = f(mu_min) if mu < mu_min else mu
            else:
                mu = mu_in * f(grow)
                mu = f(mu_max) if mu > mu_max else mu
            H = [f(v) for v in st["info"][:, b]]
            g = [f(v) for v in st["grad"][:, b]]
            th = [f(v) for v in st["theta"][:, b]]
            maxd = H[0]
            for q in range(1, npar):
                if H[_at(q, q)] > maxd:
                    maxd = H[_at(q, q)]
            thr = f(min_curv) * maxd
            msk = [(not freeze) and bool(H[_at(p, p)] > thr) for p in range(npar)]
            st["identifiable"][:, b] = msk
            x = None
            if not last and not freeze:
                x, mu = _solve(H, g, msk, mu, f(mu_max), f(grow))
            st["mu"][b] = mu
            for p in range(npar):
                nxt = th[p]
                if x is not None and msk[p]:
                    dz = x[p]
                    dz = f(-max_rel) if dz < -max_rel else (f(max_rel) if dz > max_rel else dz)
                    nxt = th[p] * (f(1.0) + dz)
                    nxt = f(lo[p, b]) if nxt < lo[p, b] else (f(hi[p, b]) if nxt > hi[p, b] else nxt)
                st["theta_try"][p, b] = nxt
                out["next"][p, b] = nxt
    assert nh == st["info"].shape[0]
    return out


def run(normal, theta0, lo, hi, n_steps, **kw):
    """The loop of aslr_plant_identify driven from the host.  normal(theta [np][B]) -> (sse, g, H).  -> dict(state,
    decision [n][B], theta_hist [n][np][B], sse_hist [n][B], margin [n][B], sse_acc [n][B]: the accepted sse after step s)"""
    p = dict(DEFAULTS)
    p.update(kw)
    st = new_state(theta0)
    out = dict(decision=[], theta_hist=[], sse_hist=[], margin=[], sse_acc=[])
    for s in range(n_steps):
        sse, g, H = normal(st["theta_try"].copy())
        r = step(st, s, s == n_steps - 1, sse, g, H, lo, hi, **p)
        out["decision"].append(r["decision"])
        out["theta_hist"].append(r["theta_eval"])
        out["sse_hist"].append(r["sse_eval"])
        out["margin"].append(r["margin"])
        out["sse_acc"].append(st["sse"].copy())
    out = {k: np.stack(v) for k, v in out.items()}
    out["state"] = st
    return out


def table_rows(theta, nj, fields):
    """what the step kernel writes into TRAJ_PARAMS for theta [np][B]: (first row, rows): K as it is, 1.0 / B"""
    k, bm = split(theta, nj, fields)
    rows = ([k] if k is not None else []) + ([1.0 / bm] if bm is not None else [])
    return (0 if k is not None else nj), np.concatenate(rows)


# ---------------------------------------------------------------------------------------------
# the data
# ---------------------------------------------------------------------------------------------
_made = {}


def case(oracle, name):
    """-> dict(sc, low, fields, Y [T+1, B, nx], U [T, B, nu] time-major, model_k / model_b [nj][B]: the model's diagonals
    (theta_0), true_k / true_b: the plant's, theta0 / truth [np][B], lo, hi, n_steps, mu0, max_rel); built once, shared,
    never changed"""
    if name in _made:
        return _made[name]
    scen, B, T, fields, n_steps, mu0, max_rel = CASES[name]
    sc = scenarios.with_traj_params(scenarios.SCENARIOS[scen](B=B, T=T, seed=4), seed=5)
    low = scenarios.lower(sc)
    nj, nx, nu = low.nj, low.nx, low.nu
    sp = scenarios.solver_params(sc, maxiter=30)
    sol = _traj_oracle.solve(oracle, low, sp)
    xs, us = sol["xs"], sol["us"]
    # (mild gains, as tests/_gpu_case.forward_inputs takes them: the full gains of one regularised sweep are unstable on some
    #  of the mismatched plants, and a run that grows to 1e18 says nothing about the parameters)
    K = 0.05 * pol.oracle_gains(oracle, low, sp, xs, us)
    rng = np.random.default_rng(11)
    mk = np.stack([pol.nominal_diag(low, b, "K") for b in range(B)], axis=1)
    mb = np.stack([pol.nominal_diag(low, b, "B") for b in range(B)], axis=1)
    tk, tb = mk * rng.uniform(0.8, 1.2, mk.shape), mb * rng.uniform(0.8, 1.2, mb.shape)
    vsa = low.dam == _abi.DAM_VSA
    dx0 = rng.uniform(-0.2, 0.2, (B, nx))
    dither = rng.uniform(-0.5, 0.5, (T, B, nu))
    if vsa:   # the stiffness commands stay positive and inside the box
        dither[..., nu // 2:] = 0.0
    if low.nu_user < nu:
        dither[..., low.nu_user:] = 0.0
    Y, U = np.zeros((T + 1, B, nx)), np.zeros((T, B, nu))
    for b in range(B):
        r = pol.rollout_one(oracle, low, b, xs[:, b], us[:, b] + dither[:, b], K[:, b], None if vsa else tk[:, b], tb[:, b], dx0[b])
        assert r["failed_knot"] < 0
        Y[:, b], U[:, b] = r["xs"], r["us"]
    Yp, Up = np.zeros_like(Y), np.zeros_like(U)
    for b in range(B):   # the same run without the dither
        r = pol.rollout_one(oracle, low, b, xs[:, b], us[:, b], K[:, b], None if vsa else tk[:, b], tb[:, b], dx0[b])
        assert r["failed_knot"] < 0
        Yp[:, b], Up[:, b] = r["xs"], r["us"]
    c = dict(sc=sc, low=low, fields=fields, Y=Y, U=U, Y_plain=Yp, U_plain=Up, model_k=mk, model_b=mb, true_k=tk, true_b=tb, n_steps=n_steps, mu0=mu0,
             max_rel=max_rel, sp=sp, xs=xs, us=us, K=K, dx0=dx0, dither=dither)
    # the fit starts from a poor guess of every second motor inertia, GUESS times the model's: a Gauss-Newton step in log B
    # from more than twice the true value overshoots (1 / B is what the step is linear in), so the loop has steps to reject
    g0 = mb * np.where(np.arange(nj) % 2 == 1, GUESS, 1.0)[:, None]
    c["start_k"], c["start_b"] = mk, g0
    c["theta0"] = np.concatenate(([mk] if "K" in fields else []) + ([g0] if "B" in fields else []))
    c["truth"] = np.concatenate(([tk] if "K" in fields else []) + ([tb] if "B" in fields else []))
    c["lo"], c["hi"] = c["theta0"] / 10.0, c["theta0"] * 3.0
    _made[name] = c
    return c


def params(c, **over):
    return dict(DEFAULTS, mu0=c["mu0"], max_rel=c["max_rel"], **over)


_runs = {}


def reference_run(oracle, name):
    """the reference loop of the case on noise-free data; built once, shared, never changed"""
    if name not in _runs:
        c = case(oracle, name)
        _runs[name] = run(lambda th: definition(oracle, c, th), c["theta0"], c["lo"], c["hi"], c["n_steps"], **params(c))
    return _runs[name]


def plain(c):
    """the case on the data without the dither"""
    return dict(c, Y=c["Y_plain"], U=c["U_plain"])


def recovery(c, theta):
    return float(np.abs(theta / c["truth"] - 1.0).max())


_recov = {}


def reference_recovery(oracle, name):
    """(on Y / U, on Y_plain / U_plain): recovery of the reference loop after N_RECOVER steps, and its final states"""
    if name not in _recov:
        c = case(oracle, name)
        out = []
        for d in (c, plain(c)):
            r = run(lambda th, d=d: definition(oracle, d, th), c["theta0"], c["lo"], c["hi"], N_RECOVER, **params(c))
            out.append((recovery(c, r["state"]["theta"]), r["state"]))
        _recov[name] = out
    return _recov[name]


def compared_steps(r):
    """Steps whose every decision lies away from rounding -> their number.  The reference has converged, and later steps are
    not compared, from the first step on which some trajectory's comparison has a margin below MARGIN, or compares two sse
    of which one lies below FLOOR times the sse of theta_0: r_t is a difference of states that agree to about 1e-13 of
    their size once the fit is exact (the rounding of the oracle's xnext), so a residual 1e-10 of the initial one is the
    last that is still signal, and below it either side's sse is its own rounding."""
    n = r["margin"].shape[0]
    for s in range(1, n):
        m = r["margin"][s]
        live = ~np.isnan(m)
        low = np.minimum(r["sse_hist"][s], r["sse_acc"][s - 1]) <= FLOOR * r["sse_hist"][0]
        if np.any(m[live] <= MARGIN) or np.any(low[live]):
            return s
    return n
