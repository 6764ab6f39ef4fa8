"""Shared by tests/test_design_host.py and tests/test_gpu_design.py: the step rule of aslr_design_descent
(include/aslr_to_amd_design.h) in numpy, operation by operation -- every numpy product and sum is rounded on its own, which
is what design_step_kernel does with contraction off, so the two agree bit for bit -- and the loop around it, driven from
the host through a `backend` that solves and differentiates: the CPU oracle here (OracleBackend), the older GPU entry points
in tests/test_gpu_design.py.

Rows are [2 nj][B] like TRAJ_PARAMS: diag K, then diag B.  `active` is a bool per row: the field is optimised."""
import copy

import numpy as np

import _sensitivity as sens
import _traj_oracle
from aslr_to_amd import _abi, scenarios

DEFAULTS = dict(eta0=0.05, grow=2.0, shrink=0.5, c1=1e-4, max_rel=0.25)


def candidate(th, g, eta, max_rel, lo, hi):
    """theta_try from the accepted entries, their gradient and the step length (design_candidate of aslr_design.hip)"""
    with np.errstate(all="ignore"):
        dz = -(eta * (th * g))
        dz = np.where(dz < -max_rel, -max_rel, np.where(dz > max_rel, max_rel, dz))
        t = th * (1.0 + dz)
        return np.where(t < lo, lo, np.where(t > hi, hi, t))


def new_state(theta0, T, nx, nu):
    """what the call starts from: theta_best = theta_0; everything else is written at s = 0"""
    R, B = theta0.shape
    return dict(theta=np.array(theta0, dtype=np.float64), cost=np.zeros(B), g_acc=np.zeros((R, B)), eta=np.zeros(B),
                xs_best=np.zeros((T + 1, B, nx)), us_best=np.zeros((T, B, nu)))


def step(st, s, last, J, grad, xs, us, active, lo, hi, eta0, grow, shrink, c1, max_rel):
    """One launch of design_step_kernel: st (new_state) is updated in place.  J [B], grad [2 nj][B] (rows that are not active
    are not read), xs / us: what XS / US hold.  -> dict(flag [B], hist_f [3][B], theta_try [2 nj][B], table [2 nj][B]: the
    K rows and the RECIPROCAL motor rows the kernel writes into TRAJ_PARAMS (NaN where it writes nothing), xs, us: what XS /
    US hold afterwards, margin [B]: |J - (J_acc + c1 pred)| where the Armijo test decided, NaN elsewhere)"""
    R, B = st["theta"].shape
    act = np.nonzero(np.asarray(active))[0]
    eta_in = np.full(B, eta0) if s == 0 else st["eta"].copy()
    frozen = (eta_in < 0.0) if s > 0 else np.zeros(B, dtype=bool)
    stepped = ~frozen if s > 0 else np.zeros(B, dtype=bool)
    th = st["theta"].copy()
    tt = th.copy()
    evaluable = np.isfinite(J)
    pred = np.zeros(B)
    with np.errstate(all="ignore"):
        for r in act:
            evaluable &= np.isfinite(grad[r])
            c = candidate(th[r], st["g_acc"][r], eta_in, max_rel, lo[r], hi[r])
            tt[r] = np.where(stepped, c, th[r])
            pred = np.where(stepped, pred + st["g_acc"][r] * (tt[r] - th[r]), pred)
        bound = st["cost"] + c1 * pred
        armijo = J <= bound
    accept = evaluable.copy() if s == 0 else (stepped & evaluable & armijo)
    freeze = frozen | ((s == 0) & ~evaluable)
    with np.errstate(all="ignore"):
        eta_out = np.where(freeze, -1.0, eta_in * np.where(accept, grow, shrink))
        margin = np.where(stepped & evaluable, np.abs(J - bound), np.nan)
    flag = np.where(freeze | ~evaluable, -1, np.where(accept, 1, 0)).astype(np.int32)
    hist_f = np.stack([J, np.where(stepped, eta_in, 0.0), pred])
    table = np.full((R, B), np.nan)
    nj = R // 2
    for r in act:
        st["theta"][r] = np.where(accept, tt[r], th[r])
        if s == 0:
            st["g_acc"][r] = np.where(accept, grad[r], 0.0)
        else:
            st["g_acc"][r] = np.where(accept, grad[r], st["g_acc"][r])
        nxt = st["theta"][r] if last else np.where(freeze, st["theta"][r], candidate(st["theta"][r], st["g_acc"][r], eta_out, max_rel, lo[r], hi[r]))
        table[r] = nxt if r < nj else 1.0 / nxt
    to_best = accept | (s == 0)
    st["cost"] = np.where(to_best, J, st["cost"])
    st["eta"] = eta_out
    st["xs_best"] = np.where(to_best[None, :, None], xs, st["xs_best"])
    st["us_best"] = np.where(to_best[None, :, None], us, st["us_best"])
    return dict(flag=flag, hist_f=hist_f, theta_try=tt, table=table, xs=st["xs_best"].copy(), us=st["us_best"].copy(), margin=margin)


def run(backend, theta0, xs0, us0, active, lo, hi, n_steps, first_maxiter, iters_per_step, is_feasible=0, **kw):
    """The loop of aslr_design_descent driven from the host.  backend.solve(theta [2 nj][B], xs, us, iterations, feasible) ->
    (xs, us, J [B]); backend.gradient(theta, xs, us, active) -> [2 nj][B].  -> dict(state: new_state after the last step,
    flag [n][B], hist_f [n][3][B], theta_hist [n][2 nj][B], margin [n][B], xs / us: the plan left in XS / US, table: the last
    table rows written, log: per step (theta_acc, cost, xs_best) before the step, for the invariants of a rejected step)"""
    p = dict(DEFAULTS)
    p.update(kw)
    T, B, nx = xs0.shape[0] - 1, xs0.shape[1], xs0.shape[2]
    st = new_state(theta0, T, nx, us0.shape[2])
    cand, xs, us = np.array(theta0, dtype=np.float64), np.array(xs0), np.array(us0)
    act = np.nonzero(np.asarray(active))[0]
    out = dict(flag=[], hist_f=[], theta_hist=[], margin=[], log=[])
    for s in range(n_steps):
        xs, us, J = backend.solve(cand, xs, us, first_maxiter if s == 0 else iters_per_step, is_feasible if s == 0 else 0)
        grad = backend.gradient(cand, xs, us, active)
        out["log"].append((st["theta"].copy(), st["cost"].copy(), st["xs_best"].copy()))
        last = s == n_steps - 1
        r = step(st, s, last, J, grad, xs, us, active, lo, hi, **p)
        np.testing.assert_array_equal(r["theta_try"], cand)   # the rule recomputes the candidate it was given
        xs, us = r["xs"], r["us"]
        # the next candidate, K and B themselves (the table's motor rows are reciprocals)
        frozen = st["eta"] < 0.0
        for row in act:
            cand[row] = st["theta"][row] if last else np.where(frozen, st["theta"][row], candidate(st["theta"][row], st["g_acc"][row], st["eta"], p["max_rel"], lo[row], hi[row]))
        for k in ("flag", "hist_f", "margin"):
            out[k].append(r[k])
        out["theta_hist"].append(r["theta_try"])
        out["table"] = r["table"]
    for k in ("flag", "hist_f", "theta_hist", "margin"):
        out[k] = np.stack(out[k])
    out.update(state=st, xs=xs, us=us)
    return out


def theta0_of(low):
    """[2 nj][B]: diag K (0 for VSA) and diag B of every trajectory, its table row or the models' constant"""
    K = np.stack([sens.diag(low, b, "K") for b in range(low.B)], axis=1)
    Bm = np.stack([sens.diag(low, b, "B") for b in range(low.B)], axis=1)
    if low.dam == _abi.DAM_VSA:
        K = np.zeros_like(K)
    return np.concatenate([K, Bm])


def with_theta(sc, theta, vsa):
    """scenario sc with the design theta [2 nj][B] as its parameter table (the control box stays the models')"""
    nj = theta.shape[0] // 2
    return dict(sc, traj_params=dict(stiffness=None if vsa else np.ascontiguousarray(theta[:nj].T),
                                     motor_inertia=np.ascontiguousarray(theta[nj:].T), u_lb=None, u_ub=None))


class OracleBackend(object):
    """solves and gradients of the CPU oracle, one B = 1 problem per trajectory (tests/_traj_oracle.py, tests/_sensitivity.py)"""

    def __init__(self, oracle, sc, sp):
        self.oracle, self.sc, self.sp = oracle, sc, copy.copy(sp)
        self.vsa = scenarios.lower(sc).dam == _abi.DAM_VSA

    def low(self, theta):
        return scenarios.lower(with_theta(self.sc, theta, self.vsa))

    def solve(self, theta, xs, us, iterations, feasible):
        low = self.low(theta)
        self.sp.maxiter, self.sp.is_feasible = int(iterations), int(feasible)
        outs = [self.oracle.solve(_traj_oracle.single(low, b), self.sp, xs[:, b:b + 1], us[:, b:b + 1]) for b in range(low.B)]
        return (np.concatenate([o["xs"] for o in outs], axis=1), np.concatenate([o["us"] for o in outs], axis=1),
                np.concatenate([o["traj_f"][_abi.TF_COST] for o in outs]))

    def gradient(self, theta, xs, us, active):
        e = sens.expected(self.oracle, self.low(theta), xs, us)
        nj = theta.shape[0] // 2
        K = e["stiffness"].T if e["stiffness"] is not None else np.zeros((nj, xs.shape[1]))
        return np.concatenate([K, e["motor_inertia"].T])


# ---- the cases of the oracle loop (tests/test_design_host.py picks nothing else; tests/test_gpu_design.py reuses them) ----
# name -> (scenario, B, T, seed, table seed or None, optimised fields, n_steps, first_maxiter, iters_per_step, eta0, max_rel).
# Seeds, iteration counts, eta0 and max_rel were picked on the oracle alone so that every case accepts some step after s = 0 and
# rejects some step (few iterations per step: the plan has not caught up with a large change of the design, the cost rises),
# with every Armijo margin |J - (J_acc + c1 pred)| above 1e-6 |J_acc|.  Smallest margins, relative to |J_acc|, measured
# there: sea_KB 5.5e-3, sea_K 2.2e-3, sea_B 6.1e-5, vsa_B 7.7e-5.  The talos rows serve the GPU bit-for-bit cases only.
CASES = {
    "sea_KB": ("two_dof_sea", 5, 10, 1, 5, "KB", 4, 20, 2, 1.0, 0.5),
    "sea_K": ("two_dof_sea", 5, 10, 1, 5, "K", 4, 20, 2, 1.0, 0.5),
    "sea_B": ("two_dof_sea", 5, 10, 1, 5, "B", 4, 20, 2, 1.0, 0.5),
    "vsa_B": ("two_dof_vsa_boxddp", 3, 10, 1, None, "B", 3, 20, 6, 0.2, 0.5),
    "talos_sea_KB": ("talos_arm_sea", 2, 5, 1, 5, "KB", 3, 6, 2, 1.0, 0.5),
    "talos_vsa_B": ("talos_arm_vsa", 2, 4, 1, None, "B", 3, 6, 2, 1.0, 0.5),
}
ORACLE_CASES = ("sea_KB", "sea_K", "sea_B", "vsa_B")
MARGIN = 1e-6


def case(name):
    scen, B, T, seed, tseed, fields, n, first, per, eta0, max_rel = CASES[name]
    sc = scenarios.SCENARIOS[scen](B=B, T=T, seed=seed)
    if tseed is not None:
        sc = scenarios.with_traj_params(sc, seed=tseed)
    low = scenarios.lower(sc)
    sp = scenarios.solver_params(sc)
    nj = low.nj
    active = np.array([("K" in fields)] * nj + [("B" in fields)] * nj)
    th0 = theta0_of(low)
    lo, hi = np.where(th0 > 0, th0 / 3.0, 1.0), np.where(th0 > 0, th0 * 3.0, 1.0)
    # bounds: a factor of 3 either way around the initial design (rows of a VSA model's K, which is 0, are never read)
    return dict(sc=sc, low=low, sp=sp, active=active, theta0=th0, lo=lo, hi=hi, n_steps=n, first_maxiter=first,
                iters_per_step=per, eta0=eta0, max_rel=max_rel, fields=fields)
