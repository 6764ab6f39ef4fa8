"""Shared by tests/test_plant_sens_host.py and tests/test_gpu_plant_sens.py: what the CPU oracle says about
aslr_policy_plant_sensitivity (include/aslr_to_amd_plant_sens.h), without changing the oracle.

 - expected(): the DEFINITION in numpy with full matrices on the oracle's records (the sweeps of tests/_covariance.records)
   and a given K, about the candidate (xs, us):
     S_0 = 0,   S_{t+1} = (Fx_t - Fu_t K_t) S_t + G_t,   V_t = K_t S_t                     (S_t = dx_t/dtheta, du_t/dtheta = -V_t)
     dJ/dtheta_p = sum_{t<T} (Lx_t^T S_t[:, p] - Lu_t^T V_t[:, p]) + Lx_T^T S_T[:, p]
     x_var_t[i] = sum_p S_t[i, p]^2 var_p,   u_var_t[k] = sum_p V_t[k, p]^2 var_p
   with theta = (diag K, diag B) of the trajectory (its row of the table, else the constants of the knot's model) and G_t the
   explicit parameter derivative of the step in the closed forms of the adjoint sweep:
     G_K[:, j] = -(delta_j / K_j) (Fx_t[:, nj+j] - e_{nj+j}),   delta_j = xs_t[j] - xs_t[nj+j]
     G_B[:, j] = -(1 / B_j) D_j (dt e_{nj+j} + e_{3nj+j}),      D_j = xnext_t[3nj+j] - xs_t[3nj+j].
   It takes xs, us and K as inputs: the GPU tests pass the device's own gains, so that only this sweep is compared.
 - fd_rollout(): central differences of the nonlinear closed loop of tests/_policy.rollout_one (no clamp) on plants with
   theta_p (1 +- h): the independent check of the definition, closed forms included.
 - variances(): seeded var ~ U(0.1, 1) relative to theta^2, so that x_var and u_var are of the order of (theta dx/dtheta)^2.

Cases are the shapes of tests/_covariance.CASES.  Everything is time-major going in (the oracle's layout) and batch-major
coming out, like Engine.policy_plant_sensitivity: dx [B, T+1, nx, nj], dx_final [B, nx, nj], dcost [B, nj], x_var
[B, T+1, nx], u_var [B, T, nu] (the device's nu), V [B, T, nu, np]; the stiffness fields are None for a VSA model."""
import numpy as np

import _covariance as cv
import _policy as pol
import _ref_path
import _sensitivity as sens
import _traj_oracle
from aslr_to_amd import _abi

CASES = cv.CASES
KINDS = ("stiffness", "motor_inertia")
OUTPUTS = ("dx_dstiffness", "dx_dmotor_inertia", "dxT_dstiffness", "dxT_dmotor_inertia", "dcost_dstiffness",
           "dcost_dmotor_inertia", "x_var", "u_var")

# tests/test_plant_sens_host.py, the definition against central differences of the nonlinear closed loop with the oracle's
# gains, per case: (relative step h, disagreement measured at h, at h / 2) on the oracle alone, worst of S_T, V and dJ/dtheta
# in the measure cv.traj_relerr; the bound of a test is ten times the value (how they were measured: the test's docstring)
FD = {
    "sea": (1e-4, 2.58e-7, 6.41e-8),
    "vsa_box": (1e-4, 4.29e-7, 1.08e-7),
    "arm_sea": (1e-4, 2.46e-8, 1.04e-8),
    "arm_vsa": (1e-4, 2.67e-8, 6.67e-9),
}


def sweep(oracle, low, xs, us):
    """(xnext, cost, deriv) of the candidate through the sweep that honours what the problem has set (cv.records's choice)"""
    path = getattr(low, "ref_path", None)
    if path is not None:
        return _ref_path.sweep(oracle, low, xs, us, path[0], path[1])
    if low.traj_params:
        return _traj_oracle.calc_diff(oracle, low, xs, us)
    return oracle.calc_diff(low, xs, us)


def has_stiffness(low):
    return low.dam == _abi.DAM_SEA


def theta(low, b, mi=0):
    """(diag K or None, diag B) of trajectory b on model mi"""
    return (sens.diag(low, b, "K", mi) if has_stiffness(low) else None), sens.diag(low, b, "B", mi)


def variances(low, seed):
    """seeded, batch-major (stiffness_var or None, motor_inertia_var) [B, nj]: (theta sqrt(U(0.1, 1)))^2"""
    rng = np.random.default_rng(seed)
    out = []
    for kind in range(2):
        r = rng.uniform(0.1, 1.0, (low.B, low.nj))
        th = np.array([theta(low, b)[kind] if theta(low, b)[kind] is not None else np.zeros(low.nj) for b in range(low.B)])
        out.append(r * th * th)
    return (out[0] if has_stiffness(low) else None), out[1]


def explicit(low, b, t, Fx, xs_t, xnext_t):
    """G_t [nx, np] of trajectory b at knot t from the closed forms; columns: stiffness (SEA only), then motor inertia"""
    nx, nj = low.nx, low.nj
    mi = int(low.node_model[t])
    k, bm = theta(low, b, mi)
    dt = float(low.desc.models[mi].dt)
    cols = []
    if k is not None:
        for j in range(nj):
            e = np.zeros(nx)
            e[nj + j] = 1.0
            cols.append(-((xs_t[j] - xs_t[nj + j]) / k[j]) * (Fx[:, nj + j] - e))
    for j in range(nj):
        e = np.zeros(nx)
        e[nj + j], e[3 * nj + j] = dt, 1.0
        cols.append(-(1.0 / bm[j]) * (xnext_t[3 * nj + j] - xs_t[3 * nj + j]) * e)
    return np.stack(cols, axis=1)


def propagate(low, xs, xnext, deriv, K, stiffness_var=None, motor_inertia_var=None):
    """the definition on given records; variances batch-major [B, nj], None = 0"""
    T, B, nx, nu, nj = low.T, low.B, low.nx, low.nu, low.nj
    sea = has_stiffness(low)
    npar = 2 * nj if sea else nj
    o = _abi.record_offsets(nx, nu)
    blk = cv.blocks(low, deriv)
    Lx, Lu = deriv[:, :, o["Lx"]:o["Lx"] + nx], deriv[:, :, o["Lu"]:o["Lu"] + nu]
    S = np.zeros((B, T + 1, nx, npar))
    V = np.zeros((B, T, nu, npar))
    dJ = np.zeros((B, npar))
    var = np.zeros((B, npar))
    if sea and stiffness_var is not None:
        var[:, :nj] = stiffness_var
    if motor_inertia_var is not None:
        var[:, npar - nj:] = motor_inertia_var
    for b in range(B):
        for t in range(T):
            Kt, Fx, Fu = K[t, b], blk["Fx"][t, b], blk["Fu"][t, b]
            V[b, t] = Kt @ S[b, t]
            dJ[b] += Lx[t, b] @ S[b, t] - Lu[t, b] @ V[b, t]
            S[b, t + 1] = (Fx - Fu @ Kt) @ S[b, t] + explicit(low, b, t, Fx, xs[t, b], xnext[t, b])
        dJ[b] += Lx[T, b] @ S[b, T]
    out = dict(V=V, x_var=np.einsum("btip,bp->bti", S * S, var), u_var=np.einsum("btkp,bp->btk", V * V, var))
    m0 = npar - nj
    out["dx_dmotor_inertia"], out["dcost_dmotor_inertia"] = S[..., m0:].copy(), dJ[:, m0:].copy()
    out["dx_dstiffness"], out["dcost_dstiffness"] = (S[..., :nj].copy(), dJ[:, :nj].copy()) if sea else (None, None)
    for kind in KINDS:
        d = out["dx_d" + kind]
        out["dxT_d" + kind] = None if d is None else d[:, T].copy()
    return out


def expected(oracle, low, xs, us, K, stiffness_var=None, motor_inertia_var=None):
    xnext, _, deriv = sweep(oracle, low, xs, us)
    return propagate(low, xs, xnext, deriv, K, stiffness_var, motor_inertia_var)


def fd_rollout(oracle, low, xs, us, K, h):
    """central differences of pol.rollout_one (clamp off) with plant theta_p (1 +- h), parameter by parameter -> the layout
    of propagate(): dxT_d*, dcost_d* and V (= -du/dtheta; columns: stiffness where there is one, then motor inertia)"""
    T, B, nx, nu, nj = low.T, low.B, low.nx, low.nu, low.nj
    sea = has_stiffness(low)
    npar = 2 * nj if sea else nj
    ST, V, dJ = np.zeros((B, nx, npar)), np.zeros((B, T, nu, npar)), np.zeros((B, npar))
    for b in range(B):
        k0, b0 = pol.nominal_diag(low, b, "K"), pol.nominal_diag(low, b, "B")
        for p in range(npar):
            runs = []
            for sgn in (1.0, -1.0):
                k, bm = k0.copy(), b0.copy()
                if sea and p < nj:
                    k[p] *= 1.0 + sgn * h
                else:
                    bm[p - (npar - nj)] *= 1.0 + sgn * h
                runs.append(pol.rollout_one(oracle, low, b, xs[:, b], us[:, b], K[:, b], k=k if sea else None, bm=bm, clamp=False))
            step = 2.0 * h * (k0[p] if sea and p < nj else b0[p - (npar - nj)])
            assert runs[0]["failed_knot"] < 0 and runs[1]["failed_knot"] < 0
            ST[b, :, p] = (runs[0]["xs"][T] - runs[1]["xs"][T]) / step
            V[b, :, :, p] = -(runs[0]["us"] - runs[1]["us"]) / step
            dJ[b, p] = (runs[0]["cost"] - runs[1]["cost"]) / step
    m0 = npar - nj
    return dict(V=V, dxT_dmotor_inertia=ST[..., m0:].copy(), dcost_dmotor_inertia=dJ[:, m0:].copy(),
                dxT_dstiffness=ST[..., :nj].copy() if sea else None, dcost_dstiffness=dJ[:, :nj].copy() if sea else None)


FD_OUTPUTS = ("V", "dxT_dstiffness", "dxT_dmotor_inertia", "dcost_dstiffness", "dcost_dmotor_inertia")


def fd_disagreement(oracle, low, xs, us, K, h):
    """worst over FD_OUTPUTS of cv.traj_relerr(definition, central differences at relative step h)"""
    want = expected(oracle, low, xs, us, K)
    got = fd_rollout(oracle, low, xs, us, K, h)
    return max(cv.traj_relerr(want[k], got[k]) for k in FD_OUTPUTS if want[k] is not None)
