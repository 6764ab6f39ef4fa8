"""Shared by tests/test_policy_host.py and tests/test_gpu_policy.py: what the CPU oracle says about aslr_policy_rollout
(include/aslr_to_amd_policy.h), without changing the oracle.

 - rollout(): the definition as a numpy loop over oracle.knot on the B = 1 problem of trajectory b whose models carry that
   SAMPLE's plant K and B (built the way tests/_traj_oracle.single builds a trajectory's): x_0 = X0[b] + dx0,
   u_t = us_t - K_t (x_t - xs_t), clamped to the knot's box when asked, x_{t+1} = xnext + w_t, costs summed in knot order.
   It takes xs, us and K as inputs: the GPU tests pass the device's own gains, so that only the roll-out is compared.
 - case(): the seeded inputs of the GPU cases -- scenario, candidate, perturbations within the issue's ranges.

Everything is time-major going in (the oracle's layout) and batch-major coming out, like Engine.policy_rollout:
cost [B, S], failed_knot [B, S], x_final [B, S, nx], xs [B, S, T+1, nx], us [B, S, T, nu]."""
import numpy as np

import _ref_path
import _traj_oracle
from _gpu_case import relerr  # noqa: F401 (pol.relerr of the host suites)
from aslr_to_amd import _abi, scenarios

# (scenario, table, path, B, S, T, 3-D chain, clamp): the shapes are the smallest that leave a partial wave of teams (B = 5:
# 4 per wave) and a sample group with one live lane (S = 17: 16 per group), the smallest problem there is, and full ones
CASES = {
    "sea_table": ("two_dof_sea", True, False, 5, 17, 5, False, False),
    "sea_plain": ("two_dof_sea", False, False, 5, 17, 5, False, False),
    "sea_path": ("two_dof_sea", True, True, 5, 17, 5, False, False),
    "sea_one": ("two_dof_sea", False, False, 1, 1, 1, False, False),
    "sea_full": ("two_dof_sea", False, False, 4, 16, 3, False, False),
    "vsa_box": ("two_dof_vsa_boxddp", True, False, 5, 17, 5, False, True),
    "pendulum_3d": ("double_pendulum", False, False, 5, 3, 3, True, False),
    "pendulum_nu1_3d": ("double_pendulum_nu1", False, False, 5, 3, 3, True, False),
}
# the narrowed box of vsa_box (torques, stiffnesses): the seeded candidate draws torques from U(-1, 1) and stiffnesses from
# U(0.1, 5) and is clipped to it, so the feedback term pushes some controls of some samples out of it
BOX_LB, BOX_UB = (-0.9, -0.9, 0.3, 0.3), (0.9, 0.9, 4.5, 4.5)
XREG = 1e-3  # regularisation of the one backward sweep the gains come from


def scenario(name, B, T, table, path):
    if name.startswith("double_pendulum"):
        sc = scenarios.SCENARIOS[name](T=T)
        sc["x0"] = np.asarray(sc["x0"]) + np.random.default_rng(2).uniform(-0.3, 0.3, (B, 8))
    else:
        sc = scenarios.SCENARIOS[name](B=B, T=T, seed=4)
    if table:
        sc = scenarios.with_traj_params(sc, seed=5)
        if name == "two_dof_vsa_boxddp":
            sc["traj_params"]["u_lb"] = np.tile(np.array(BOX_LB), (B, 1))
            sc["traj_params"]["u_ub"] = np.tile(np.array(BOX_UB), (B, 1))
    if path:  # 4 rows from row 2 on: knots 0 and 1 read rows 2 and 3, the others hold the last row
        sc = _ref_path.with_path(sc, _ref_path.random_path(sc, 4, 13), row0=2)
    return sc


def nominal_diag(low, b, field):
    """diagonal of K or B of trajectory b (its row of the table, else the constant of model 0)"""
    m = _traj_oracle.single(low, b).desc.models[0]
    return np.array([getattr(m, field)[j * low.nj + j] for j in range(low.nj)])


def perturbations(low, S, seed, stiffness=True):
    """seeded, batch-major: plant K and B within +-30 % of the trajectory's nominal, |dx0| <= 1e-2, |w| <= 1e-3"""
    rng = np.random.default_rng(seed)
    B, T, nx, nj = low.B, low.T, low.nx, low.nj
    kn = np.array([nominal_diag(low, b, "K") for b in range(B)])[:, None, :]
    bn = np.array([nominal_diag(low, b, "B") for b in range(B)])[:, None, :]
    out = dict(plant_stiffness=kn * rng.uniform(0.7, 1.3, (B, S, nj)), plant_motor_inertia=bn * rng.uniform(0.7, 1.3, (B, S, nj)),
               dx0=rng.uniform(-1e-2, 1e-2, (B, S, nx)), disturbance=rng.uniform(-1e-3, 1e-3, (B, S, T, nx)))
    if low.dam == _abi.DAM_VSA or not stiffness:
        out["plant_stiffness"] = None
    return out


def case(oracle, key):
    """-> dict(sc, low, xs, us, pert, S, clamp, three_d, sp): the candidate is seeded controls (gc.random_candidate's recipe
    for us, seed 3, clipped to the narrowed box where there is one) and the oracle's open-loop roll-out of them from x0, so
    that the closed loop starts on its reference and x - xs is of the size of the perturbations"""
    name, table, path, B, S, T, three_d, clamp = CASES[key]
    sc = scenario(name, B, T, table, path)
    low = scenarios.lower(sc)
    rng = np.random.default_rng(3)
    us = rng.uniform(-1.0, 1.0, (T, B, low.nu))
    if low.dam == _abi.DAM_VSA:
        us[..., low.nu // 2:] = rng.uniform(0.1, 5.0, (T, B, low.nu // 2))
        us = np.clip(us, BOX_LB, BOX_UB)
    if low.nu_user < low.nu:
        us[..., low.nu_user:] = 0.0   # padded commands
    zx, zk = np.zeros((T + 1, low.nx)), np.zeros((T, low.nu, low.nx))
    xs = np.stack([rollout_one(oracle, low, b, zx, us[:, b], zk)["xs"] for b in range(B)], axis=1)
    return dict(sc=sc, low=low, xs=xs, us=us, pert=perturbations(low, S, 17), S=S, clamp=clamp, three_d=three_d,
                sp=scenarios.solver_params(sc))


def oracle_gains(oracle, low, sp, xs, us):
    """K [T, B, nu, nx] of one calcDiff + backward sweep of the oracle on the candidate (XREG, feasible); with a table or a
    path through the per-trajectory loops of the other suites"""
    path = getattr(low, "ref_path", None)
    if path is not None:
        deriv = _ref_path.sweep(oracle, low, xs, us, path[0], path[1])[2]
    elif low.traj_params:
        deriv = _traj_oracle.calc_diff(oracle, low, xs, us)[2]
    else:
        deriv = oracle.calc_diff(low, xs, us)[2]
    gaps = np.zeros((low.T + 1, low.B, low.nx))
    if low.traj_params:
        out = _traj_oracle.backward_pass(oracle, low, sp, deriv, gaps, us, XREG, 1, np.zeros((low.T, low.B, low.nu)))
    else:
        out = oracle.backward_pass(low, sp, deriv, gaps, us, XREG, 1)
    assert not np.asarray(out["fail"]).any(), "the oracle's backward sweep failed on the seeded candidate"
    return out["K"]


def plant_problem(low, b, k=None, bm=None):
    """B = 1 problem of trajectory b whose every model carries the plant's diagonals (None: the trajectory's own)"""
    lb = _traj_oracle.single(low, b)
    nj = low.nj
    for i in range(lb.desc.nmodels):
        for j in range(nj):
            if k is not None:
                lb.desc.models[i].K[j * nj + j] = k[j]
            if bm is not None:
                lb.desc.models[i].B[j * nj + j] = bm[j]
    return lb


def bad(v):
    v = np.abs(np.asarray(v))
    return bool((~np.isfinite(v)).any() or (v >= 1e30).any())


def rollout_one(oracle, low, b, xs, us, K, k=None, bm=None, dx0=None, w=None, clamp=False, x0=None):
    """one sample of trajectory b: xs [T+1, nx], us [T, nu], K [T, nu, nx] -> dict(cost, failed_knot, xs, us, bound: some
    control was moved by the clamp)"""
    T = low.T
    lb = plant_problem(low, b, k, bm)
    path = getattr(low, "ref_path", None)
    ref = lambda t: (path[0][_ref_path.row_of(t, path[1], path[0].shape[0]), b] if path is not None
                     else None if low.frame_ref is None else low.frame_ref[b])
    x = np.array(low.x0[b] if x0 is None else x0, dtype=np.float64)
    if dx0 is not None:
        x = x + dx0
    X, U = np.zeros((T + 1, low.nx)), np.zeros((T, low.nu))
    cost, failed, bound = 0.0, -1, False
    for t in range(T):
        X[t] = x
        mi = int(low.node_model[t])
        u = us[t] - K[t] @ (x - xs[t])
        m = lb.desc.models[mi]
        if clamp and m.has_u_limits:
            uc = np.clip(u, np.array(m.u_lb[:low.nu]), np.array(m.u_ub[:low.nu]))
            bound = bound or bool((uc != u).any())
            u = uc
        U[t] = u
        kn = oracle.knot(lb, mi, x, u, frame_ref=ref(t), diff=False)
        cost = cost + kn["cost"]
        if failed < 0 and bad(kn["xnext"]):
            failed = t
        x = kn["xnext"] if w is None else kn["xnext"] + w[t]
    X[T] = x
    cost = cost + oracle.knot(lb, int(low.node_model[T]), x, None, frame_ref=ref(T), diff=False)["cost"]
    return dict(cost=np.nan if failed >= 0 else cost, failed_knot=failed, xs=X, us=U, bound=bound)


def rollout(oracle, low, xs, us, K, S, plant_stiffness=None, plant_motor_inertia=None, dx0=None, disturbance=None,
            clamp=False):
    """every sample of every trajectory; xs [T+1, B, nx], us [T, B, nu], K [T, B, nu, nx] time-major, perturbations
    batch-major -> batch-major dict(cost, failed_knot, x_final, xs, us, bound)"""
    B, T = low.B, low.T
    out = dict(cost=np.zeros((B, S)), failed_knot=np.zeros((B, S), dtype=np.int32), x_final=np.zeros((B, S, low.nx)),
               xs=np.zeros((B, S, T + 1, low.nx)), us=np.zeros((B, S, T, low.nu)), bound=np.zeros((B, S), dtype=bool))
    pick = lambda a, b, s: None if a is None else a[b, s]
    for b in range(B):
        for s in range(S):
            r = rollout_one(oracle, low, b, xs[:, b], us[:, b], K[:, b], pick(plant_stiffness, b, s),
                            pick(plant_motor_inertia, b, s), pick(dx0, b, s), pick(disturbance, b, s), clamp)
            out["cost"][b, s], out["failed_knot"][b, s], out["bound"][b, s] = r["cost"], r["failed_knot"], r["bound"]
            out["xs"][b, s], out["us"][b, s], out["x_final"][b, s] = r["xs"], r["us"], r["xs"][T]
    return out


OUTPUTS = ("cost", "x_final", "xs", "us")
