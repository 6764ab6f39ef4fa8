"""Shared by tests/test_ref_path_host.py and tests/test_gpu_ref_path.py: what the CPU oracle says about a problem with
time-varying reference placements (aslr_set_reference_path), without changing the oracle.

 - one knot: oracle.knot(low, mi, x, u, frame_ref=row) evaluates a knot against a given reference, so a sweep over a path
   is that call per (t, b) with row min(row0 + t, n_rows - 1);
 - a full solve: a path that holds four via-points (scenarios.hold_via_points: three running segments and the terminal
   node) is exactly a B = 1 problem with four distinct action models whose frame-placement `ref`s are the four rows and no
   frame_ref table -- built here the way tests/_traj_oracle.single copies a description.

Paths are time-major [n_rows, B, 12] here (the device's layout, lowering.lower_reference_path)."""
import ctypes as C

import numpy as np

import _traj_oracle
from aslr_to_amd import _abi, scenarios
from aslr_to_amd.lowering import LoweredProblem

SCENARIOS = {"sea2": scenarios.two_dof_sea, "vsa2": scenarios.two_dof_vsa_boxddp, "sea7": scenarios.talos_arm_sea}


def rot_z(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def random_path(sc, n_rows, seed):
    """[B, n_rows, 12]: per trajectory and row, the scenario's own target moved by U(-0.03, 0.03) in x and y and turned about
    z by U(-0.3, 0.3)"""
    refs = np.asarray(sc["frame_refs"], dtype=np.float64).reshape(-1, 12)
    rng = np.random.default_rng(seed)
    B = refs.shape[0]
    path = np.repeat(refs[:, None, :], n_rows, axis=1)
    path[:, :, 9:11] += rng.uniform(-0.03, 0.03, (B, n_rows, 2))
    ang = rng.uniform(-0.3, 0.3, (B, n_rows))
    for b in range(B):
        for i in range(n_rows):
            path[b, i, :9] = (rot_z(ang[b, i]) @ path[b, i, :9].reshape(3, 3)).reshape(9)
    return path


def row_of(t, row0, n_rows):
    return min(row0 + t, n_rows - 1)


def sweep(oracle, low, xs, us, path_tm, row0, diff=True):
    """calc / calcDiff of every knot against its row of the path -> xnext [T+1, B, nx], cost [T+1, B], deriv [T+1, B, rec]
    (None without diff).  With a parameter table on `low` the knot of trajectory b is evaluated with that trajectory's models
    (tests/_traj_oracle.single)."""
    T, B = low.T, low.B
    xnext, cost = np.zeros((T + 1, B, low.nx)), np.zeros((T + 1, B))
    deriv = np.zeros((T + 1, B, low.rec)) if diff else None
    for b in range(B):
        lb = _traj_oracle.single(low, b) if low.traj_params else low
        for t in range(T + 1):
            k = oracle.knot(lb, int(low.node_model[t]), xs[t, b], us[t, b] if t < T else None,
                            frame_ref=path_tm[row_of(t, row0, path_tm.shape[0]), b], diff=diff)
            xnext[t, b], cost[t, b] = k["xnext"], k["cost"]
            if diff:
                deriv[t, b] = k["rec"]
    return xnext, cost, deriv


def trial_cost(oracle, low, xs_try, us_try, path_tm, row0):
    """cost of one candidate [T+1, B, nx], [T, B, nu]: its knot costs against their rows, summed in knot order -> [B]"""
    c = sweep(oracle, low, xs_try, us_try, path_tm, row0, diff=False)[1]
    total = np.zeros(low.B)
    for t in range(low.T + 1):
        total = total + c[t]
    return total


def _set_placement_refs(model, row):
    n = 0
    for c in range(model.ncosts):
        if model.costs[c].type == _abi.COST_FRAME_PLACEMENT:
            for i in range(12):
                model.costs[c].ref[i] = row[i]
            n += 1
    return n


def four_models(low, via, rows=None):
    """The problem of `low` (one running model, one terminal model) with the via-points written into FOUR action models:
    models 0..2 are the running model with rows 0..2 as their frame-placement references, model 3 the terminal model with
    row 3; node t uses the model of its segment; no frame_ref table.  via: [4, 12] shared by the trajectories `rows`
    (default: all) -> a LoweredProblem of those trajectories."""
    assert low.desc.nmodels == 2 and (np.asarray(low.node_model[:-1]) == 0).all() and low.node_model[-1] == 1
    rows = range(low.B) if rows is None else rows
    desc = _abi.ProblemDesc()
    C.memmove(C.byref(desc), C.byref(low.desc), C.sizeof(desc))
    desc.nmodels = 4
    for i in range(4):
        desc.models[i] = low.desc.models[0 if i < 3 else 1]
        assert _set_placement_refs(desc.models[i], via[i]) >= 1
    T = low.T
    node_model = np.searchsorted([T // 3, 2 * T // 3, T], np.arange(T + 1), side="right").astype(np.int32)
    x0 = np.ascontiguousarray(low.x0[list(rows)])
    desc.B = x0.shape[0]
    desc.node_model = node_model.ctypes.data_as(C.POINTER(C.c_int32))
    desc.x0 = x0.ctypes.data_as(C.POINTER(C.c_double))
    desc.frame_ref = None
    return LoweredProblem(desc, node_model, x0, None, low.nj, low.nx, low.nu, low.dam, low.nu_user)


def solve(oracle, low, via, sp, log_cap=0):
    """the oracle's solve of every trajectory b against its own via-points via[b] ([B, 4, 12]), one four-model B = 1 problem
    each -> the dict tests/_traj_oracle.solve returns"""
    outs = [oracle.solve(four_models(low, via[b], [b]), sp, log_cap=log_cap) for b in range(low.B)]
    out = {k: np.concatenate([o[k] for o in outs], axis=1) for k in ("xs", "us", "traj_f", "traj_i")}
    if log_cap:
        out["log"] = np.concatenate([o["log"] for o in outs], axis=2)
    return out


# the full-solve cases: scenario seed 5, via-points from scenarios.reference_via_points(seed=11), the scenarios' own solver,
# maxiter and th_stop
FULL_SOLVE_CASES = {"two_dof_sea": ("sea2", 16, 30), "two_dof_vsa_boxddp": ("vsa2", 16, 30), "talos_arm_sea": ("sea7", 8, 12)}


def full_solve_case(name):
    """-> scenario (without the path), its via-points [B, 4, 12], solver parameters"""
    key, B, T = FULL_SOLVE_CASES[name]
    sc = SCENARIOS[key](B=B, T=T, seed=5)
    return sc, scenarios.reference_via_points(sc, seed=11), scenarios.solver_params(sc)


def with_path(sc, path, row0=0):
    out = dict(sc)
    out["ref_path"], out["ref_row0"] = path, row0
    return out
