"""Lower a (batched) shooting problem to the POD `aslr_problem_desc_t` of include/aslr_to_amd.h.

Pure host logic (numpy + ctypes): no GPU, no torch.  Used by the engine and, in tests, to feed the
same description to the CPU oracle.
"""
import ctypes as C

import numpy as np

from . import _abi


class LoweredProblem(object):
    """Owns the ctypes description and the numpy buffers its pointers refer to."""

    def __init__(self, desc, node_model, x0, frame_ref, nj, nx, nu, dam, nu_user=None, traj_params=None):
        self.desc, self.node_model, self.x0, self.frame_ref = desc, node_model, x0, frame_ref
        # per-trajectory parameter table: dict of the given fields (device-sized, see lower_traj_params), or None
        self.traj_params = traj_params
        # time-varying reference placements: (path [N, B, 12] time-major, row0) as lower_reference_path made it, or None
        self.ref_path = None
        self.nj, self.nx, self.nu, self.dam = nj, nx, nu, dam
        # nu: control size on the device; nu_user: the models' own nu (smaller for a pendulum actuation with one motor
        # command: the lowered controls are padded, models._DifferentialBase.lower)
        self.nu_user = nu if nu_user is None else nu_user
        self.B, self.T = desc.B, desc.T
        self.rec = _abi.record_len(nx, nu)


def lower_reference_path(desc, path, row0=0):
    """Validate a time-varying reference path against a lowered description (the checks aslr_set_reference_path repeats
    on its side, with its messages) and bring it to the device's layout: path [B, N, 12] (row-major R, p) or B lists of N
    SE3 -> C-contiguous float64 [N, B, 12], time-major."""
    B = desc.B
    if len(path) and hasattr(path[0], "__len__") and len(path[0]) and hasattr(path[0][0], "as12"):
        path = [[f.as12() for f in row] for row in path]
    a = np.array(path, dtype=np.float64)
    if a.ndim != 3 or a.shape[0] != B or a.shape[2] != 12:
        raise ValueError("frame_ref_path must have shape [B=%d, n_rows, 12], got %r" % (B, a.shape))
    n_rows = a.shape[1]
    if n_rows < 1:
        raise ValueError("n_rows must be >= 1")
    if not np.all(np.isfinite(a)):
        raise ValueError("frame_ref_path entries must be finite")
    if not 0 <= int(row0) < n_rows:
        raise ValueError("row0 must lie in [0, n_rows)")
    if not any(desc.models[i].costs[c].type == _abi.COST_FRAME_PLACEMENT
               for i in range(desc.nmodels) for c in range(desc.models[i].ncosts)):
        raise ValueError("no model of the problem has a frame-placement cost")
    return np.ascontiguousarray(a.transpose(1, 0, 2))


TRAJ_PARAM_FIELDS = ("stiffness", "motor_inertia", "u_lb", "u_ub")


def lower_traj_params(desc, nj, nu, nu_user, dam, stiffness=None, motor_inertia=None, u_lb=None, u_ub=None, rows=None):
    """Validate a per-trajectory parameter table against a lowered description (the checks aslr_set_trajectory_params
    repeats on its side) and bring it to the device's sizes: -> dict of C-contiguous float64 arrays, stiffness /
    motor_inertia [B, nj] and u_lb / u_ub [B, nu], holding the given fields only; None when no field is given.
    Bounds of width nu_user < nu (one-command pendulum actuation) are padded with the box the models give their padded
    commands, [-1, 1] (models._DifferentialBase.lower): the padded commands stay at zero inside it.
    rows: the number of rows when it is not the shard's B -- the P problems of a pool (Engine.solve_pool)."""
    given = dict(stiffness=stiffness, motor_inertia=motor_inertia, u_lb=u_lb, u_ub=u_ub)
    if all(v is None for v in given.values()):
        return None
    B = desc.B if rows is None else int(rows)
    per = "trajectory" if rows is None else "pool problem"
    models = [desc.models[i] for i in range(desc.nmodels)]
    out = {}
    for name, v in given.items():
        if v is None:
            continue
        a = np.array(v, dtype=np.float64, ndmin=2)
        # accepted widths (the first one is named in the messages) and the width on the device
        widths, width = ((nj,), nj) if name in ("stiffness", "motor_inertia") else ((nu_user, nu), nu)
        if a.ndim != 2 or a.shape[0] != B:
            raise ValueError("%s needs one row per %s ([%d, %d]), got shape %r" % (name, per, B, widths[0], a.shape))
        if a.shape[1] not in widths:
            raise ValueError("%s must have %d entries per %s, got %d" % (name, widths[0], per, a.shape[1]))
        if a.shape[1] < width:
            a = np.concatenate([a, np.full((B, width - a.shape[1]), -1.0 if name == "u_lb" else 1.0)], axis=1)
        out[name] = np.ascontiguousarray(a)
    if "stiffness" in out:
        if dam == _abi.DAM_VSA:
            raise ValueError("a VSA model takes its stiffness from u: no per-trajectory stiffness")
        if not (np.all(np.isfinite(out["stiffness"])) and np.all(out["stiffness"] >= 0.0)):
            raise ValueError("stiffness entries must be finite and >= 0")
    if "motor_inertia" in out and not (np.all(np.isfinite(out["motor_inertia"])) and np.all(out["motor_inertia"] > 0.0)):
        raise ValueError("motor_inertia entries must be finite and > 0")
    if "u_lb" in out or "u_ub" in out:
        limited = [m for m in models if m.has_u_limits]
        if not limited:
            raise ValueError("u_lb / u_ub given, but no action model of the problem has control limits")
        lb = out["u_lb"] if "u_lb" in out else np.array(limited[0].u_lb[:nu])[None]
        ub = out["u_ub"] if "u_ub" in out else np.array(limited[0].u_ub[:nu])[None]
        if not np.all(lb <= ub):  # (also false for NaN)
            raise ValueError("u_lb <= u_ub must hold for every trajectory and control")
    for i, m in enumerate(models):
        for nm in ("K", "B"):
            M = np.array(getattr(m, nm)[:nj * nj]).reshape(nj, nj)
            if np.any(M != np.diag(np.diag(M))):
                raise ValueError("per-trajectory parameters need diagonal K and B: %s of action model %d is not" % (nm, i))
    return out


def param_table(desc, nj, nu, dam, tp, rows):
    """The table the library builds from the fields `tp` (what lower_traj_params returned) for `rows` columns, in the layout
    of region TRAJ_PARAMS and of aslr_pool_params_t.params_dev: float64 [2 nj + 2 nu, rows], row-major -- K, 1 / B (the
    reciprocal formed on the host, as the library forms it), u_lb, u_ub; a field left out repeats the models' constant
    (model 0's K and B, the first limited model's box, zeros without one; K = 0 for VSA).  Host arithmetic only: the
    library lowers the fields itself, this is its statement in numpy for checks and tools."""
    tp = tp or {}
    m0 = desc.models[0]
    limited = [desc.models[i] for i in range(desc.nmodels) if desc.models[i].has_u_limits]
    diag = lambda M: np.array(M[:nj * nj], dtype=np.float64).reshape(nj, nj).diagonal()
    const = dict(stiffness=diag(m0.K), motor_inertia=diag(m0.B),
                 u_lb=np.array(limited[0].u_lb[:nu], dtype=np.float64) if limited else np.zeros(nu),
                 u_ub=np.array(limited[0].u_ub[:nu], dtype=np.float64) if limited else np.zeros(nu))
    col = {k: (np.asarray(tp[k], dtype=np.float64) if k in tp else np.tile(const[k], (rows, 1))) for k in TRAJ_PARAM_FIELDS}
    k = np.zeros((rows, nj)) if dam == _abi.DAM_VSA else col["stiffness"]
    return np.ascontiguousarray(np.concatenate([k, 1.0 / col["motor_inertia"], col["u_lb"], col["u_ub"]], axis=1).T)


def lower_problem(x0s, running_models, terminal_model, frame_refs=None, stiffness=None, motor_inertia=None, u_lb=None,
                  u_ub=None):
    """x0s: [B, nx] (or [nx]); running_models: list of T IntegratedActionModelEulerASR;
    frame_refs: optional [B, 12] (row-major R, p) or list of SE3 overriding every frame-placement
    reference per trajectory; stiffness / motor_inertia [B, nj], u_lb / u_ub [B, nu]: optional per-trajectory
    diagonals of K and B and control boxes (lower_traj_params; LoweredProblem.traj_params)."""
    x0 = np.ascontiguousarray(np.atleast_2d(np.asarray(x0s, dtype=np.float64)))
    B = x0.shape[0]
    T = len(running_models)
    if T < 1:
        raise ValueError("a shooting problem needs at least one running model")
    state = terminal_model.state
    chain_model = state.pinocchio
    nj, nx = chain_model.nv, state.ndx
    if x0.shape[1] != nx:
        raise ValueError("x0 must have %d entries" % nx)
    # distinct models by identity, in order of first appearance
    table, index = [], {}
    node_model = np.zeros(T + 1, dtype=np.int32)
    for t, m in enumerate(list(running_models) + [terminal_model]):
        if m.state.pinocchio is not chain_model:
            raise ValueError("all action models of a problem must share one robot model")
        key = id(m)
        if key not in index:
            if len(table) >= _abi.MAX_MODELS:
                raise ValueError("at most %d distinct action models per problem" % _abi.MAX_MODELS)
            index[key] = len(table)
            table.append(m)
        node_model[t] = index[key]
    nu_user = table[0].nu
    nu = table[0].differential.nu_dev
    dam = table[0].differential.dam
    desc = _abi.ProblemDesc()
    desc.B, desc.T, desc.nmodels = B, T, len(table)
    desc.chain = chain_model.to_struct()
    for i, m in enumerate(table):
        if m.nu != nu_user or m.differential.dam != dam:
            raise ValueError("all action models of a problem must share nu and the actuation kind")
        desc.models[i] = m.lower()
    fr = None
    if frame_refs is not None:
        if len(frame_refs) != B:
            raise ValueError("frame_refs needs one entry per trajectory")
        if hasattr(frame_refs[0], "as12"):
            fr = np.stack([f.as12() for f in frame_refs])
        else:
            fr = np.asarray(frame_refs, dtype=np.float64)
        fr = np.ascontiguousarray(fr.reshape(B, 12))
        desc.frame_ref = fr.ctypes.data_as(C.POINTER(C.c_double))
    desc.node_model = node_model.ctypes.data_as(C.POINTER(C.c_int32))
    desc.x0 = x0.ctypes.data_as(C.POINTER(C.c_double))
    tp = lower_traj_params(desc, nj, nu, nu_user, dam, stiffness, motor_inertia, u_lb, u_ub)
    return LoweredProblem(desc, node_model, x0, fr, nj, nx, nu, dam, nu_user, tp)


def shard_rows(B, rank, world_size):
    """Contiguous block of the batch owned by `rank`: rows [lo, hi)."""
    if not 0 <= rank < world_size:
        raise ValueError("rank out of range")
    base, rem = divmod(B, world_size)
    lo = rank * base + min(rank, rem)
    hi = lo + base + (1 if rank < rem else 0)
    return lo, hi
