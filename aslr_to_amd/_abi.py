"""ctypes mirror of include/aslr_to_amd.h and the loader of the HIP shared library.

The product path has NO CPU fallback: if ``csrc/libaslr_to_hip.so`` is missing or cannot be
loaded, importing the compute path raises.  (The CPU restatement under ``oracle/`` is test
infrastructure and is never imported from here.)
"""
import ctypes as C
import os

MAX_NJ = 7
MAX_NX = 28
MAX_NU = 14
MAX_COSTS = 6
MAX_MODELS = 4
NALPHA = 10
ABI_VERSION = 5

OK, E_INVALID, E_HIP, E_NODEVICE, E_WORKSPACE = 0, -1, -2, -3, -4
DAM_SEA, DAM_VSA = 0, 1
COST_FRAME_PLACEMENT, COST_STATE, COST_CONTROL, COST_PENDULUM, COST_STIFFNESS = range(5)
SOLVER_DDP, SOLVER_FDDP, SOLVER_BOXDDP = 0, 1, 2
ST_CONVERGED, ST_REG_MAX, ST_BACKWARD_ERR, ST_FORWARD_ERR = 1, 2, 4, 8

(R_XS, R_US, R_XNEXT, R_COST, R_DERIV, R_GAPS, R_KGAIN, R_KFF, R_QU, R_VX, R_VXX, R_XS_TRY,
 R_US_TRY, R_TRAJ_F, R_TRAJ_I, R_X0, R_FRAME_REF, R_VXXF, R_DESC, R_NODE_MODEL, R_COST_TRY, R_DYN, R_POOL_SAVE,
 R_TRAJ_PARAMS, R_COUNT) = range(25)

(TF_COST, TF_STOP, TF_XREG, TF_D1, TF_D2, TF_STEP, TF_DV, TF_DVEXP, TF_DG, TF_DQ,
 TF_COST_TRY0) = range(11)
TF_DVTRY0 = TF_COST_TRY0 + NALPHA
TF_COUNT = TF_DVTRY0 + NALPHA
(TI_ITER, TI_STATUS, TI_FEASIBLE, TI_WAS_FEASIBLE, TI_RECALC, TI_ACCEPTED, TI_DONE, TI_NTRIALS,
 TI_GAPFLAG, TI_TRYFAIL0) = range(10)
TI_COUNT = TI_TRYFAIL0 + NALPHA

# rows of the per-iteration log (aslr_set_iteration_log)
(LOG_COST, LOG_STOP, LOG_XREG, LOG_STEP, LOG_D1, LOG_D2, LOG_DV, LOG_DVEXP, LOG_ACCEPTED, LOG_STATUS, LOG_FEASIBLE,
 LOG_COUNT) = range(12)

_d = C.c_double
_i = C.c_int32


class Chain(C.Structure):
    _fields_ = [("nj", _i), ("_pad0", _i), ("gravity", _d * 3),
                ("joint_R", (_d * 9) * MAX_NJ), ("joint_p", (_d * 3) * MAX_NJ),
                ("axis", (_d * 3) * MAX_NJ), ("mass", _d * MAX_NJ), ("com", (_d * 3) * MAX_NJ),
                ("inertia", (_d * 9) * MAX_NJ)]


class Cost(C.Structure):
    _fields_ = [("type", _i), ("frame_joint", _i), ("weight", _d), ("act_w", _d * MAX_NX),
                ("ref", _d * MAX_NX), ("frame_R", _d * 9), ("frame_p", _d * 3), ("lambda_", _d)]


class Model(C.Structure):
    _fields_ = [("dam", _i), ("nu", _i), ("ncosts", _i), ("has_u_limits", _i), ("dt", _d),
                ("K", _d * (MAX_NJ * MAX_NJ)), ("B", _d * (MAX_NJ * MAX_NJ)),
                ("S", _d * (MAX_NJ * MAX_NJ)), ("u_lb", _d * MAX_NU), ("u_ub", _d * MAX_NU),
                ("costs", Cost * MAX_COSTS)]


class ProblemDesc(C.Structure):
    _fields_ = [("B", _i), ("T", _i), ("nmodels", _i), ("_pad0", _i), ("chain", Chain),
                ("models", Model * MAX_MODELS), ("node_model", C.POINTER(_i)),
                ("x0", C.POINTER(_d)), ("frame_ref", C.POINTER(_d))]


class SolverParams(C.Structure):
    _fields_ = [("solver", _i), ("maxiter", _i), ("is_feasible", _i), ("fixed_iterations", _i),
                ("reg_init", _d), ("th_stop", _d), ("th_grad", _d), ("th_gaptol", _d),
                ("th_stepdec", _d), ("th_stepinc", _d), ("th_acceptstep", _d),
                ("th_acceptnegstep", _d), ("reg_min", _d), ("reg_max", _d),
                ("reg_incfactor", _d), ("reg_decfactor", _d), ("boxqp_maxiter", _i),
                ("_pad0", _i), ("boxqp_th_acceptstep", _d), ("boxqp_th_grad", _d),
                ("boxqp_reg", _d)]


class Pool(C.Structure):
    """aslr_pool_t: device pointers of a pool solve (aslr_solve_pool)."""
    _fields_ = [("P", _i), ("_pad0", _i), ("x0", C.c_void_p), ("frame_ref", C.c_void_p), ("xs_out", C.c_void_p),
                ("us_out", C.c_void_p), ("stat_f", C.c_void_p), ("stat_i", C.c_void_p), ("slot_problem", C.c_void_p),
                ("counters", C.c_void_p), ("xs_init", C.c_void_p), ("us_init", C.c_void_p)]


class TrajParams(C.Structure):
    """aslr_traj_params_t: nullable HOST pointers of a per-trajectory parameter table (aslr_set_trajectory_params)."""
    _fields_ = [("stiffness", C.POINTER(_d)), ("motor_inertia", C.POINTER(_d)), ("u_lb", C.POINTER(_d)),
                ("u_ub", C.POINTER(_d))]


class PoolParams(C.Structure):
    """aslr_pool_params_t (include/aslr_to_amd_pool_params.h): nullable HOST tables [P][nj] / [P][nu] with one row per pool
    problem, and the DEVICE scratch [2 nj + 2 nu][P] the call uploads the lowered table to (aslr_solve_pool_params)."""
    _fields_ = [("stiffness", C.POINTER(_d)), ("motor_inertia", C.POINTER(_d)), ("u_lb", C.POINTER(_d)),
                ("u_ub", C.POINTER(_d)), ("params_dev", C.c_void_p)]


class Mpc(C.Structure):
    """aslr_mpc_t: a receding-horizon run (aslr_mpc_run); device pointers, time-major arrays."""
    _fields_ = [("n_steps", _i), ("first_maxiter", _i), ("iters_per_step", _i), ("_pad0", _i),
                ("disturbance", C.c_void_p), ("x_closed", C.c_void_p), ("u_closed", C.c_void_p),
                ("stat_f", C.c_void_p), ("stat_i", C.c_void_p)]


class Design(C.Structure):
    """aslr_design_t (include/aslr_to_amd_design.h): a design descent (aslr_design_descent); device pointers, rows [2 nj][B]."""
    _fields_ = [("n_steps", _i), ("first_maxiter", _i), ("iters_per_step", _i), ("opt_stiffness", _i),
                ("opt_motor_inertia", _i), ("_pad0", _i), ("eta0", _d), ("grow", _d), ("shrink", _d), ("c1", _d),
                ("max_rel", _d), ("lo", C.c_void_p), ("hi", C.c_void_p), ("theta_best", C.c_void_p),
                ("cost_best", C.c_void_p), ("xs_best", C.c_void_p), ("us_best", C.c_void_p), ("hist_f", C.c_void_p),
                ("hist_i", C.c_void_p), ("theta_hist", C.c_void_p), ("g_acc", C.c_void_p), ("eta", C.c_void_p),
                ("grad", C.c_void_p)]


class Identify(C.Structure):
    """aslr_identify_t (include/aslr_to_amd_identify.h): a plant identification (aslr_plant_identify); device pointers, rows
    [np][B]."""
    _fields_ = [("n_steps", _i), ("fit_stiffness", _i), ("fit_motor_inertia", _i), ("_pad0", _i), ("mu0", _d), ("mu_min", _d),
                ("mu_max", _d), ("grow", _d), ("shrink", _d), ("max_rel", _d), ("min_curv", _d), ("weights", C.c_void_p),
                ("lo", C.c_void_p), ("hi", C.c_void_p), ("theta", C.c_void_p), ("sse", C.c_void_p), ("grad", C.c_void_p),
                ("information", C.c_void_p), ("mu", C.c_void_p), ("identifiable", C.c_void_p), ("n_accepted", C.c_void_p),
                ("hist_theta", C.c_void_p), ("hist_sse", C.c_void_p), ("hist_decision", C.c_void_p), ("work", C.c_void_p)]


class Region(C.Structure):
    _fields_ = [("offset", C.c_int64), ("bytes", C.c_int64)]


def default_solver_params(solver=SOLVER_DDP):
    """Defaults of crocoddyl.SolverDDP / BoxQP; pure host logic, mirrors
    aslr_solver_params_default() of the library (tests check they agree)."""
    sp = SolverParams()
    sp.solver = solver
    sp.maxiter = 100
    sp.is_feasible = 0
    sp.fixed_iterations = 0
    sp.reg_init = float("nan")
    sp.th_stop = 1e-9
    sp.th_grad = 1e-12
    sp.th_gaptol = 1e-16
    sp.th_stepdec = 0.5
    sp.th_stepinc = 0.01
    sp.th_acceptstep = 0.1
    sp.th_acceptnegstep = 2.0
    sp.reg_min = 1e-9
    sp.reg_max = 1e9
    sp.reg_incfactor = 10.0
    sp.reg_decfactor = 10.0
    sp.boxqp_maxiter = 100
    sp.boxqp_th_acceptstep = 0.1
    sp.boxqp_th_grad = 1e-5
    sp.boxqp_reg = 0.0
    return sp


def record_len(nx, nu):
    n = 2 * nx * nx + 2 * nx * nu + nu * nu + nx + nu
    return (n + 15) // 16 * 16


def record_offsets(nx, nu):
    """Offsets (in doubles) of the blocks of one DERIV record."""
    o = {}
    o["Fx"] = 0
    o["Fu"] = o["Fx"] + nx * nx
    o["Lxx"] = o["Fu"] + nx * nu
    o["Lxu"] = o["Lxx"] + nx * nx
    o["Luu"] = o["Lxu"] + nx * nu
    o["Lx"] = o["Luu"] + nu * nu
    o["Lu"] = o["Lx"] + nx
    return o


LIB_NAME = "libaslr_to_hip.so"
_lib = None


def lib_path():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", LIB_NAME)


_vp, _i64, _sp = C.c_void_p, C.c_int64, C.POINTER(SolverParams)
_rollout = [_vp, C.c_int, _vp, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp]
_mpc_plant = [_vp, _sp, C.POINTER(Mpc), C.c_int, _vp, _vp, C.c_int, _vp, _vp, _vp]

# header under include/ -> {function it declares: (restype, argtypes)}, in the order of the symbol lists below; argtypes
# None: left unset (a function without parameters).  The base header comes first; every extension is exported from the same
# library under a header of its own, so that the base header, its symbol list and ABI_VERSION stay what existing bindings
# check against.  (The aslr_debug_* exports are in no header and not bound here.)
PROTOTYPES = {
    "aslr_to_amd.h": {
        "aslr_abi_version": (C.c_int, None),
        "aslr_sizeof": (_i64, [C.c_int]),
        "aslr_record_len": (_i, [_i, _i]),
        "aslr_solver_params_default": (None, [_sp, _i]),
        "aslr_workspace_bytes": (_i64, [C.POINTER(ProblemDesc)]),
        "aslr_problem_create": (C.c_int, [C.POINTER(ProblemDesc), _vp, _i64, _vp, C.POINTER(_vp)]),
        "aslr_problem_destroy": (C.c_int, [_vp]),
        "aslr_problem_region": (C.c_int, [_vp, _i, C.POINTER(Region)]),
        "aslr_calc": (C.c_int, [_vp, _vp]),
        "aslr_calc_diff": (C.c_int, [_vp, _vp]),
        "aslr_backward_pass": (C.c_int, [_vp, _sp, _vp]),
        "aslr_forward_pass": (C.c_int, [_vp, _sp, _vp]),
        "aslr_solve": (C.c_int, [_vp, _sp, _i, _vp, C.POINTER(_i)]),
        "aslr_iterate": (C.c_int, [_vp, _sp, _i, _vp]),
        "aslr_iterate_timed": (C.c_int, [_vp, _sp, _i, _vp, C.POINTER(C.c_float)]),
        "aslr_finalize": (C.c_int, [_vp, _vp]),
        "aslr_count_active": (C.c_int, [_vp, _vp, C.POINTER(_i)]),
        "aslr_dam_eval": (C.c_int, [_vp, _i, _i] + [_vp] * 12),
        "aslr_quasi_static": (C.c_int, [_vp, _i, _d, _vp, _vp]),
        "aslr_last_error": (C.c_char_p, None),
        "aslr_dam_residuals": (C.c_int, [_vp, _i, _i, _vp, _vp, _vp, _vp]),
        "aslr_residual_len": (_i, [C.POINTER(Model), _i]),
        "aslr_frame_placement": (C.c_int, [_vp, _i, C.POINTER(_d), C.POINTER(_d), _i, _vp, _i64, _vp, _vp]),
        "aslr_set_iteration_log": (C.c_int, [_vp, _vp, _i]),
        "aslr_iterate_n": (C.c_int, [_vp, _sp, _i, _i, _vp]),
        "aslr_set_subshards": (C.c_int, [_vp, _i]),
        "aslr_solve_pool": (C.c_int, [_vp, _sp, C.POINTER(Pool), _i, _i, _vp, C.POINTER(_i)]),
        "aslr_set_trajectory_params": (C.c_int, [_vp, C.POINTER(TrajParams), _vp]),
        "aslr_mpc_run": (C.c_int, [_vp, _sp, C.POINTER(Mpc), _vp]),
        "aslr_set_reference_path": (C.c_int, [_vp, _vp, _i, _i, _vp]),
        "aslr_reference_row": (C.c_int, [_vp, C.POINTER(_i)]),
    },
    "aslr_to_amd_sens.h": {"aslr_cost_sensitivity": (C.c_int, [_vp] * 6)},
    "aslr_to_amd_policy.h": {"aslr_policy_rollout": (C.c_int, _rollout)},
    "aslr_to_amd_mpc_plant.h": {"aslr_mpc_run_plant": (C.c_int, _mpc_plant)},
    "aslr_to_amd_pool_params.h": {
        "aslr_solve_pool_params": (C.c_int, [_vp, _sp, C.POINTER(Pool), C.POINTER(PoolParams), _i, _i, _vp, C.POINTER(_i)])},
    "aslr_to_amd_cov.h": {"aslr_policy_covariance": (C.c_int, [_vp] * 9)},
    "aslr_to_amd_lqg.h": {"aslr_policy_lqg": (C.c_int, [_vp, _i, C.POINTER(_i)] + [_vp] * 11)},
    "aslr_to_amd_plant_sens.h": {"aslr_policy_plant_sensitivity": (C.c_int, [_vp] * 12)},
    "aslr_to_amd_design.h": {"aslr_design_descent": (C.c_int, [_vp, _sp, C.POINTER(Design), _vp])},
    "aslr_to_amd_policy_all.h": {"aslr_policy_rollout_all": (C.c_int, _rollout)},
    "aslr_to_amd_mpc_plant_all.h": {"aslr_mpc_run_plant_all": (C.c_int, _mpc_plant)},
    "aslr_to_amd_policy_noise.h": {
        "aslr_policy_rollout_noise": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_uint64, _vp, _vp, _vp, _vp, C.c_int] + [_vp] * 10)},
    "aslr_to_amd_identify.h": {"aslr_plant_identify": (C.c_int, [_vp, C.POINTER(Identify), _vp])},
    "aslr_to_amd_smooth.h": {"aslr_state_smooth": (C.c_int, [_vp, _i, C.POINTER(_i)] + [_vp] * 5 + [_i, C.c_double] + [_vp] * 8)},
}

# header -> the module attribute that lists what it declares (EXPORTED_SYMBOLS: the base header's)
SYMBOL_LISTS = {
    "aslr_to_amd.h": "EXPORTED_SYMBOLS", "aslr_to_amd_sens.h": "EXTENSION_SYMBOLS", "aslr_to_amd_policy.h": "POLICY_SYMBOLS",
    "aslr_to_amd_mpc_plant.h": "MPC_PLANT_SYMBOLS", "aslr_to_amd_pool_params.h": "POOL_PARAMS_SYMBOLS",
    "aslr_to_amd_cov.h": "COV_SYMBOLS", "aslr_to_amd_lqg.h": "LQG_SYMBOLS", "aslr_to_amd_plant_sens.h": "PLANT_SENS_SYMBOLS",
    "aslr_to_amd_design.h": "DESIGN_SYMBOLS", "aslr_to_amd_policy_all.h": "POLICY_ALL_SYMBOLS",
    "aslr_to_amd_mpc_plant_all.h": "MPC_PLANT_ALL_SYMBOLS", "aslr_to_amd_policy_noise.h": "POLICY_NOISE_SYMBOLS",
    "aslr_to_amd_identify.h": "IDENTIFY_SYMBOLS", "aslr_to_amd_smooth.h": "SMOOTH_SYMBOLS",
}
globals().update((attr, list(PROTOTYPES[header])) for header, attr in SYMBOL_LISTS.items())


def load_library():
    """Load the HIP C-ABI library; raise loudly when it is absent (no fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise ImportError(
            "aslr_to_amd: the HIP extension %s is missing. Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950). "
            "There is no CPU fallback." % path)
    # torch first: its bundled HIP runtime must be the one (and only) libamdhip64 in the process, or
    # device pointers of torch tensors would belong to a different runtime than our kernel launches
    import torch  # noqa: F401
    lib = C.CDLL(path)
    for functions in PROTOTYPES.values():
        for name, (restype, argtypes) in functions.items():
            f = getattr(lib, name)
            f.restype = restype
            if argtypes is not None:
                f.argtypes = argtypes
    if lib.aslr_abi_version() != ABI_VERSION:
        raise ImportError("aslr_to_amd: ABI version mismatch between %s and the Python layer" % path)
    for which, st in enumerate((Chain, Cost, Model, ProblemDesc, SolverParams, Region, Pool, TrajParams, Mpc)):
        if lib.aslr_sizeof(which) != C.sizeof(st):
            raise ImportError("aslr_to_amd: struct %s size mismatch (C %d, Python %d)"
                              % (st.__name__, lib.aslr_sizeof(which), C.sizeof(st)))
    _lib = lib
    return lib


class AslrError(RuntimeError):
    pass


def check(rc, what):
    if rc != OK:
        msg = {E_INVALID: "invalid argument", E_HIP: "HIP error", E_NODEVICE: "no GPU device",
               E_WORKSPACE: "workspace too small or misaligned"}.get(rc, "error %d" % rc)
        detail = ""
        if _lib is not None:
            e = _lib.aslr_last_error()
            if e:
                detail = ": " + e.decode()
        raise AslrError("%s failed: %s%s" % (what, msg, detail))
