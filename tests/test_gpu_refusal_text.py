"""The whole text of aslr_last_error() for the refusals of the extension calls whose host code is shared: aslr_policy_rollout,
aslr_policy_rollout_all, aslr_mpc_run_plant, aslr_mpc_run_plant_all, aslr_solve_pool, aslr_solve_pool_params,
aslr_cost_sensitivity, aslr_policy_plant_sensitivity and aslr_design_descent.

Every expected string is written out; none is formatted from the pattern the library formats.  Every case returns before a
launch (the bounds cases of aslr_design_descent after its two small read-backs), on handles of B = 2, T = 3; no pointer given
here is ever written through.

Refusals no test reaches, because create refuses first or only a failing device call produces them:
  "... no per-trajectory-parameter kernels for (nj, dam)": aslr_problem_create admits only the sizes that have a row in the
  table of kernel sets, and every row has its TP row (the extension calls take their kernels from the handle's row and
  refuse no size of their own);
  "... motor inertia entry B[j] of model i is 0" and "... motor inertia entry [b][j] of the initial design is not positive":
  create refuses a singular B, aslr_set_trajectory_params a non-positive one;
  "... %d of %d problems finished within the iteration bound" and "... putting the handle's x0 / frame_ref back failed": behind
  the pool's launches;
  "aslr_mpc_run_plant: ... would overflow" through the reference row (the n_steps * hold form is covered)."""
import ctypes as C

import numpy as np
import pytest

import _gpu_case as gc
from aslr_to_amd import _abi, scenarios

pytestmark = pytest.mark.gpu

ROLLOUTS = ("aslr_policy_rollout", "aslr_policy_rollout_all")
MPC_PLANTS = ("aslr_mpc_run_plant", "aslr_mpc_run_plant_all")
TABLE_SET = {
    "aslr_solve_pool": "aslr_solve_pool: the handle has a per-trajectory parameter table set (a pool problem would inherit its "
                       "slot's parameters); clear it with aslr_set_trajectory_params(p, NULL, stream)",
    "aslr_solve_pool_params": "aslr_solve_pool_params: the handle has a per-trajectory parameter table set (the refill overwrites "
                              "region TRAJ_PARAMS: the table would be lost); clear it with aslr_set_trajectory_params(p, NULL, "
                              "stream), or give its rows in pp",
}


def _sea():
    return scenarios.lower(scenarios.two_dof_sea(B=2, T=3))


def _edited(edit):
    low = _sea()
    edit(low.desc)
    return low


def _non_diagonal(d):
    d.models[0].K[1] = 0.1                      # K[0][1] of model 0


def _zero_stiffness(d):
    for i in range(d.nmodels):
        d.models[i].K[0] = 0.0                  # K[0][0]


def _both_in_model_0(d):
    d.models[0].K[1] = 0.1
    d.models[0].K[0] = 0.0


def _zero_before_non_diagonal(d):
    d.models[0].K[0] = 0.0                      # model 0: a zero stiffness ...
    d.models[1].K[1] = 0.1                      # ... model 1: not diagonal.  The walk meets model 0's zero first


def _models_differ(d):
    d.models[1].K[0] = 2.0 * d.models[0].K[0]
    d.models[1].B[0] = 2.0 * d.models[0].B[0]


def _stiffness_two(d):
    for i in range(d.nmodels):
        d.models[i].K[0] = 2.0


def _no_frame_ref(d):
    d.frame_ref = C.POINTER(C.c_double)()


def _two_running_models(d):
    d.node_model[1] = 1                         # the terminal model on a running knot


def _limits_differ(d):
    d.models[1].has_u_limits = 1
    for c in range(4):
        d.models[1].u_lb[c] = d.models[0].u_lb[c]
        d.models[1].u_ub[c] = d.models[0].u_ub[c]
    d.models[1].u_lb[0] -= 1.0
    d.models[1].u_ub[0] += 1.0


def _vsa():
    return scenarios.lower(scenarios.two_dof_vsa_boxddp(B=2, T=3))


def _vsa_limits_differ():
    low = _vsa()
    _limits_differ(low.desc)
    return low


LOWERED = {
    "sea": _sea,
    "vsa": _vsa,
    "arm": lambda: scenarios.lower(scenarios.talos_arm_sea(B=2, T=3)),
    "arm_vsa": lambda: scenarios.lower(scenarios.talos_arm_vsa(B=2, T=3)),
    "non_diagonal": lambda: _edited(_non_diagonal),
    "zero_stiffness": lambda: _edited(_zero_stiffness),
    "both_in_model_0": lambda: _edited(_both_in_model_0),
    "zero_before_non_diagonal": lambda: _edited(_zero_before_non_diagonal),
    "models_differ": lambda: _edited(_models_differ),
    "stiffness_two": lambda: _edited(_stiffness_two),
    "no_frame_ref": lambda: _edited(_no_frame_ref),
    "two_running_models": lambda: _edited(_two_running_models),
    "vsa_limits_differ": _vsa_limits_differ,
    "table": _sea,
    "zero_in_table": _sea,
    "path": _sea,
}


class Handles(object):
    """the handles of this file, each created once on first use and never solved on"""

    def __init__(self):
        import torch
        self.made = {}
        self.buf = torch.zeros(4096, dtype=torch.float64, device="cuda")      # stands wherever a device pointer goes
        self.ptr = C.c_void_p(self.buf.data_ptr())

    def __getitem__(self, name):
        if name not in self.made:
            e = gc.engine(LOWERED[name]())
            if name == "table":
                e.set_trajectory_params(motor_inertia=np.full((2, 2), 0.02))
            if name == "zero_in_table":
                e.set_trajectory_params(stiffness=np.array([[1.0, 1.0], [0.0, 1.0]]))
            if name == "path":
                sc = scenarios.two_dof_sea(B=2, T=3)
                e.set_reference_path(scenarios.hold_via_points(scenarios.reference_via_points(sc), 3))
            self.made[name] = e
        return self.made[name]


@pytest.fixture(scope="module")
def handles():
    h = Handles()
    yield h
    for e in h.made.values():
        e.close()


def _sp(solver="SolverFDDP", **more):
    return scenarios.solver_params(dict(solver=solver, maxiter=3, th_stop=1e-7), **more)


def _refused(e, name, args, text):
    lib = _abi.load_library()
    assert lib.aslr_workspace_bytes(None) < 0          # another call's message is in the buffer first
    rc = getattr(lib, name)(e.handle if e is not None else None, *args)
    assert rc == _abi.E_INVALID, (name, rc)
    assert lib.aslr_last_error().decode() == text


# ---------------------------------------------------------------------------------------------------------------------
# aslr_policy_rollout / aslr_policy_rollout_all
# ---------------------------------------------------------------------------------------------------------------------
def _rollout_args(h, n_samples=1, plant_stiffness=False, plant_motor_inertia=False, outputs=True):
    p, out = h.ptr, h.ptr if outputs else None
    return (n_samples, p if plant_stiffness else None, p if plant_motor_inertia else None, None, None, 0, out, out, out, None,
            None, None)


@pytest.mark.parametrize("fn", ROLLOUTS)
def test_rollout_refusals(handles, fn):
    h = handles
    _refused(None, fn, _rollout_args(h), fn + ": the problem handle p is NULL")
    _refused(h["sea"], fn, _rollout_args(h, n_samples=0), fn + ": n_samples is 0, must be positive")
    _refused(h["sea"], fn, _rollout_args(h, n_samples=-3), fn + ": n_samples is -3, must be positive")
    _refused(h["sea"], fn, _rollout_args(h, n_samples=1048561), fn + ": n_samples is 1048561, above the 1048560 of one launch")
    _refused(h["sea"], fn, _rollout_args(h, outputs=False), fn + ": all five outputs are NULL: nothing to compute")
    _refused(h["vsa"], fn, _rollout_args(h, plant_stiffness=True),
             fn + ": plant_stiffness on a VSA model, which takes its stiffness from u")
    for which in (dict(plant_stiffness=True), dict(plant_motor_inertia=True)):
        _refused(h["non_diagonal"], fn, _rollout_args(h, **which),
                 fn + ": a plant argument needs diagonal K and B, and those of model 0 are not")
    _refused(h["zero_before_non_diagonal"], fn, _rollout_args(h, plant_motor_inertia=True),
             fn + ": a plant argument needs diagonal K and B, and those of model 1 are not")


def test_the_two_joint_rollout_names_the_call_that_serves_the_arms(handles):
    _refused(handles["arm"], "aslr_policy_rollout", _rollout_args(handles),
             "aslr_policy_rollout: the roll-out kernel is built for the nx = 8 sizes (2 joints), not for this 7-joint handle "
             "(the 7-joint team form is not built); aslr_policy_rollout_all serves every size")
    # the size is judged before the plant arguments
    _refused(handles["arm"], "aslr_policy_rollout", _rollout_args(handles, plant_stiffness=True, n_samples=2),
             "aslr_policy_rollout: the roll-out kernel is built for the nx = 8 sizes (2 joints), not for this 7-joint handle "
             "(the 7-joint team form is not built); aslr_policy_rollout_all serves every size")


# ---------------------------------------------------------------------------------------------------------------------
# aslr_mpc_run_plant / aslr_mpc_run_plant_all
# ---------------------------------------------------------------------------------------------------------------------
def _mpc(h, n_steps=1, first_maxiter=1, iters_per_step=1, buffers=True):
    p = h.buf.data_ptr() if buffers else None
    return _abi.Mpc(n_steps=n_steps, first_maxiter=first_maxiter, iters_per_step=iters_per_step, x_closed=p, u_closed=p,
                    stat_f=p, stat_i=p)


def _plant_args(h, sp, mpc, hold=1, plant_stiffness=False, plant_motor_inertia=False):
    return (C.byref(sp) if sp is not None else None, C.byref(mpc) if mpc is not None else None, hold,
            h.ptr if plant_stiffness else None, h.ptr if plant_motor_inertia else None, 0, None, None, None)


@pytest.mark.parametrize("fn", MPC_PLANTS)
def test_mpc_plant_refusals(handles, fn):
    h, sp = handles, _sp()
    e, mpc = h["sea"], _mpc(h)
    _refused(None, fn, _plant_args(h, sp, mpc), fn + ": NULL argument: the problem handle p")
    _refused(e, fn, _plant_args(h, None, mpc), fn + ": NULL argument: sp")
    _refused(e, fn, _plant_args(h, sp, None), fn + ": NULL argument: mpc")
    for bad in (dict(n_steps=0), dict(first_maxiter=0), dict(iters_per_step=0)):
        _refused(e, fn, _plant_args(h, sp, _mpc(h, **bad)), fn + ": n_steps, first_maxiter and iters_per_step must be >= 1")
    _refused(e, fn, _plant_args(h, sp, _mpc(h, buffers=False)), fn + ": x_closed, u_closed, stat_f and stat_i must be given")
    _refused(h["two_running_models"], fn, _plant_args(h, sp, mpc),
             fn + ": the running knots use more than one action model: shifting the plan needs one (references that vary along "
             "the horizon: aslr_set_reference_path)")
    e.enable_iteration_log(4)
    try:
        _refused(e, fn, _plant_args(h, sp, mpc), fn + ": an iteration log is set (every step would overwrite it): clear it with "
                 "aslr_set_iteration_log(p, NULL, 0)")
    finally:
        e.enable_iteration_log(0)
    _refused(h["arm_vsa"], fn, _plant_args(h, sp, mpc), fn + ": the solver kernels for (nj=7, VSA) are built for SolverBoxDDP "
             "only: model-level evaluation only with SolverDDP / SolverFDDP")
    _refused(e, fn, _plant_args(h, sp, mpc, hold=0), fn + ": hold = 0 must lie in [1, T = 3]")
    _refused(e, fn, _plant_args(h, sp, mpc, hold=4), fn + ": hold = 4 must lie in [1, T = 3]")
    _refused(h["vsa"], fn, _plant_args(h, _sp("SolverBoxDDP"), mpc, plant_stiffness=True),
             fn + ": plant_stiffness on a VSA model, which takes its stiffness from u")
    for which in (dict(plant_stiffness=True), dict(plant_motor_inertia=True)):
        _refused(h["non_diagonal"], fn, _plant_args(h, sp, mpc, **which),
                 fn + ": a plant argument needs diagonal K and B, and those of model 0 are not")
    _refused(e, fn, _plant_args(h, sp, _mpc(h, n_steps=2 ** 30), hold=3),
             fn + ": n_steps * hold, or the reference row after them, would overflow: reposition the row with "
             "aslr_set_reference_path")


def test_the_two_joint_mpc_plant_names_the_call_that_serves_the_arms(handles):
    _refused(handles["arm"], "aslr_mpc_run_plant", _plant_args(handles, _sp(), _mpc(handles), plant_stiffness=True),
             "aslr_mpc_run_plant: the plant kernel is built for the nx = 8 sizes (2 joints), not for this 7-joint handle; "
             "aslr_mpc_run_plant_all serves every size")


# ---------------------------------------------------------------------------------------------------------------------
# aslr_solve_pool / aslr_solve_pool_params
# ---------------------------------------------------------------------------------------------------------------------
def _pool(h, P=1, frame_ref=False, **missing):
    p = h.buf.data_ptr()
    pool = _abi.Pool(P=P, x0=p, xs_out=p, us_out=p, stat_f=p, stat_i=p, slot_problem=p, counters=p,
                     frame_ref=p if frame_ref else None)
    for k in missing:
        setattr(pool, k, None)
    return pool


def _host(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(C.POINTER(C.c_double))


def _pool_params(h, params_dev=True, **fields):
    """aslr_pool_params_t with the host rows given (P = 1) and the arrays that keep them alive"""
    pp, keep = _abi.PoolParams(), []
    for k, v in fields.items():
        a, ptr = _host(v)
        keep.append(a)
        setattr(pp, k, ptr)
    pp.params_dev = h.buf.data_ptr() if params_dev else None
    return pp, keep


def _pool_args(h, fn, sp, pool, pp=None):
    head = (C.byref(sp) if sp is not None else None, C.byref(pool) if pool is not None else None)
    tail = (2, 4, None, None)
    return head + tail if fn == "aslr_solve_pool" else head + (C.byref(pp),) + tail


@pytest.mark.parametrize("fn", ("aslr_solve_pool", "aslr_solve_pool_params"))
def test_pool_refusals(handles, fn):
    h, sp = handles, _sp()
    pp, keep = _pool_params(h, motor_inertia=[[0.02, 0.02]])
    e, pool = h["sea"], _pool(h)
    _refused(None, fn, _pool_args(h, fn, sp, pool, pp), fn + ": the problem handle p is NULL")
    _refused(e, fn, _pool_args(h, fn, None, pool, pp), fn + ": sp is NULL")
    _refused(e, fn, _pool_args(h, fn, sp, None, pp), fn + ": pool is NULL")
    _refused(e, fn, _pool_args(h, fn, sp, _pool(h, P=0), pp), fn + ": pool->P = 0 must be >= 1")
    for k in ("x0", "xs_out", "us_out", "stat_f", "stat_i", "slot_problem", "counters"):
        _refused(e, fn, _pool_args(h, fn, sp, _pool(h, **{k: None}), pp),
                 fn + ": x0, xs_out, us_out, stat_f, stat_i, slot_problem and counters of the pool must be given")
    _refused(e, fn, _pool_args(h, fn, _sp(maxiter=0), pool, pp),
             fn + ": sp->maxiter = 0 must be >= 1 and sp->fixed_iterations = 0 must be 0 (slots stop by themselves)")
    _refused(e, fn, _pool_args(h, fn, _sp(fixed_iterations=1), pool, pp),
             fn + ": sp->maxiter = 3 must be >= 1 and sp->fixed_iterations = 1 must be 0 (slots stop by themselves)")
    _refused(h["no_frame_ref"], fn, _pool_args(h, fn, sp, _pool(h, frame_ref=True), pp),
             fn + ": per-problem frame references need a problem created with a frame_ref table")
    _refused(h["table"], fn, _pool_args(h, fn, sp, pool, pp), TABLE_SET[fn])
    _refused(h["path"], fn, _pool_args(h, fn, sp, pool, pp),
             fn + ": the handle has a reference path set (a pool problem would inherit its slot's path); clear it with "
             "aslr_set_reference_path(p, NULL, 0, 0, stream)")
    pp7, keep7 = _pool_params(h, motor_inertia=[[0.02] * 7])
    _refused(h["arm_vsa"], fn, _pool_args(h, fn, sp, pool, pp7), fn + ": the solver kernels for (nj=7, VSA) are built for "
             "SolverBoxDDP only: model-level evaluation only with SolverDDP / SolverFDDP")
    del keep, keep7


def test_pool_params_without_a_field_is_the_older_call_by_name(handles):
    h = handles
    pp, _ = _pool_params(h)
    _refused(h["table"], "aslr_solve_pool_params", _pool_args(h, "aslr_solve_pool_params", _sp(), _pool(h), pp),
             TABLE_SET["aslr_solve_pool"])
    _refused(h["sea"], "aslr_solve_pool_params", (C.byref(_sp()), C.byref(_pool(h, P=0)), None, 2, 4, None, None),
             "aslr_solve_pool: pool->P = 0 must be >= 1")


def test_pool_params_refusals_of_its_own(handles):
    h, fn, sp = handles, "aslr_solve_pool_params", _sp()
    bsp = _sp("SolverBoxDDP")

    def refused(name, text, sp=sp, params_dev=True, **fields):
        pp, keep = _pool_params(h, params_dev=params_dev, **fields)
        _refused(h[name], fn, _pool_args(h, fn, sp, _pool(h), pp), fn + text)
        del keep

    one, four = [[0.02, 0.02]], [[1.0] * 4]
    refused("sea", ": params_dev is NULL while a parameter field is given (DEVICE scratch of [2 nj + 2 nu][P] doubles)",
            params_dev=False, motor_inertia=one)
    # ---- the row builder it shares with aslr_set_trajectory_params ----
    refused("vsa", ": a VSA model takes its stiffness from u: no stiffness table", sp=bsp, stiffness=one)
    refused("non_diagonal", ": K and B of every model must be diagonal", motor_inertia=one)
    refused("sea", ": u_lb / u_ub given, but no model of the problem has control limits", u_lb=[[0.0, 0.0]])
    refused("models_differ", ": the models differ in K: give the stiffness table", motor_inertia=one)
    refused("models_differ", ": the models differ in B: give the motor_inertia table", stiffness=one)
    refused("vsa_limits_differ", ": the models differ in u_lb: give the u_lb table", sp=bsp, motor_inertia=one)
    refused("vsa_limits_differ", ": the models differ in u_ub: give the u_ub table", sp=bsp, u_lb=four)
    refused("sea", ": stiffness entries must be finite", stiffness=[[1.0, np.nan]])
    refused("sea", ": motor_inertia entries must be finite and > 0", motor_inertia=[[0.02, 0.0]])
    refused("sea", ": motor_inertia entries must be finite and > 0", motor_inertia=[[np.inf, 0.02]])
    refused("vsa", ": u_lb <= u_ub must hold in every entry (no NaN)", sp=bsp, u_lb=[[200.0] * 4])
    refused("vsa", ": u_lb <= u_ub must hold in every entry (no NaN)", sp=bsp, u_ub=[[np.nan] * 4])


# ---------------------------------------------------------------------------------------------------------------------
# aslr_cost_sensitivity / aslr_policy_plant_sensitivity: the walk over the models, then over the table
# ---------------------------------------------------------------------------------------------------------------------
def _sens_args(h, fn, stiffness=True, nothing=False):
    """outputs that ask for the stiffness term (or not), for either call"""
    p = h.ptr
    if fn == "aslr_cost_sensitivity":
        return (None,) * 5 if nothing else (p if stiffness else None, p, None, None, None)
    if nothing:
        return (None,) * 11
    return (None, None, None, None, p if stiffness else None, p, None, None, None, None, None)


@pytest.mark.parametrize("fn", ("aslr_cost_sensitivity", "aslr_policy_plant_sensitivity"))
def test_the_walk_over_the_models_and_the_table(handles, fn):
    h = handles
    _refused(None, fn, _sens_args(h, fn), fn + ": the problem handle p is NULL")
    _refused(h["non_diagonal"], fn, _sens_args(h, fn), fn + ": K and B of model 0 must be diagonal")
    _refused(h["non_diagonal"], fn, _sens_args(h, fn, stiffness=False), fn + ": K and B of model 0 must be diagonal")
    _refused(h["zero_stiffness"], fn, _sens_args(h, fn),
             fn + ": stiffness entry K[0] of model 0 is 0 (the stiffness term divides by it)")
    # two defects at once: the diagonal test of a model comes before its entries ...
    _refused(h["both_in_model_0"], fn, _sens_args(h, fn), fn + ": K and B of model 0 must be diagonal")
    # ... and the entries of model 0 before the diagonal test of model 1
    _refused(h["zero_before_non_diagonal"], fn, _sens_args(h, fn),
             fn + ": stiffness entry K[0] of model 0 is 0 (the stiffness term divides by it)")
    _refused(h["zero_in_table"], fn, _sens_args(h, fn),
             fn + ": stiffness entry [1][0] of the parameter table is 0 (the stiffness term divides by it)")


def test_cost_sensitivity_refusals_of_its_own(handles):
    h, fn = handles, "aslr_cost_sensitivity"
    _refused(h["sea"], fn, _sens_args(h, fn, nothing=True), fn + ": all four outputs are NULL: nothing to compute")
    _refused(h["vsa"], fn, _sens_args(h, fn), fn + ": dcost_dstiffness on a VSA model, which takes its stiffness from u")


def test_plant_sensitivity_refusals_of_its_own(handles):
    h, fn, p = handles, "aslr_policy_plant_sensitivity", handles.ptr
    _refused(h["sea"], fn, _sens_args(h, fn, nothing=True), fn + ": all eight outputs are NULL: nothing to compute")
    vsa_text = fn + ": a stiffness argument on a VSA model, which takes its stiffness from u"
    _refused(h["vsa"], fn, _sens_args(h, fn), vsa_text)
    _refused(h["vsa"], fn, (p, None, None, None, None, p, None, None, None, None, None), vsa_text)
    _refused(h["sea"], fn, (None, None, None, None, None, None, None, None, p, p, None),
             fn + ": x_var or u_var with stiffness_var and motor_inertia_var both NULL: no variance to propagate")
    # without a stiffness output the zero stiffness is not divided by: the call is not refused for it (and not made here)


# ---------------------------------------------------------------------------------------------------------------------
# aslr_design_descent
# ---------------------------------------------------------------------------------------------------------------------
def _design(h, **fields):
    p = h.buf.data_ptr()
    d = _abi.Design(n_steps=1, first_maxiter=1, iters_per_step=1, opt_stiffness=1, opt_motor_inertia=0, eta0=0.05, grow=2.0,
                    shrink=0.5, c1=1e-4, max_rel=0.25, lo=p, hi=p, theta_best=p, cost_best=p, xs_best=p, us_best=p, g_acc=p,
                    eta=p, grad=p)
    for k, v in fields.items():
        setattr(d, k, v)
    return d


def test_design_descent_refusals(handles):
    import torch
    h, fn, sp = handles, "aslr_design_descent", _sp()
    e = h["sea"]

    def refused(name, text, sp=sp, **fields):
        d = _design(h, **fields)
        _refused(h[name], fn, (C.byref(sp), C.byref(d), None), fn + text)

    d = _design(h)
    _refused(None, fn, (C.byref(sp), C.byref(d), None), fn + ": NULL argument: the problem handle p")
    _refused(e, fn, (None, C.byref(d), None), fn + ": NULL argument: sp")
    _refused(e, fn, (C.byref(sp), None, None), fn + ": NULL argument: d")
    for k in ("n_steps", "first_maxiter", "iters_per_step"):
        refused("sea", ": n_steps, first_maxiter and iters_per_step must be >= 1", **{k: 0})
    refused("sea", ": neither opt_stiffness nor opt_motor_inertia is set: nothing to optimise", opt_stiffness=0)
    refused("vsa", ": opt_stiffness on a VSA model, which takes its stiffness from u", sp=_sp("SolverBoxDDP"))
    for k in ("lo", "hi", "theta_best", "cost_best", "xs_best", "us_best", "g_acc", "eta", "grad"):
        refused("sea", ": lo, hi, theta_best, cost_best, xs_best, us_best, g_acc, eta and grad must be given", **{k: None})
    refused("sea", ": eta0 = 0 must be finite and > 0", eta0=0.0)
    refused("sea", ": eta0 = inf must be finite and > 0", eta0=float("inf"))
    refused("sea", ": grow = 0.5 must be finite and >= 1", grow=0.5)
    refused("sea", ": shrink = 1 must lie in (0, 1)", shrink=1.0)
    refused("sea", ": c1 = 0 must lie in (0, 1)", c1=0.0)
    refused("sea", ": max_rel = 1 must lie in (0, 1)", max_rel=1.0)
    e.enable_iteration_log(4)
    try:
        refused("sea", ": an iteration log is set (every step would overwrite it): clear it with aslr_set_iteration_log(p, NULL, 0)")
    finally:
        e.enable_iteration_log(0)
    refused("arm_vsa", ": the solver kernels for (nj=7, VSA) are built for SolverBoxDDP only: model-level evaluation only with "
            "SolverDDP / SolverFDDP", opt_stiffness=0, opt_motor_inertia=1)
    refused("non_diagonal", ": K and B of model 0 must be diagonal")
    refused("zero_before_non_diagonal", ": K and B of model 1 must be diagonal")       # (no look at zeros in this walk)
    refused("models_differ", ": the models differ in K: give the stiffness table")
    refused("zero_stiffness", ": stiffness entry [0][0] of the initial design is not positive")
    # ---- the bounds, [2 nj][B] with the stiffness rows first: read back, nothing enqueued before the refusal ----
    bounds = {v: torch.full((4, 2), v, dtype=torch.float64, device="cuda") for v in (0.0, 1.0, 3.0, 4.0)}
    rows = lambda v: bounds[v].data_ptr()
    refused("stiffness_two", ": bounds [0][0] are (0, 1): 0 < lo <= hi must hold, finite", lo=rows(0.0), hi=rows(1.0))
    refused("stiffness_two", ": bounds [0][0] are (4, 3): 0 < lo <= hi must hold, finite", lo=rows(4.0), hi=rows(3.0))
    refused("stiffness_two", ": entry [0][0] of the initial design, 2, lies outside its bounds [3, 4]", lo=rows(3.0), hi=rows(4.0))
    torch.cuda.synchronize()
