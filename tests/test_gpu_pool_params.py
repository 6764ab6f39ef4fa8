"""aslr_solve_pool_params on the GPU: a pool whose problems carry their own stiffness, motor inertia and control box.

The yardstick is BITWISE equality with one batched aslr_solve of the same P problems on a handle whose parameter table holds
the same rows.  That path is held to the per-trajectory CPU oracle by tests/test_gpu_traj_params.py, so no tolerance is
introduced here.  The draws are tests/_pool_params.py's; tests/test_pool_params_host.py asserts on the oracle alone that they
converge and need different iteration counts."""
import ctypes as C

import numpy as np
import pytest

import _gpu_case as gc
import _pool_params as pp
from aslr_to_amd import _abi, crocoddyl, scenarios
from aslr_to_amd.lowering import param_table

pytestmark = pytest.mark.gpu

_batch_cache = {}


def _batch(key, c):
    """the batched solve of the case's P problems with the table: computed once per case, shared, never modified"""
    import torch
    if key not in _batch_cache:
        e, _ = gc.solve_gpu(scenarios.lower(pp.batch_scenario(c)), c["sp"])
        _batch_cache[key] = dict(xs=e.region(_abi.R_XS).permute(1, 0, 2).contiguous().clone(),
                                 us=e.region(_abi.R_US).permute(1, 0, 2).contiguous().clone(),
                                 cost=e.traj_f(_abi.TF_COST).clone(), iters=e.traj_i(_abi.TI_ITER).clone(),
                                 status=e.traj_i(_abi.TI_STATUS).clone())
        torch.cuda.synchronize()
        e.close()
    return _batch_cache[key]


def _assert_same(r, ref, what=""):
    import torch
    for k in ("iters", "status", "cost", "xs", "us"):
        assert r[k].shape == ref[k].shape and torch.equal(r[k], ref[k]), "%s %s differs from the batch with the table" % (what, k)


def _differs_by(a, b, ratio=1.5):
    """rows of a and b differ by more than `ratio` in some joint"""
    q = a / b
    return ((q > ratio) | (q < 1.0 / ratio)).any(axis=-1)


@pytest.mark.parametrize("name", sorted(pp.CASES))
def test_pool_with_parameters_is_the_batch_with_the_table(name):
    """Every problem of the pool gets, bit for bit, the solve the batch with the table gives it: xs, us, cost, iterations and
    status, whatever the refill period and the sub-shard count.

    What keeps this from being vacuous, asserted below: P > slots, so slots are refilled, and P >= slots, so the first round
    fills every slot: its sweep is the `full` one that sets the handle's const mark, and every later refill meets launches
    that would skip the model-only record chunks.  The batch's iteration counts differ.  The result differs from the
    constant-parameter pool on most problems.  And refilled slots change design: each of the P - slots refills puts a
    problem j >= slots behind some earlier problem i < j; the two rows are independent draws, and a pair lies within 1.5x in
    BOTH joints of a 2-joint case with probability 0.25 (per joint 1 - (1 - log 1.5 / log 4)^2 = 0.50; less with 7 joints).
    The share of such (i, j) pairs that differ by more than 1.5x is asserted to be above 0.6, so that all P - slots links of
    whatever schedule the device takes avoiding them is out of the question (0.4^110 for two_dof_sea; the arms have few
    refills, 8 and 6, but seven joints: their shares are 1.00 and 0.97).
    test_one_slot_takes_a_different_design_with_every_refill makes the same point with a schedule that is known."""
    import torch
    c = pp.case(name)
    P, slots = c["P"], c["slots"]
    assert P > slots
    ref = _batch(name, c)
    assert int(ref["iters"].min()) < int(ref["iters"].max())
    Bm = c["params"]["motor_inertia"]
    pairs = [(i, j) for j in range(slots, P) for i in range(j)]
    share = np.mean([_differs_by(Bm[i], Bm[j]) for i, j in pairs])
    print("%s: %d refills, %.2f of the candidate (predecessor, problem) pairs differ by more than 1.5x in motor inertia"
          % (name, P - slots, share))
    assert share > 0.6
    sc = c["sc"]
    e = gc.engine(scenarios.lower(pp.slot_scenario(c)))
    for refill_every, nsub in c["runs"]:
        e.set_subshards(nsub)
        r = e.solve_pool(sc["x0"], sc["frame_refs"], c["sp"], refill_every=refill_every, poll_every=2 * refill_every,
                         **c["params"])
        _assert_same(r, ref, "%s refill_every=%d subshards=%d:" % (name, refill_every, nsub))
        low = e.low
        np.testing.assert_array_equal(gc.to_np(r["params"]), param_table(low.desc, low.nj, low.nu, low.dam, {
            k: np.asarray(v, dtype=np.float64) for k, v in c["params"].items()}, P))
    e.set_subshards(1)
    plain = e.solve_pool(sc["x0"], sc["frame_refs"], c["sp"], refill_every=2, poll_every=4)
    moved = (plain["xs"] != ref["xs"]).flatten(1).any(dim=1)
    print("%s: %d of %d problems differ from the constant-parameter pool" % (name, int(moved.sum()), P))
    assert int(moved.sum()) > P // 2


def test_one_slot_takes_a_different_design_with_every_refill():
    """One slot, six problems: problem j follows problem j - 1 in the slot, and its motor inertia is 2x or 1/2x its
    predecessor's (the model-only chunks Fu = dt B^-1 S and the motor rows of Fx of the slot's records are stale at every
    refill).  Equal to the batch with the table, bit for bit."""
    c = pp.case("two_dof_sea", P=6, T=10)
    Bm = c["params"]["motor_inertia"].copy()
    Bm[:] = Bm[0] * np.array([1.0, 2.0, 1.0, 0.5, 1.0, 2.0])[:, None]
    assert _differs_by(Bm[1:], Bm[:-1]).all()
    c["params"]["motor_inertia"] = c["table"]["motor_inertia"] = Bm
    ref = _batch("one_slot", c)
    e = gc.engine(scenarios.lower(pp.slot_scenario(c, 1)))
    for refill_every in (1, 4):
        r = e.solve_pool(c["sc"]["x0"], c["sc"]["frame_refs"], c["sp"], refill_every=refill_every, **c["params"])
        _assert_same(r, ref, "refill_every=%d:" % refill_every)


@pytest.mark.parametrize("name, field", [("two_dof_sea", "stiffness"), ("two_dof_sea", "motor_inertia"),
                                         ("two_dof_vsa_boxddp", "u_lb"), ("two_dof_vsa_boxddp", "u_ub")])
def test_each_field_alone(name, field):
    """one field given, the others None (the models' constants): equal to the batch solve with that one-field table"""
    c = pp.case(name, P=90, T=10, fields=(field,))
    assert set(c["params"]) == {field}
    ref = _batch((name, field), c)
    e = gc.engine(scenarios.lower(pp.slot_scenario(c, 40)))
    r = e.solve_pool(c["sc"]["x0"], c["sc"]["frame_refs"], c["sp"], refill_every=2, poll_every=4, **c["params"])
    _assert_same(r, ref, field)
    if field in ("stiffness", "motor_inertia"):   # (a scaled bound alone need not bind: -100 f on a torque, 0 f on a stiffness)
        plain = e.solve_pool(c["sc"]["x0"], c["sc"]["frame_refs"], c["sp"], refill_every=2, poll_every=4)
        assert (plain["xs"] != r["xs"]).any()


@pytest.mark.parametrize("name", ["two_dof_sea", "two_dof_vsa_boxddp"])
def test_rows_equal_to_the_constants_change_nothing(name):
    """rows that repeat the models' constants: the bits of solve_pool without parameters.  With all four keywords None the
    old entry point is called, and aslr_solve_pool_params with every field NULL returns that same function's result."""
    import torch
    c = pp.case(name, P=90, T=10)
    sc, sp = c["sc"], c["sp"]
    const = {k: v for k, v in scenarios.constant_traj_params(sc).items() if v is not None}
    e = gc.engine(scenarios.lower(pp.slot_scenario(c, 40)))
    plain = e.solve_pool(sc["x0"], sc["frame_refs"], sp, refill_every=2, poll_every=4)
    assert "params" not in plain   # (the old call path)
    r = e.solve_pool(sc["x0"], sc["frame_refs"], sp, refill_every=2, poll_every=4, **const)
    assert "params" in r
    _assert_same(r, plain, "constants:")
    none = e.solve_pool(sc["x0"], sc["frame_refs"], sp, refill_every=2, poll_every=4, stiffness=None, motor_inertia=None,
                        u_lb=None, u_ub=None)
    assert "params" not in none
    _assert_same(none, plain, "all None:")
    # the C entry point with pp == NULL and with every field NULL: aslr_solve_pool itself
    for ppar in (None, C.byref(_abi.PoolParams())):
        out = _raw_pool(e, sc, sp, ppar)
        _assert_same(out, plain, "delegated:")


def _pool_struct(e, sc, P=None):
    """the device arrays of a pool of the scenario's problems, as Engine.solve_pool makes them -> (aslr_pool_t, tensors)"""
    import torch
    dev = e.device
    x0 = torch.as_tensor(np.asarray(sc["x0"]), dtype=torch.float64, device=dev).contiguous()
    fr = torch.as_tensor(np.asarray(sc["frame_refs"]), dtype=torch.float64, device=dev).contiguous()
    P = x0.shape[0] if P is None else P
    t = dict(x0=x0, fr=fr, xs=torch.full((P, e.T + 1, e.nx), 7.0, dtype=torch.float64, device=dev),
             us=torch.full((P, e.T, e.nu), 7.0, dtype=torch.float64, device=dev),
             sf=torch.full((P, 4), 7.0, dtype=torch.float64, device=dev), si=torch.full((P, 2), 7, dtype=torch.int32, device=dev),
             slot=torch.full((e.B,), 7, dtype=torch.int32, device=dev), cnt=torch.full((2,), 7, dtype=torch.int32, device=dev))
    pool = _abi.Pool()
    pool.P = P
    pool.x0, pool.frame_ref = x0.data_ptr(), fr.data_ptr()
    pool.xs_out, pool.us_out, pool.stat_f, pool.stat_i = t["xs"].data_ptr(), t["us"].data_ptr(), t["sf"].data_ptr(), t["si"].data_ptr()
    pool.slot_problem, pool.counters = t["slot"].data_ptr(), t["cnt"].data_ptr()
    return pool, t


def _raw_pool(e, sc, sp, ppar):
    import torch
    pool, t = _pool_struct(e, sc)
    it = C.c_int32(0)
    e._call("aslr_solve_pool_params", C.byref(sp), C.byref(pool), ppar, 2, 4, e._stream(), C.byref(it))
    torch.cuda.synchronize()
    return dict(xs=t["xs"], us=e.cut_u(t["us"]), cost=t["sf"][:, 0], iters=t["si"][:, 0], status=t["si"][:, 1])


def _solve(e, sp):
    e.set_candidate(None, None)
    e.solve(sp)
    gc.sync()


def _assert_handles_equal(e, fresh):
    import torch
    for rid in (_abi.R_X0, _abi.R_XS, _abi.R_US):
        assert torch.equal(e.region(rid), fresh.region(rid)), rid
    assert torch.equal(e.traj_i(_abi.TI_ITER), fresh.traj_i(_abi.TI_ITER))
    assert torch.equal(e.traj_i(_abi.TI_STATUS), fresh.traj_i(_abi.TI_STATUS))
    assert torch.equal(e.traj_f(_abi.TF_COST), fresh.traj_f(_abi.TF_COST))


@pytest.mark.parametrize("name", ["two_dof_sea", "talos_arm_sea"])
def test_the_handle_afterwards_is_a_fresh_handle(name):
    """After a pool with parameters the handle is back on the models' constants with its own x0 / targets: a plain solve
    equals the same solve on a fresh engine (X0, XS, US, iterations, status, cost), and so does set_trajectory_params
    followed by a solve.  SEA: Fu = dt B^-1 S and the motor rows of Fx are model-only record chunks, so a const mark left
    standing after the pool would keep the last designs' chunks under the plain solve: this is the test that notices."""
    import torch
    small = dict(P=50, T=10) if name == "two_dof_sea" else dict(P=8, T=8)
    c = pp.case(name, **small)
    slots = 16 if name == "two_dof_sea" else 4
    sp = scenarios.solver_params(c["sc"], solver="SolverFDDP", maxiter=8)
    slot_sc = pp.slot_scenario(c, slots)
    e = gc.engine(scenarios.lower(slot_sc))
    _solve(e, sp)   # (a solve BEFORE the pool: the handle's const mark is set when the pool starts)
    e.solve_pool(c["sc"]["x0"], c["sc"]["frame_refs"], sp, refill_every=2, poll_every=4, **c["params"])
    _solve(e, sp)
    fresh = gc.engine(scenarios.lower(slot_sc))
    _solve(fresh, sp)
    _assert_handles_equal(e, fresh)
    plain_xs = fresh.region(_abi.R_XS).clone()
    # ... a pool without parameters on it is the pool of a fresh engine as well
    a = e.solve_pool(c["sc"]["x0"], c["sc"]["frame_refs"], sp, refill_every=2, poll_every=4)
    b = fresh.solve_pool(c["sc"]["x0"], c["sc"]["frame_refs"], sp, refill_every=2, poll_every=4)
    _assert_same(a, b, "plain pool afterwards:")
    # ... and a table set after a pool with parameters
    e.solve_pool(c["sc"]["x0"], c["sc"]["frame_refs"], sp, refill_every=2, poll_every=4, **c["params"])
    rows = {k: v[slots:2 * slots] for k, v in c["params"].items()}
    for h in (e, fresh):
        h.set_trajectory_params(**rows)
        _solve(h, sp)
    _assert_handles_equal(e, fresh)
    assert not torch.equal(e.region(_abi.R_XS), plain_xs)   # (the table made a difference)


def _host(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(C.POINTER(C.c_double))


def _refused(e, sc, sp, word, P=None, params_dev=True, psp=True, ppool=True, **fields):
    """the raw call is refused with ASLR_E_INVALID under its own name, names the cause, and writes nothing: the outputs,
    the pool scratch and params_dev keep their fill"""
    import torch
    pool, t = _pool_struct(e, sc, P)
    if P is not None and P <= 0:
        pool.P = P
    n = max(pool.P, 1)
    par = _abi.PoolParams()
    keep = []
    for k, v in fields.items():
        a, ptr = _host(v)
        keep.append(a)
        setattr(par, k, ptr)
    dev = torch.full((2 * e.low.nj + 2 * e.nu, n), 7.0, dtype=torch.float64, device=e.device)
    par.params_dev = dev.data_ptr() if params_dev else None
    it = C.c_int32(-5)
    with torch.cuda.device(e.device):
        rc = e.lib.aslr_solve_pool_params(e.handle, C.byref(sp) if psp else None, C.byref(pool) if ppool else None,
                                          C.byref(par), 2, 4, e._stream(), C.byref(it))
    torch.cuda.synchronize()
    msg = e.lib.aslr_last_error().decode()
    assert rc == _abi.E_INVALID, (rc, msg)
    assert msg.startswith("aslr_solve_pool_params:") and word in msg, msg
    assert it.value == -5
    for k in ("xs", "us", "sf"):
        assert bool((t[k] == 7.0).all()), k
    for k in ("si", "slot", "cnt"):
        assert bool((t[k] == 7).all()), k
    assert bool((dev == 7.0).all())


def test_refusals_write_nothing_and_leave_the_handle_usable():
    import torch
    c = pp.case("two_dof_sea", P=12, T=6)
    sc = c["sc"]
    sp = scenarios.solver_params(sc, solver="SolverFDDP", maxiter=6)
    slot_sc = pp.slot_scenario(c, 4)
    low = scenarios.lower(slot_sc)
    e = gc.engine(low)
    _solve(e, sp)
    before = {rid: e.region(rid).clone() for rid in (_abi.R_X0, _abi.R_XS, _abi.R_US, _abi.R_TRAJ_PARAMS, _abi.R_TRAJ_I)}
    Bm, Km = c["params"]["motor_inertia"], c["params"]["stiffness"]
    # ---- what aslr_solve_pool refuses ----
    _refused(e, sc, sp, "sp is NULL", psp=False, motor_inertia=Bm)
    _refused(e, sc, sp, "pool is NULL", ppool=False, motor_inertia=Bm)
    _refused(e, sc, sp, "pool->P", P=0, motor_inertia=Bm)
    sp_bad = scenarios.solver_params(sc, solver="SolverFDDP", maxiter=0)
    _refused(e, sc, sp_bad, "maxiter", motor_inertia=Bm)
    sp_fix = scenarios.solver_params(sc, solver="SolverFDDP", maxiter=6, fixed_iterations=1)
    _refused(e, sc, sp_fix, "fixed_iterations", motor_inertia=Bm)
    pool, t = _pool_struct(e, sc)
    pool.xs_out = None
    par = _abi.PoolParams()
    a, par.motor_inertia = _host(Bm)
    dev = torch.zeros((8, 12), dtype=torch.float64, device=e.device)
    par.params_dev = dev.data_ptr()
    with pytest.raises(_abi.AslrError, match="aslr_solve_pool_params: x0, xs_out"):
        e._call("aslr_solve_pool_params", C.byref(sp), C.byref(pool), C.byref(par), 2, 4, e._stream(), None)
    # ---- a table, a reference path, no scratch ----
    e.set_trajectory_params(motor_inertia=Bm[:4])
    _refused(e, sc, sp, "parameter table", motor_inertia=Bm)
    e.set_trajectory_params()
    via = scenarios.hold_via_points(scenarios.reference_via_points(slot_sc), 6)
    e.set_reference_path(via)
    _refused(e, sc, sp, "reference path", motor_inertia=Bm)
    e.set_reference_path(None)
    _refused(e, sc, sp, "params_dev", params_dev=False, motor_inertia=Bm)
    # ---- what aslr_set_trajectory_params refuses in a table ----
    _refused(e, sc, sp, "no model of the problem has control limits", u_lb=np.zeros((12, 2)), u_ub=np.ones((12, 2)))
    _refused(e, sc, sp, "stiffness entries must be finite", stiffness=np.where(np.arange(12)[:, None] == 11, np.nan, Km))
    _refused(e, sc, sp, "motor_inertia entries must be finite and > 0", motor_inertia=np.where(np.arange(12)[:, None] == 11, 0.0, Bm))
    _refused(e, sc, sp, "motor_inertia entries must be finite and > 0", motor_inertia=np.full((12, 2), np.inf))
    # the handle is as it was: no region moved, a plain solve is a fresh handle's, and the pool with parameters runs
    torch.cuda.synchronize()
    for rid, v in before.items():
        if rid != _abi.R_TRAJ_PARAMS:   # (set_trajectory_params above wrote the table region)
            assert torch.equal(e.region(rid), v), rid
    _solve(e, sp)
    fresh = gc.engine(low)
    _solve(fresh, sp)
    _assert_handles_equal(e, fresh)
    r = e.solve_pool(sc["x0"], sc["frame_refs"], sp, **c["params"])
    assert r["xs"].shape[0] == 12 and bool(torch.isfinite(r["cost"]).all())
    # ---- VSA: stiffness, bounds out of order; models that differ in a field left out; K not diagonal ----
    cv = pp.case("two_dof_vsa_boxddp", P=6, T=5)
    scv, spv = cv["sc"], scenarios.solver_params(cv["sc"], maxiter=5)
    ev = gc.engine(scenarios.lower(pp.slot_scenario(cv, 4)))
    _refused(ev, scv, spv, "VSA", stiffness=np.ones((6, 2)))
    _refused(ev, scv, spv, "u_lb <= u_ub", u_lb=np.full((6, 4), 200.0))
    _refused(ev, scv, spv, "u_lb <= u_ub", u_lb=np.zeros((6, 4)), u_ub=np.full((6, 4), np.nan))
    cs = pp.case("two_dof_sea", P=6, T=5)
    s3 = dict(cs["sc"])
    s3["terminal"].differential.B = 2.0 * np.asarray(s3["terminal"].differential.B)
    e3 = gc.engine(scenarios.lower(pp.slot_scenario(cs, 4)))
    _refused(e3, s3, sp, "differ in B", stiffness=np.ones((6, 2)))
    low4 = scenarios.lower(pp.slot_scenario(pp.case("two_dof_sea", P=6, T=5), 4))
    for i in range(low4.desc.nmodels):
        low4.desc.models[i].K[1] = low4.desc.models[i].K[2] = 1e-3
    e4 = gc.engine(low4)
    _refused(e4, cs["sc"], sp, "diagonal", motor_inertia=np.ones((6, 2)))
    # a solver the size is not built for
    c7 = pp.case("talos_arm_vsa", P=3, T=4)
    e7 = gc.engine(scenarios.lower(pp.slot_scenario(c7, 2)))
    sp7 = scenarios.solver_params(c7["sc"], solver="SolverFDDP", maxiter=4)
    _refused(e7, c7["sc"], sp7, "SolverBoxDDP", motor_inertia=c7["params"]["motor_inertia"])


def test_python_facade_and_shape_checks():
    """SolverFDDP.solve_pool(..., stiffness=, motor_inertia=) end to end, and the host-side shape check of the rows"""
    c = pp.case("two_dof_sea", P=20, T=8)
    sc = c["sc"]
    ref = _batch("facade", c)
    slot_sc = pp.slot_scenario(c, 8)
    problem = crocoddyl.ShootingProblem(slot_sc["x0"], slot_sc["running"], slot_sc["terminal"], frame_refs=slot_sc["frame_refs"])
    solver = crocoddyl.SolverFDDP(problem)
    solver.th_stop = sc["th_stop"]
    r = solver.solve_pool(sc["x0"], sc["frame_refs"], maxiter=c["sp"].maxiter, refill_every=2, poll_every=4, **c["params"])
    _assert_same(r, ref, "facade:")
    with pytest.raises(ValueError, match="one row per pool problem"):
        solver.solve_pool(sc["x0"], sc["frame_refs"], maxiter=5, motor_inertia=c["params"]["motor_inertia"][:8])
