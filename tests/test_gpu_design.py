"""aslr_design_descent on the GPU (include/aslr_to_amd_design.h; design_step_kernel, csrc/aslr_design.hip): the step kernel
alone against the numpy rule of tests/_design.py bit for bit, the whole call against the same loop driven from the host
through aslr_set_trajectory_params / aslr_solve / aslr_cost_sensitivity on a second engine bit for bit, against the CPU-oracle
loop of tests/test_design_host.py within the project's parity bounds, the state the call leaves on the handle, the refusals
and the Python facade."""
import copy
import ctypes as C

import numpy as np
import pytest

import _design as D
import _ext_call as ext
import _gpu_case as gc
from aslr_to_amd import _abi, crocoddyl, scenarios

pytestmark = pytest.mark.gpu

def _table(e):
    import torch
    r = _abi.Region()
    _abi.check(e.lib.aslr_problem_region(e.handle, _abi.R_TRAJ_PARAMS, C.byref(r)), "aslr_problem_region")
    return e.ws[r.offset:r.offset + r.bytes].view(torch.float64).view(2 * (e.nx // 4) + 2 * e.nu, e.B)


class _Buffers(object):
    """every buffer of an aslr_design_t, sentinel-filled, and the struct that points at them"""

    def __init__(self, e, n_steps, lo, hi, history=True):
        import torch
        nj, B, T = e.nx // 4, e.B, e.T
        n = max(int(n_steps), 1)
        shapes = dict(theta_best=(2 * nj, B), cost_best=(B,), xs_best=(T + 1, B, e.nx), us_best=(T, B, e.nu), g_acc=(2 * nj, B),
                      eta=(B,), grad=(2 * nj, B))
        if history:
            shapes.update(hist_f=(n, 3, B), theta_hist=(n, 2 * nj, B))
        self.t = {k: torch.full(s, ext.SENTINEL, dtype=torch.float64, device=e.device) for k, s in shapes.items()}
        if history:
            self.t["hist_i"] = torch.full((n, B), -77, dtype=torch.int32, device=e.device)
        self.t["lo"] = torch.as_tensor(np.ascontiguousarray(lo), dtype=torch.float64, device=e.device)
        self.t["hi"] = torch.as_tensor(np.ascontiguousarray(hi), dtype=torch.float64, device=e.device)
        self.outputs = [k for k in self.t if k not in ("lo", "hi")]

    def struct(self, c, **over):
        d = _abi.Design()
        d.n_steps, d.first_maxiter, d.iters_per_step = c["n_steps"], c["first_maxiter"], c["iters_per_step"]
        d.opt_stiffness, d.opt_motor_inertia = int("K" in c["fields"]), int("B" in c["fields"])
        p = dict(D.DEFAULTS, eta0=c["eta0"], max_rel=c["max_rel"])
        d.eta0, d.grow, d.shrink, d.c1, d.max_rel = p["eta0"], p["grow"], p["shrink"], p["c1"], p["max_rel"]
        for k, t in self.t.items():
            setattr(d, k, t.data_ptr())
        for k, v in over.items():
            setattr(d, k, v)
        return d

    def untouched(self):
        for k in self.outputs:
            t = self.t[k]
            assert bool((t == (-77 if t.dtype != self.t["eta"].dtype else ext.SENTINEL)).all()), "%s was written by a refused call" % k

    def np(self):
        return {k: gc.to_np(t) for k, t in self.t.items()}


def _descend(e, sp, c, bufs, expect=_abi.OK, **over):
    import torch
    d = bufs.struct(c, **over)
    with torch.cuda.device(e.device):
        rc = e.lib.aslr_design_descent(e.handle, C.byref(sp), C.byref(d), e._stream())
    gc.sync()
    if expect != _abi.OK:
        assert rc == expect, rc
        return e.lib.aslr_last_error().decode()
    assert rc == _abi.OK, e.lib.aslr_last_error().decode()
    return bufs.np()


class _GpuBackend(object):
    """the loop of tests/_design.run through the entry points that existed before aslr_design_descent, on an engine of its own"""

    def __init__(self, e, sp):
        self.e, self.sp = e, copy.copy(sp)
        self.nj, self.vsa = e.nx // 4, e.low.dam == _abi.DAM_VSA

    def solve(self, theta, xs, us, iterations, feasible):
        e, nj = self.e, self.nj
        e.set_trajectory_params(stiffness=None if self.vsa else np.ascontiguousarray(theta[:nj].T),
                                motor_inertia=np.ascontiguousarray(theta[nj:].T))
        gc._upload(e, XS=xs, US=us)
        for rid in (_abi.R_KFF, _abi.R_GAPS, _abi.R_VXXF):
            e.region(rid).zero_()
        self.sp.maxiter, self.sp.is_feasible = int(iterations), int(feasible)
        e.solve(self.sp, poll_every=0)
        gc.sync()
        return gc.to_np(e.region(_abi.R_XS)), gc.to_np(e.region(_abi.R_US)), gc.to_np(e.traj_f(_abi.TF_COST))

    def gradient(self, theta, xs, us, active):
        import torch
        e, nj = self.e, self.nj
        g = torch.zeros((2 * nj, e.B), dtype=torch.float64, device=e.device)
        pk = C.c_void_p(g.data_ptr()) if active[0] else None
        pb = C.c_void_p(g[nj:].data_ptr()) if active[nj] else None
        with torch.cuda.device(e.device):
            rc = e.lib.aslr_cost_sensitivity(e.handle, pk, pb, None, None, e._stream())
        assert rc == _abi.OK, e.lib.aslr_last_error().decode()
        gc.sync()
        return gc.to_np(g)


def _host_loop(c, sp, subshards=1):
    host = gc.engine(c["low"])
    if subshards > 1:
        host.set_subshards(subshards)
    low = c["low"]
    r = D.run(_GpuBackend(host, sp), c["theta0"], np.zeros((low.T + 1, low.B, low.nx)), np.zeros((low.T, low.B, low.nu)),
              c["active"], c["lo"], c["hi"], c["n_steps"], c["first_maxiter"], c["iters_per_step"], eta0=c["eta0"], max_rel=c["max_rel"])
    # the host loop ends like the call: the accepted design in the table, the best plan in XS / US
    nj = low.nj
    th = r["state"]["theta"]
    host.set_trajectory_params(stiffness=None if low.dam == _abi.DAM_VSA else np.ascontiguousarray(th[:nj].T),
                               motor_inertia=np.ascontiguousarray(th[nj:].T))
    return host, r


def _device_run(c, sp, subshards=1):
    e = gc.engine(c["low"])
    if subshards > 1:
        e.set_subshards(subshards)
    e.set_candidate(None, None)
    bufs = _Buffers(e, c["n_steps"], c["lo"], c["hi"])
    return e, _descend(e, sp, c, bufs)


# ---- (a) the step kernel alone ----
@pytest.mark.parametrize("name, B, fields", [("two_dof_sea", 3, "KB"), ("two_dof_sea", 65, "KB"), ("talos_arm_sea", 3, "KB"),
                                             ("talos_arm_sea", 65, "KB"), ("two_dof_sea", 65, "K"), ("two_dof_sea", 65, "B")])
def test_step_kernel_matches_the_numpy_rule_bit_for_bit(name, B, fields):
    """design_step_kernel launched alone on random state, T = 4, at (nx, nu) = (8, 2) and (28, 7), B = 3 and 65 (more than one
    wave's worth of blocks, a column stride that is no multiple of anything): s = 0 with a trajectory whose cost is NaN (it
    freezes) and one whose gradient is Inf, a middle step and a last step with a frozen trajectory, accepted and rejected
    ones.  Every buffer the kernel writes, the TRAJ_PARAMS column, XS / US in both directions, the zeroed regions.  With one
    field optimised the rows of the other are inactive: their theta, g_acc and table rows stay as they were, their theta_hist
    rows repeat theta."""
    import torch
    T = 4
    sc = scenarios.with_traj_params(scenarios.SCENARIOS[name](B=B, T=T, seed=1), seed=5)
    low = scenarios.lower(sc)
    e = gc.engine(low)
    lib = e.lib
    lib.aslr_debug_design_step.restype = C.c_int
    lib.aslr_debug_design_step.argtypes = [C.c_void_p, C.POINTER(_abi.Design), C.c_int32, C.c_int32, C.c_void_p]
    nj, nx, nu = low.nj, low.nx, low.nu
    rng = np.random.default_rng(3)
    th0 = D.theta0_of(low)
    lo, hi = th0 / 1.5, th0 * 1.5
    c = dict(n_steps=1, first_maxiter=1, iters_per_step=1, fields=fields, eta0=0.7, max_rel=0.3)
    p = dict(D.DEFAULTS, eta0=0.7, max_rel=0.3)
    active = np.array([("K" in fields)] * nj + [("B" in fields)] * nj)
    for s, last in ((0, False), (2, False), (2, True)):
        st = D.new_state(th0 * rng.uniform(0.8, 1.2, th0.shape), T, nx, nu)
        st["theta"] = np.clip(st["theta"], lo, hi)
        st["cost"] = rng.uniform(50.0, 60.0, B)
        st["g_acc"] = rng.uniform(-1.0, 1.0, (2 * nj, B)) / st["theta"]
        st["eta"] = rng.uniform(0.1, 2.0, B)
        st["xs_best"], st["us_best"] = rng.uniform(-1, 1, (T + 1, B, nx)), rng.uniform(-1, 1, (T, B, nu))
        J = st["cost"] + rng.uniform(-3.0, 3.0, B)
        grad = rng.uniform(-1.0, 1.0, (2 * nj, B))
        xs, us = rng.uniform(-1, 1, (T + 1, B, nx)), rng.uniform(-1, 1, (T, B, nu))
        J[1] = np.nan
        grad[nj if "B" in fields else 0, 2] = np.inf
        grad[~active] = np.nan   # (rows of a field that is not optimised are not read)
        if s > 0:
            st["eta"][0] = -1.0   # frozen
        bufs = _Buffers(e, 1, lo, hi)
        for k in ("theta", "cost", "g_acc", "eta", "xs_best", "us_best"):
            key = {"theta": "theta_best", "cost": "cost_best"}.get(k, k)
            bufs.t[key].copy_(torch.as_tensor(st[k]))
        bufs.t["grad"].copy_(torch.as_tensor(grad))
        gc._upload(e, XS=xs, US=us)
        e.region(_abi.R_TRAJ_F)[_abi.TF_COST].copy_(torch.as_tensor(J))
        for rid in (_abi.R_KFF, _abi.R_GAPS, _abi.R_VXXF):
            e.region(rid).fill_(3.5)
        before = rng.uniform(1.0, 2.0, tuple(_table(e).shape))
        _table(e).copy_(torch.as_tensor(before))
        d = bufs.struct(c)
        with torch.cuda.device(e.device):
            assert lib.aslr_debug_design_step(e.handle, C.byref(d), s, int(last), e._stream()) == _abi.OK
        gc.sync()
        want = D.step(st, s, last, J, grad, xs, us, active, lo, hi, **p)
        got = bufs.np()
        what = "%s B=%d %s s=%d last=%d: " % (name, B, fields, s, last)
        if B > 3:   # (the case is not empty: frozen or not evaluable, accepted, and after s = 0 rejected trajectories)
            assert set(np.unique(want["flag"])) == ({-1, 0, 1} if s > 0 else {-1, 1}), want["flag"]
        for k, key in (("theta", "theta_best"), ("cost", "cost_best"), ("g_acc", "g_acc"), ("eta", "eta"), ("xs_best", "xs_best"),
                       ("us_best", "us_best")):
            ext.same(got[key], st[k], what + key)
        ext.same(got["hist_f"][0], want["hist_f"], what + "hist_f")
        np.testing.assert_array_equal(got["hist_i"][0], want["flag"], err_msg=what + "hist_i")
        ext.same(got["theta_hist"][0], want["theta_try"], what + "theta_hist")
        ext.same(gc.to_np(e.region(_abi.R_XS)), want["xs"], what + "XS")
        ext.same(gc.to_np(e.region(_abi.R_US)), want["us"], what + "US")
        tab = before.copy()
        tab[:2 * nj][active] = want["table"][active]
        assert np.isnan(want["table"][~active]).all() and not np.isnan(want["table"][active]).any()
        ext.same(gc.to_np(_table(e)), tab, what + "TRAJ_PARAMS (the box rows untouched)")
        for rid in (_abi.R_KFF, _abi.R_GAPS, _abi.R_VXXF):
            assert not gc.to_np(e.region(rid)).view(np.int64).any(), what + "region %d is not all zero" % rid


# ---- (b) the whole call is the host-driven loop ----
WHOLE = [("sea_KB", 1), ("sea_KB", 2), ("sea_K", 1), ("sea_B", 1), ("vsa_B", 1), ("talos_sea_KB", 1), ("talos_vsa_B", 1)]


def _assert_call_equals_loop(c, e, got, host, r, what):
    st = r["state"]
    ext.same(got["theta_best"], st["theta"], what + "theta_best")
    ext.same(got["cost_best"], st["cost"], what + "cost_best")
    ext.same(got["xs_best"], st["xs_best"], what + "xs_best")
    ext.same(got["us_best"], st["us_best"], what + "us_best")
    ext.same(got["hist_f"], r["hist_f"], what + "hist_f")
    np.testing.assert_array_equal(got["hist_i"], r["flag"], err_msg=what + "hist_i")
    ext.same(got["theta_hist"], r["theta_hist"], what + "theta_hist")
    ext.same(gc.to_np(e.region(_abi.R_XS)), r["xs"], what + "XS")
    ext.same(gc.to_np(e.region(_abi.R_US)), r["us"], what + "US")
    ext.same(gc.to_np(_table(e)), gc.to_np(_table(host)), what + "TRAJ_PARAMS")
    for rid in (_abi.R_TRAJ_F, _abi.R_TRAJ_I):   # those of the last step's solve
        gc.same_bits(e.region(rid), host.region(rid), what + "region %d" % rid)


@pytest.mark.parametrize("name, subshards", WHOLE)
def test_the_call_equals_the_host_driven_loop_bit_for_bit(name, subshards):
    c = D.case(name)
    sp = c["sp"]
    e, got = _device_run(c, sp, subshards)
    host, r = _host_loop(c, sp, subshards)
    print("%s: flags %s" % (name, r["flag"].T.tolist()))
    _assert_call_equals_loop(c, e, got, host, r, "%s, %d sub-shard(s): " % (name, subshards))
    assert (r["flag"][0] == 1).all() and np.abs(r["theta_hist"][-1] - c["theta0"]).max() > 0.0   # the design moved


# ---- (c) against the CPU-oracle loop ----
@pytest.mark.parametrize("name", D.ORACLE_CASES)
def test_the_call_follows_the_oracle_loop(oracle, name):
    """the accept / reject sequence of the oracle loop exactly (tests/test_design_host.py keeps every decision away from
    rounding); theta_best within 1e-6 and cost_best within 1e-4 in absolute difference: the parity bounds of
    tests/test_gpu_headline.py (tests/_parity.compare)"""
    c = D.case(name)
    low = c["low"]
    ref = D.run(D.OracleBackend(oracle, c["sc"], c["sp"]), c["theta0"], np.zeros((low.T + 1, low.B, low.nx)),
                np.zeros((low.T, low.B, low.nu)), c["active"], c["lo"], c["hi"], c["n_steps"], c["first_maxiter"],
                c["iters_per_step"], eta0=c["eta0"], max_rel=c["max_rel"])
    e, got = _device_run(c, c["sp"])
    np.testing.assert_array_equal(got["hist_i"], ref["flag"])
    dth = float(np.abs(got["theta_best"] - ref["state"]["theta"]).max())
    dc = float(np.abs(got["cost_best"] - ref["state"]["cost"]).max())
    print("%s: max |theta_best - oracle| %.2e, max |cost_best - oracle| %.2e" % (name, dth, dc))
    assert dth < 1e-6, dth
    assert dc < 1e-4, dc


# ---- (d) the handle afterwards ----
@pytest.mark.parametrize("name", ["sea_KB", "vsa_B"])
def test_the_handle_is_left_on_the_accepted_design(name):
    """a solve and a sensitivity sweep on the handle after the call equal those of a fresh engine that was given theta_acc
    through aslr_set_trajectory_params, from the same candidate: a forgotten re-arm of the model-only record chunks or a
    stale host copy of the table shows here"""
    import torch
    c = D.case(name)
    sp = copy.copy(c["sp"])
    e, got = _device_run(c, sp)
    nj, vsa = c["low"].nj, c["low"].dam == _abi.DAM_VSA
    fresh = gc.engine(c["low"])
    fresh.set_trajectory_params(stiffness=None if vsa else np.ascontiguousarray(got["theta_best"][:nj].T),
                                motor_inertia=np.ascontiguousarray(got["theta_best"][nj:].T))
    gc._upload(fresh, XS=got["xs_best"], US=got["us_best"])
    sp.maxiter = 5
    outs = []
    for h in (e, fresh):
        h.solve(sp, poll_every=0)
        s = h.cost_sensitivity()
        gc.sync()
        outs.append((s, [gc.to_np(h.region(r)) for r in ext.SOLVE_REGIONS]))
    for a, b, rid in zip(outs[0][1], outs[1][1], ext.SOLVE_REGIONS):
        np.testing.assert_array_equal(a.view(np.int64) if a.dtype == np.float64 else a, b.view(np.int64) if b.dtype == np.float64 else b,
                                      err_msg="region %d of a solve after the call" % rid)
    for k in ("motor_inertia", "x0", "costate") + (() if vsa else ("stiffness",)):
        gc.same_bits(getattr(outs[0][0], k), getattr(outs[1][0], k), "d%s after the call" % k)
    # ... and the table can be set again from the host afterwards
    e.set_trajectory_params(motor_inertia=np.ascontiguousarray(got["theta_best"][nj:].T))


# ---- (e) refusals ----
def test_refusals_write_nothing_and_leave_the_handle_solving():
    import torch
    c = D.case("sea_KB")
    low, sp = c["low"], c["sp"]
    _, fresh = gc.solve_gpu(low, sp)
    e = gc.engine(low)
    bufs = _Buffers(e, c["n_steps"], c["lo"], c["hi"])

    def refused(words, sp_=sp, c_=c, e_=e, bufs_=bufs, **over):
        msg = _descend(e_, sp_, c_, bufs_, expect=_abi.E_INVALID, **over)
        assert msg.startswith("aslr_design_descent:") and all(w in msg for w in words), msg
        bufs_.untouched()

    d0 = bufs.struct(c)
    assert e.lib.aslr_design_descent(e.handle, None, C.byref(d0), e._stream()) == _abi.E_INVALID
    assert e.lib.aslr_last_error().decode().startswith("aslr_design_descent:")
    assert e.lib.aslr_design_descent(e.handle, C.byref(sp), None, e._stream()) == _abi.E_INVALID
    assert e.lib.aslr_last_error().decode().startswith("aslr_design_descent:")
    for k in ("lo", "hi", "theta_best", "cost_best", "xs_best", "us_best", "g_acc", "eta", "grad"):
        refused(["must be given"], **{k: None})
    for k in ("n_steps", "first_maxiter", "iters_per_step"):
        refused([">= 1"], **{k: 0})
    refused(["neither"], opt_stiffness=0, opt_motor_inertia=0)
    for k, bad in (("eta0", 0.0), ("eta0", float("nan")), ("grow", 0.5), ("shrink", 1.0), ("shrink", 0.0), ("c1", 0.0), ("c1", 1.0),
                   ("max_rel", 0.0), ("max_rel", 1.0)):
        refused([k], **{k: bad})
    # bounds: lo = 0, lo > hi, NaN; an initial design outside them
    for mutate, words in ((lambda lo, hi: lo.__setitem__((0, 1), 0.0), ["bounds"]),
                          (lambda lo, hi: hi.__setitem__((2, 0), lo[2, 0] * 0.5), ["bounds"]),
                          (lambda lo, hi: hi.__setitem__((1, 2), float("nan")), ["bounds"]),
                          (lambda lo, hi: lo.__setitem__((3, 1), c["theta0"][3, 1] * 1.01), ["initial design", "outside"])):
        lo, hi = c["lo"].copy(), c["hi"].copy()
        mutate(lo, hi)
        b2 = _Buffers(e, c["n_steps"], lo, hi)
        refused(words, bufs_=b2)
    # an iteration log that is set
    e.enable_iteration_log(8)
    refused(["iteration log"])
    e.enable_iteration_log(0)
    # a stiffness of 0 in the initial design
    tp = {k: v for k, v in c["sc"]["traj_params"].items() if v is not None}
    zero = np.array(tp["stiffness"])
    zero[1, 0] = 0.0
    e.set_trajectory_params(**dict(tp, stiffness=zero))
    refused(["not positive"])
    e.set_trajectory_params(**tp)
    # opt_stiffness on a VSA model; the (7, VSA) handle with SolverDDP; non-diagonal B
    cv = D.case("vsa_B")
    ev = gc.engine(cv["low"])
    bv = _Buffers(ev, cv["n_steps"], cv["lo"], cv["hi"])
    refused(["VSA"], sp_=cv["sp"], c_=cv, e_=ev, bufs_=bv, opt_stiffness=1)
    c7 = D.case("talos_vsa_B")
    e7 = gc.engine(c7["low"])
    b7 = _Buffers(e7, c7["n_steps"], c7["lo"], c7["hi"])
    refused(["SolverBoxDDP only"], sp_=scenarios.solver_params(c7["sc"], solver="SolverDDP"), c_=c7, e_=e7, bufs_=b7)
    sc = scenarios.two_dof_sea(B=2, T=4, seed=1)
    m = copy.copy(sc["running"][0])   # (shallow: the robot model stays shared with the terminal model)
    m.differential = copy.copy(m.differential)
    m.differential.B = np.array(m.differential.B, dtype=float) + np.array([[0.0, 1e-4], [1e-4, 0.0]])
    lowd = scenarios.lower(dict(sc, running=[m] * 4))
    ed = gc.engine(lowd)
    th = np.ones((4, 2))
    bd = _Buffers(ed, 2, th * 1e-6, th * 1e6)
    refused(["diagonal"], sp_=scenarios.solver_params(sc), c_=dict(c, n_steps=2), e_=ed, bufs_=bd)
    mk = copy.copy(sc["running"][0])
    mk.differential = copy.copy(mk.differential)
    mk.differential.K = np.array(mk.differential.K, dtype=float) + np.array([[0.0, 1e-3], [1e-3, 0.0]])
    ek = gc.engine(scenarios.lower(dict(sc, running=[mk] * 4)))
    bk = _Buffers(ek, 2, th * 1e-6, th * 1e6)
    refused(["diagonal"], sp_=scenarios.solver_params(sc), c_=dict(c, n_steps=2), e_=ek, bufs_=bk)
    # the first handle still solves to the bits of a fresh one
    e.set_candidate(None, None)
    e.solve(sp)
    gc.sync()
    after = gc.solution(e)
    for k in ("xs", "us", "traj_i"):
        np.testing.assert_array_equal(after[k], fresh[k], err_msg=k)


# ---- (f) the Python facade ----
def test_python_facade():
    """solver.optimize_design on sea_KB and vsa_B: the documented shapes, None stiffness for VSA, the bits of the raw call,
    solver.xs on the accepted design; scalar and [nj] bounds are broadcast; the models' constants as the initial design"""
    for name in ("sea_KB", "vsa_B"):
        c = D.case(name)
        sc, low = c["sc"], c["low"]
        nj, B, T, vsa = low.nj, low.B, low.T, low.dam == _abi.DAM_VSA
        _, raw = _device_run(c, c["sp"])
        tp = sc.get("traj_params") or {}
        problem = crocoddyl.ShootingProblem(sc["x0"], sc["running"], sc["terminal"], frame_refs=sc["frame_refs"],
                                            stiffness=tp.get("stiffness"), motor_inertia=tp.get("motor_inertia"))
        solver = getattr(crocoddyl, sc["solver"])(problem)
        solver.th_stop = c["sp"].th_stop
        kb = None if vsa else (c["lo"][:nj].T, c["hi"][:nj].T)
        r = solver.optimize_design(c["n_steps"], c["iters_per_step"], maxiter=c["first_maxiter"], stiffness_bounds=kb,
                                   motor_inertia_bounds=(c["lo"][nj:].T, c["hi"][nj:].T), eta0=c["eta0"], max_rel=c["max_rel"],
                                   keep_history=True)
        assert (r.stiffness is None) == vsa
        if not vsa:
            assert tuple(r.stiffness.shape) == (B, nj) and tuple(r.stiffness_history.shape) == (B, c["n_steps"], nj)
            ext.same(gc.to_np(r.stiffness), raw["theta_best"][:nj].T, "stiffness")
        assert tuple(r.motor_inertia.shape) == (B, nj) and tuple(r.cost.shape) == (B,)
        assert tuple(r.xs.shape) == (B, T + 1, low.nx) and tuple(r.us.shape) == (B, T, problem.engine.nu_user)
        assert tuple(r.accepted_history.shape) == (B, c["n_steps"]) and tuple(r.motor_inertia_history.shape) == (B, c["n_steps"], nj)
        ext.same(gc.to_np(r.motor_inertia), raw["theta_best"][nj:].T, "motor_inertia")
        ext.same(gc.to_np(r.cost), raw["cost_best"], "cost")
        ext.same(gc.to_np(r.xs), raw["xs_best"].transpose(1, 0, 2), "xs")
        np.testing.assert_array_equal(gc.to_np(r.accepted_history), raw["hist_i"].T)
        ext.same(gc.to_np(solver.xs), gc.to_np(r.xs), "solver.xs is the accepted plan")
        ext.same(problem.lowered.traj_params["motor_inertia"], gc.to_np(r.motor_inertia), "the problem's table")
    # scalar bounds, no table: the models' constants are the initial design
    sc = scenarios.two_dof_sea(B=3, T=6, seed=2)
    problem = crocoddyl.ShootingProblem(sc["x0"], sc["running"], sc["terminal"], frame_refs=sc["frame_refs"])
    solver = crocoddyl.SolverFDDP(problem)
    r = solver.optimize_design(2, 2, maxiter=10, stiffness_bounds=(1e-3, 1e6), motor_inertia_bounds=None)
    m0 = D.theta0_of(scenarios.lower(sc))
    ext.same(gc.to_np(r.motor_inertia), m0[2:].T, "motor inertia is not optimised: the models' constant")
    assert float((r.stiffness - problem.engine.region(_abi.R_XS).new_tensor(m0[:2].T)).abs().max()) > 0.0
    with pytest.raises(_abi.AslrError, match="outside its bounds"):
        solver.optimize_design(2, 2, maxiter=10, stiffness_bounds=(1e-3, 1e-2))
