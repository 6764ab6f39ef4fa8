"""aslr_plant_identify on the GPU (include/aslr_to_amd_identify.h; csrc/aslr_identify.inc.hpp): the normal-equation kernel
against the definition of tests/_identify.py, the step kernel alone against its numpy mirror bit for bit, the whole call
against the same loop driven from the host through the older entry points, against the reference loop, the recovery of the
true plant, batch independence, the state the call leaves on the handle, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import _ext_call as ext
import _gpu_case as gc
import _identify as I
from aslr_to_amd import _abi, crocoddyl, scenarios

pytestmark = pytest.mark.gpu
NAMES = sorted(I.CASES)


def _table(e):
    import torch
    r = _abi.Region()
    _abi.check(e.lib.aslr_problem_region(e.handle, _abi.R_TRAJ_PARAMS, C.byref(r)), "aslr_problem_region")
    return e.ws[r.offset:r.offset + r.bytes].view(torch.float64).view(2 * (e.nx // 4) + 2 * e.nu, e.B)


def _debug(lib):
    lib.aslr_debug_identify_step.restype = C.c_int
    lib.aslr_debug_identify_step.argtypes = [C.c_void_p, C.POINTER(_abi.Identify), C.c_int32, C.c_int32, C.c_void_p]
    lib.aslr_debug_identify_normal.restype = C.c_int
    lib.aslr_debug_identify_normal.argtypes = [C.c_void_p, C.POINTER(_abi.Identify), C.c_void_p]


def _shapes(B, npar, n):
    nh = npar * (npar + 1) // 2
    return dict(theta=(npar, B), sse=(B,), grad=(npar, B), information=(nh, B), mu=(B,), identifiable=(npar, B), n_accepted=(B,),
                hist_theta=(n, npar, B), hist_sse=(n, B), hist_decision=(n, B), work=(2 * npar + 1 + nh, B))


INT32 = ("identifiable", "n_accepted", "hist_decision")


def _struct(e, outs, fields, n_steps, lo, hi, p, weights=None, keep=None, **over):
    d = _abi.Identify()
    d.n_steps, d.fit_stiffness, d.fit_motor_inertia = n_steps, int("K" in fields), int("B" in fields)
    for k in ("mu0", "mu_min", "mu_max", "grow", "shrink", "max_rel", "min_curv"):
        setattr(d, k, p[k])
    tl, th, tw = ext.dev(e.device, lo), ext.dev(e.device, hi), ext.dev(e.device, weights)
    d.lo, d.hi, d.weights = tl.data_ptr(), th.data_ptr(), None if tw is None else tw.data_ptr()
    for k, o in outs.items():
        setattr(d, k, o.buf.data_ptr())
    for k, v in over.items():
        setattr(d, k, v)
    if keep is not None:
        keep.extend([tl, th, tw])
    return d


def _engine(c, theta=None, rows=None):
    """a fresh engine on the case's scenario (trajectories `rows`), Y / U in XS / US, the table on theta (default theta_0)"""
    low, fields = c["low"], c["fields"]
    sc = c["sc"]
    if rows is not None:
        sc = dict(sc, x0=np.asarray(sc["x0"])[rows], frame_refs=None if sc.get("frame_refs") is None else np.asarray(sc["frame_refs"])[rows],
                  traj_params={k: (None if v is None else np.asarray(v)[rows]) for k, v in sc["traj_params"].items()})
        if sc.get("B") is not None:
            sc["B"] = len(rows)
        low = scenarios.lower(sc)
    rows = list(range(c["low"].B)) if rows is None else list(rows)
    e = gc.engine(low)
    gc._upload(e, XS=c["Y"][:, rows], US=c["U"][:, rows])
    _set_theta(e, c, c["theta0"][:, rows] if theta is None else theta, rows)
    return e


def _set_theta(e, c, theta, rows=None):
    nj = c["low"].nj
    rows = list(range(c["low"].B)) if rows is None else rows
    k, bm = I.split(theta, nj, c["fields"])
    vsa = c["low"].dam == _abi.DAM_VSA
    e.set_trajectory_params(stiffness=None if vsa else np.ascontiguousarray((c["start_k"][:, rows] if k is None else k).T),
                            motor_inertia=np.ascontiguousarray((c["start_b"][:, rows] if bm is None else bm).T))


def _call(e, c, n_steps, lo=None, hi=None, expect=_abi.OK, weights=None, which=None, fields=None, p=None, null=(), **over):
    fields = fields or c["fields"]
    npar = I.n_params(c["low"].nj, fields)
    lo, hi = (c["lo"] if lo is None else lo), (c["hi"] if hi is None else hi)
    outs = ext.outputs(e.device, _shapes(e.B, npar, max(n_steps, 1)), which or list(_shapes(1, 1, 1)), int32=INT32)
    keep = []
    d = _struct(e, outs, fields, n_steps, lo, hi, p or I.params(c), weights, keep, **over)
    for k in null:   # a NULL pointer where the struct wants a buffer
        setattr(d, k, None)
    return ext.call(e, "aslr_plant_identify", [e.handle, C.byref(d), e._stream()], outs, expect)


# ---- 1. the normal kernel against the definition ----
@pytest.mark.parametrize("name", NAMES)
def test_normal_kernel_matches_the_definition(oracle, name):
    """theta 10 % off the truth (seeded signs), weights seeded in (0.5, 2): sse, grad and information within 1e-9 in the
    project's relerr, per array; through the call with n_steps = 1, which also leaves theta as the accepted set"""
    c = I.case(oracle, name)
    rng = np.random.default_rng(5)
    theta = c["truth"] * (1.0 + 0.1 * rng.choice([-1.0, 1.0], c["truth"].shape))
    w = rng.uniform(0.5, 2.0, (c["low"].B, c["low"].nx))
    want = I.definition(oracle, c, theta, w)
    e = _engine(c, theta)
    got = _call(e, c, 1, lo=theta / 2, hi=theta * 2, weights=np.ascontiguousarray(w.T))
    for k, ref in zip(("sse", "grad", "information"), want):
        err = gc.relerr(got[k], ref)
        print("%s %s: relerr %.2e (max |reference| %.2e)" % (name, k, err, np.abs(ref).max()))
        assert err < 1e-9, (k, err)
    ext.same(got["theta"], theta, "theta")
    assert (got["n_accepted"] == 1).all() and (got["hist_decision"] == 1).all() and (got["identifiable"] == 1).all()


# ---- 2. the step kernel alone ----
@pytest.mark.parametrize("name, B", [("two_dof_sea", 5), ("two_dof_sea", 65), ("two_dof_vsa_boxddp", 5), ("talos_arm_sea", 5), ("talos_arm_vsa", 5)])
def test_step_kernel_matches_the_numpy_mirror_bit_for_bit(name, B):
    """identify_step_kernel launched alone on seeded state: s = 0 with a trajectory whose sse is NaN (it freezes), a middle
    step with accepted, rejected and frozen trajectories, one whose H is indefinite (failed pivots: mu grows until the damping
    carries it), one with a zero diagonal entry (masked parameter), and a last step.  Every buffer the kernel writes and the
    TRAJ_PARAMS column."""
    import torch
    low = scenarios.lower(scenarios.with_traj_params(scenarios.SCENARIOS[name](B=B, T=3, seed=1), seed=5))
    e = gc.engine(low)
    _debug(e.lib)
    nj = low.nj
    fields = "B" if low.dam == _abi.DAM_VSA else "KB"
    npar = I.n_params(nj, fields)
    nh = npar * (npar + 1) // 2
    rng = np.random.default_rng(3)
    p = dict(I.DEFAULTS, mu0=0.5, max_rel=0.3, min_curv=1e-9)
    for s, last in ((0, False), (2, False), (2, True)):
        th = rng.uniform(0.5, 2.0, (npar, B))
        lo, hi = th / 1.2, th * 1.2
        st = I.new_state(th)
        st["theta_try"] = np.clip(th * rng.uniform(0.7, 1.4, th.shape), lo, hi)
        st["sse"], st["mu"] = rng.uniform(1.0, 2.0, B), 10.0 ** rng.integers(-6, 2, B).astype(float)
        st["n_accepted"] = rng.integers(1, 3, B).astype(np.int32)

        def spd():
            M = rng.uniform(-1, 1, (B, npar, 2 * npar))
            return np.stack([I.pack(M[b] @ M[b].T) for b in range(B)], axis=1)
        st["info"], st["grad"] = spd(), rng.uniform(-1, 1, (npar, B))
        h_try, g_try = spd(), rng.uniform(-1, 1, (npar, B))
        sse_try = st["sse"] + rng.uniform(-0.5, 0.5, B)
        sse_try[1] = np.nan
        if s > 0:
            st["mu"][0] = -1.0   # frozen
        # trajectory 2: indefinite (a large off-diagonal entry), accepted or not it is what the solve sees
        for arr in (st["info"], h_try):
            arr[I._at(1, 0), 2] = 50.0 * np.sqrt(arr[I._at(0, 0), 2] * arr[I._at(1, 1), 2])
        # trajectory 3: parameter 1 has no curvature
        for arr in (st["info"], h_try):
            for q in range(npar):
                arr[I._at(max(1, q), min(1, q)), 3] = 0.0
        outs = ext.outputs(e.device, _shapes(B, npar, 1), list(_shapes(1, 1, 1)), int32=INT32)
        d = _struct(e, outs, fields, 1, lo, hi, p, keep=[])
        put = lambda k, v: outs[k].buf[:v.size].copy_(torch.as_tensor(np.ascontiguousarray(v).reshape(-1)))
        for k, key in (("theta", "theta"), ("sse", "sse"), ("grad", "grad"), ("information", "info"), ("mu", "mu"), ("n_accepted", "n_accepted")):
            put(k, st[key])
        put("work", np.concatenate([st["theta_try"], sse_try[None], g_try, h_try]))
        before = rng.uniform(1.0, 2.0, tuple(_table(e).shape))
        _table(e).copy_(torch.as_tensor(before))
        with torch.cuda.device(e.device):
            assert e.lib.aslr_debug_identify_step(e.handle, C.byref(d), s, int(last), e._stream()) == _abi.OK
        gc.sync()
        want = I.step(st, s, last, sse_try, g_try, h_try, lo, hi, **p)
        got = {k: ext.payload(*o) for k, o in outs.items()}
        for o in outs.values():
            assert ext.guard_intact(o.buf)
        what = "%s B=%d s=%d last=%d: " % (name, B, s, last)
        if B > 5:
            assert set(np.unique(want["decision"])) == ({-1, 0, 1} if s > 0 else {-1, 1}), want["decision"]
        if not last:
            assert st["mu"][2] > 1.0, "the indefinite trajectory did not take the failed-pivot path"
            assert st["identifiable"][1, 3] == 0 and st["identifiable"][0, 3] == 1
        for k, key in (("theta", "theta"), ("sse", "sse"), ("grad", "grad"), ("information", "info"), ("mu", "mu")):
            ext.same(got[k], st[key], what + k)
        np.testing.assert_array_equal(got["identifiable"], st["identifiable"], err_msg=what + "identifiable")
        np.testing.assert_array_equal(got["n_accepted"], st["n_accepted"], err_msg=what + "n_accepted")
        np.testing.assert_array_equal(got["hist_decision"][0], want["decision"], err_msg=what + "hist_decision")
        ext.same(got["hist_theta"][0], want["theta_eval"], what + "hist_theta")
        ext.same(got["hist_sse"][0], want["sse_eval"], what + "hist_sse")
        ext.same(got["work"][:npar], want["next"], what + "the next candidate")
        r0, rows = I.table_rows(want["next"], nj, fields)
        tab = before.copy()
        tab[r0:r0 + npar] = rows
        ext.same(gc.to_np(_table(e)), tab, what + "TRAJ_PARAMS (the other rows untouched)")


# ---- 3. / 4. / 5. the whole call ----
def _device_run(c, n_steps=None, **kw):
    e = _engine(c)
    return e, _call(e, c, n_steps or c["n_steps"], **kw)


def _host_loop(c):
    """the loop of the call driven from the host through the entry points that existed before and the two debug exports:
    aslr_set_trajectory_params(candidate), aslr_calc_diff, identify_normal_kernel, identify_step_kernel -> engine, outputs"""
    import torch
    host = _engine(c)
    _debug(host.lib)
    npar, B = c["theta0"].shape
    n = c["n_steps"]
    outs = ext.outputs(host.device, _shapes(B, npar, n), list(_shapes(1, 1, 1)), int32=INT32)
    th0 = torch.as_tensor(np.ascontiguousarray(c["theta0"]).reshape(-1))
    outs["theta"].buf[:npar * B].copy_(th0)
    outs["work"].buf[:npar * B].copy_(th0)
    keep = []
    for s in range(n):
        cand = ext.payload(*outs["work"])[:npar]
        _set_theta(host, c, cand)
        host.calc_diff()
        d = _struct(host, outs, c["fields"], n, c["lo"], c["hi"], I.params(c), keep=keep)
        d.hist_theta = outs["hist_theta"].buf.data_ptr() + 8 * s * npar * B   # (the debug step takes them as those of its step)
        d.hist_sse = outs["hist_sse"].buf.data_ptr() + 8 * s * B
        d.hist_decision = outs["hist_decision"].buf.data_ptr() + 4 * s * B
        with torch.cuda.device(host.device):
            assert host.lib.aslr_debug_identify_normal(host.handle, C.byref(d), host._stream()) == _abi.OK
            assert host.lib.aslr_debug_identify_step(host.handle, C.byref(d), s, int(s == n - 1), host._stream()) == _abi.OK
        gc.sync()
    for o in outs.values():
        assert ext.guard_intact(o.buf)
    return host, {k: ext.payload(*o) for k, o in outs.items()}


@pytest.mark.parametrize("name", NAMES)
def test_the_call_equals_the_host_driven_loop_bit_for_bit(oracle, name):
    """every output, the scratch and TRAJ_PARAMS"""
    c = I.case(oracle, name)
    e, got = _device_run(c)
    host, want = _host_loop(c)
    print("%s: decisions %s" % (name, want["hist_decision"].T.tolist()))
    ext.same(got, want, name)
    ext.same(gc.to_np(_table(e)), gc.to_np(_table(host)), name + ": TRAJ_PARAMS")
    assert (want["hist_decision"] == 0).any() and (want["hist_decision"][1:] == 1).any()


@pytest.mark.parametrize("name", NAMES)
def test_the_call_follows_the_reference_loop(oracle, name):
    """the accept / reject sequence of the reference loop on the compared steps (tests/test_identify_host.py keeps those away
    from rounding); the candidates evaluated there within 1e-6 and their sse within 1e-4, relative"""
    c = I.case(oracle, name)
    ref = I.reference_run(oracle, name)
    n = I.compared_steps(ref)
    _, got = _device_run(c)
    np.testing.assert_array_equal(got["hist_decision"][:n], ref["decision"][:n])
    dth = float(np.abs(got["hist_theta"][:n] / ref["theta_hist"][:n] - 1.0).max())
    ds = float((np.abs(got["hist_sse"][:n] - ref["sse_hist"][:n]) / ref["sse_hist"][:n]).max())
    print("%s: %d compared steps, theta %.2e, sse %.2e relative" % (name, n, dth, ds))
    assert dth < 1e-6, dth
    assert ds < 1e-4, ds


@pytest.mark.parametrize("name", NAMES)
def test_truth_recovered(oracle, name):
    """N_RECOVER steps on two data sets: the oracle-made data of the case, and data made on the device -- aslr_policy_rollout
    (2 joints) / aslr_policy_rollout_all of the case's policy on the true plant from x0 + dx0, trajectories kept (no dither:
    the roll-out applies the policy as it is).  theta_acc within 16 times the recovery error the reference loop records for
    the data set (tests/_identify.RECOVERY; for the device-made data its CPU twin, the oracle's run without the dither)"""
    c = I.case(oracle, name)
    low = c["low"]
    vsa = low.dam == _abi.DAM_VSA
    _, got = _device_run(c, I.N_RECOVER)
    rec = I.recovery(c, got["theta"])
    print("%s, oracle-made data: recovery %.2e (reference %.2e)" % (name, rec, I.RECOVERY[name][0]))
    e = gc.engine(low)
    gc._upload(e, XS=c["xs"], US=c["us"], KGAIN=c["K"])
    pert = dict(plant_stiffness=None if vsa else np.ascontiguousarray(c["true_k"].T)[:, None],
                plant_motor_inertia=np.ascontiguousarray(c["true_b"].T)[:, None], dx0=c["dx0"][:, None])
    run = ext.policy_rollout(e, "aslr_policy_rollout" if low.nj == 2 else "aslr_policy_rollout_all", 1, pert)
    assert (run["failed_knot"] < 0).all()
    data = dict(c, Y=np.ascontiguousarray(run["xs"][:, 0].transpose(1, 0, 2)), U=np.ascontiguousarray(run["us"][:, 0].transpose(1, 0, 2)))
    twin = float(np.abs(data["Y"] - c["Y_plain"]).max() / np.abs(c["Y_plain"]).max())
    got2 = _call(_engine(data), data, I.N_RECOVER)
    rec2 = I.recovery(c, got2["theta"])
    print("%s, device-made data (%.1e from its CPU twin): recovery %.2e (reference %.2e)" % (name, twin, rec2, I.RECOVERY[name][1]))
    assert twin < 1e-9, twin
    assert (got["identifiable"] == 1).all() and (got2["identifiable"] == 1).all()
    assert rec < 16 * I.RECOVERY[name][0], rec
    assert rec2 < 16 * I.RECOVERY[name][1], rec2


# ---- 6. batch independence ----
@pytest.mark.parametrize("name", NAMES)
def test_a_trajectory_does_not_depend_on_the_batch(oracle, name):
    c = I.case(oracle, name)
    B = c["low"].B
    _, full = _device_run(c)
    b = B - 1
    for rows in ([b], [b, 0], [1, b, 0]):
        sub = dict(c, lo=c["lo"][:, rows], hi=c["hi"][:, rows])
        e = _engine(c, rows=rows)
        got = _call(e, sub, c["n_steps"])
        at = rows.index(b)
        for k in ("theta", "sse", "grad", "information", "mu", "identifiable", "n_accepted"):
            ext.same(got[k][..., at], full[k][..., b], "%s: %s of trajectory %d in the batch %s" % (name, k, b, rows))
        ext.same(got["hist_sse"][:, at], full["hist_sse"][:, b], "hist_sse")


# ---- 7. the handle afterwards ----
@pytest.mark.parametrize("name", NAMES)
def test_the_handle_is_left_on_the_fit(oracle, name):
    import copy
    c = I.case(oracle, name)
    e, got = _device_run(c)
    fresh = _engine(c, got["theta"])
    sp = copy.copy(c["sp"])
    sp.maxiter = 5
    outs = []
    for h in (e, fresh):
        s = h.cost_sensitivity()
        h.solve(sp, poll_every=0)
        gc.sync()
        outs.append((s, [gc.to_np(h.region(r)) for r in ext.SOLVE_REGIONS]))
    for a, b, rid in zip(outs[0][1], outs[1][1], ext.SOLVE_REGIONS):
        ext.same(a, b, "region %d of a solve after the call" % rid)
    for k in ("motor_inertia", "x0", "costate") + (() if c["low"].dam == _abi.DAM_VSA else ("stiffness",)):
        gc.same_bits(getattr(outs[0][0], k), getattr(outs[1][0], k), "d%s after the call" % k)
    _set_theta(e, c, got["theta"])   # ... and the table can be set again from the host


# ---- 8. refusals ----
def test_refusals_write_nothing(oracle):
    c = I.case(oracle, "sea")
    e = _engine(c)
    before = gc.to_np(_table(e))

    def refused(words, c_=c, e_=e, **kw):
        msg = _call(e_, c_, kw.pop("n_steps", c["n_steps"]), expect=_abi.E_INVALID, **kw)
        assert msg.startswith("aslr_plant_identify:") and all(w in msg for w in words), msg

    assert e.lib.aslr_plant_identify(e.handle, None, e._stream()) == _abi.E_INVALID
    assert e.lib.aslr_last_error().decode().startswith("aslr_plant_identify:")
    refused([">= 1"], n_steps=0)
    refused(["neither"], fit_stiffness=0, fit_motor_inertia=0)
    for k in ("lo", "hi", "theta", "sse", "grad", "information", "mu", "identifiable", "n_accepted", "work"):
        refused(["must be given"], null=(k,))
    for k, bad in (("mu0", 0.0), ("mu0", float("nan")), ("mu_min", 0.0), ("mu_max", float("inf")), ("grow", 1.0), ("shrink", 1.0),
                   ("shrink", 0.0), ("max_rel", 0.0), ("max_rel", 1.0), ("min_curv", -1.0), ("min_curv", 1.0)):
        refused([k], p=dict(I.params(c), **{k: bad}))
    for mutate, words in ((lambda lo, hi: lo.__setitem__((0, 1), 0.0), ["bounds"]),
                          (lambda lo, hi: hi.__setitem__((2, 0), lo[2, 0] * 0.5), ["bounds"]),
                          (lambda lo, hi: hi.__setitem__((1, 2), float("nan")), ["bounds"]),
                          (lambda lo, hi: lo.__setitem__((3, 1), c["theta0"][3, 1] * 1.01), ["initial parameters", "outside"])):
        lo, hi = c["lo"].copy(), c["hi"].copy()
        mutate(lo, hi)
        refused(words, lo=lo, hi=hi)
    ext.same(gc.to_np(_table(e)), before, "TRAJ_PARAMS after the refusals")
    cv = I.case(oracle, "vsa")
    ev = _engine(cv)
    th = np.concatenate([cv["theta0"], cv["theta0"]])
    refused(["VSA"], c_=dict(cv, lo=th / 2, hi=th * 2), e_=ev, fields="KB")
    import copy
    sc = scenarios.two_dof_sea(B=2, T=4, seed=1)
    m = copy.copy(sc["running"][0])
    m.differential = copy.copy(m.differential)
    m.differential.B = np.array(m.differential.B, dtype=float) + np.array([[0.0, 1e-4], [1e-4, 0.0]])
    ed = gc.engine(scenarios.lower(dict(sc, running=[m] * 4)))
    one = np.ones((4, 2))
    refused(["diagonal"], c_=dict(c, lo=one * 1e-6, hi=one * 1e6), e_=ed)
    # a non-positive stiffness in the initial table
    tp = {k: v for k, v in c["sc"]["traj_params"].items() if v is not None}
    zero = np.array(tp["stiffness"])
    zero[1, 0] = 0.0
    e.set_trajectory_params(**dict(tp, stiffness=zero))
    refused(["not positive"])


# ---- the Python facade ----
def test_python_facade(oracle):
    c = I.case(oracle, "sea")
    sc, low = c["sc"], c["low"]
    nj, B = low.nj, low.B
    _, raw = _device_run(c)
    problem = crocoddyl.ShootingProblem(sc["x0"], sc["running"], sc["terminal"], frame_refs=sc.get("frame_refs"),
                                        stiffness=c["start_k"].T, motor_inertia=c["start_b"].T)
    p = I.params(c)
    r = problem.identify_plant(c["Y"].transpose(1, 0, 2), c["U"].transpose(1, 0, 2)[..., :problem.nu], n_steps=c["n_steps"],
                               stiffness_bounds=(c["lo"][:nj].T, c["hi"][:nj].T), motor_inertia_bounds=(c["lo"][nj:].T, c["hi"][nj:].T),
                               mu0=p["mu0"], grow=p["grow"], shrink=p["shrink"], max_rel=p["max_rel"], min_curv=p["min_curv"],
                               keep_history=True)
    ext.same(gc.to_np(r.stiffness), raw["theta"][:nj].T, "stiffness")
    ext.same(gc.to_np(r.motor_inertia), raw["theta"][nj:].T, "motor_inertia")
    ext.same(gc.to_np(r.sse), raw["sse"], "sse")
    np.testing.assert_array_equal(gc.to_np(r.n_accepted), raw["n_accepted"])
    info = gc.to_np(r.information)
    assert info.shape == (B, 2 * nj, 2 * nj) and (info == info.transpose(0, 2, 1)).all()
    ext.same(info, I.unpack(raw["information"], 2 * nj).transpose(2, 0, 1), "information")
    assert gc.to_np(r.identifiable).all() and tuple(r.decision_history.shape) == (B, c["n_steps"])
    ext.same(problem.lowered.traj_params["motor_inertia"], gc.to_np(r.motor_inertia), "the problem's table")
