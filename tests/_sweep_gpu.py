"""The bodies that the GPU suites of the policy-sweep calls share (tests/test_gpu_covariance.py, test_gpu_plant_sens.py,
test_gpu_lqg.py; tests/test_gpu_sensitivity.py where one fits), imported like _mpc_plant_gpu (`import _sweep_gpu as sw`).  A
suite keeps its argument list (`_raw`), its reference and whatever only its call has.

`call(e, which=None, expect=OK)` is the suite's `_raw` with the case's input arrays bound; `call_for(b)` is the same with
the inputs cut to trajectory b.  each_output_alone takes the call with the engine bound as well.  The bodies that work on
dicts of numpy arrays alone are held to firing when they must by tests/test_sweep_gpu_host.py, on a CPU."""
import numpy as np

import _covariance as cv
import _ext_call as ext
import _gpu_case as gc
import _traj_oracle
from aslr_to_amd import _abi, crocoddyl

POLICY_REGIONS = (_abi.R_XS, _abi.R_US, _abi.R_KGAIN)


def make_cases(oracle, keys, extend=None):
    """key -> the seeded inputs of the case (tests/_covariance.case: the open-loop candidate comes from the oracle), built once
    and never changed; extend(c) adds what a suite needs beside them"""
    made = {}
    for key in keys:
        made[key] = cv.case(oracle, key)
        if extend is not None:
            extend(made[key])
    return made


def make_loaded(cases):
    """-> get(key) -> (engine with the candidate and its gains in place, the device's K), made on first use and shared: the
    call under test changes nothing it reads"""
    made = {}

    def get(key):
        if key not in made:
            made[key] = ext.with_gains(cases[key])
        return made[key]
    return get


def matches(got, want, fields, label):
    """every field: the reference's shape, and within 1e-9 of it in max |a - b| / max |b| per trajectory (cv.traj_relerr: a
    trajectory whose reference is all zero must match exactly).  Prints the figure."""
    for k in fields:
        assert got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
        err = cv.traj_relerr(got[k], want[k])
        print("%s %s: %.2e (max |reference| %.2e)" % (label, k, err, np.abs(want[k]).max()))
        assert err < 1e-9, (k, err)


def zero_gain_rows(key, K, got):
    """gains after a BoxDDP backward sweep (K [T, B, nu, nx]): some rows are zero, and so is their variance"""
    if key in ("vsa_box", "arm_vsa"):
        zero = np.abs(K).max(axis=-1) == 0.0
        assert zero.any() and not zero.all()
        assert (got["u_var"].transpose(1, 0, 2)[zero] == 0.0).all()


def padded_control(key, got):
    if key == "nu1":
        assert (got["u_var"][..., 1] == 0.0).all()   # the padded control


def each_output_alone(call, full):
    """each output alone: the bits of the call with all of them (and nothing written past any buffer: the guarded call
    checks the guards)"""
    for k in full:
        ext.same(call(which=(k,)), {k: full[k]}, "alone")


def trajectory_alone(c, e, K, call, call_for):
    """trajectory B - 1 of the batch on `e` (the one behind the last full wave of teams) against the same trajectory alone in
    a B = 1 engine (tests/_traj_oracle.single: its row of the table in the models) with the batch's candidate and gains
    uploaded: bit for bit"""
    low = c["low"]
    batch = call(e)
    b = low.B - 1
    e1 = gc.engine(_traj_oracle.single(low, b))
    gc._upload(e1, XS=c["xs"][:, b:b + 1], US=c["us"][:, b:b + 1], KGAIN=K[:, b:b + 1])
    alone = call_for(b)(e1)
    ext.same({k: v[0] for k, v in alone.items()}, {k: v[b] for k, v in batch.items()}, "trajectory %d" % b)


def side_effects_of_calc_diff(c, call):
    """3 iterations, the call, 3 more iterations: XS, US, TRAJ_F and TRAJ_I are, bit for bit, those of 3 iterations,
    aslr_calc_diff, 3 iterations on a fresh engine"""
    low, sp = c["low"], c["sp"]
    runs = []
    for step in (call, lambda e: e.calc_diff()):
        e = gc.engine(low)
        e.set_candidate(None, None)
        e.iterate_n(sp, True, 3)
        step(e)
        e.iterate_n(sp, False, 3)
        gc.sync()
        runs.append(gc.solution(e))
    assert (runs[1]["traj_i"][_abi.TI_ITER] > 3).any()
    for k in runs[0]:
        np.testing.assert_array_equal(runs[0][k], runs[1][k], err_msg=k)


def stored_policy_round_trip(problem, e, facade_call, want):
    """facade_call(problem, xs, us, K) at the engine's policy, stored and given explicitly while the engine holds another:
    the bits of `want` (field -> tensor), and the engine's own policy is back afterwards -> the stored xs, us, K"""
    xs, us, K = (e.region(r).clone() for r in POLICY_REGIONS)
    for r in POLICY_REGIONS:
        e.region(r).fill_(0.25)
    again = facade_call(problem, xs.permute(1, 0, 2), us.permute(1, 0, 2), K.permute(1, 0, 2, 3))
    for k, ref in want.items():
        gc.same_bits(getattr(again, k), ref, "the stored policy given explicitly")
    for r in POLICY_REGIONS:
        assert (e.region(r) == 0.25).all()
    return xs, us, K


def padded_controls_are_cut(cases, facade_call):
    """facade_call(solver) on the nu1 case after 3 iterations: u_var has the user's one control"""
    c = cases["nu1"]
    sc, T = c["sc"], c["low"].T
    solver = crocoddyl.SolverDDP(crocoddyl.ShootingProblem(sc["x0"], sc["running"], sc["terminal"], frame_refs=sc["frame_refs"]))
    solver.solve([], [], 3)
    r1 = facade_call(solver)
    gc.sync()
    assert tuple(r1.u_var.shape) == (3, T, 1) and tuple(r1.x_var.shape) == (3, T + 1, 8)
