"""The backward sweep when the trajectories of one wave part ways: some fail (and, in a solve, retry at a larger x_reg or stop at
the ceiling) while their neighbours in the same wave publish, are already done, or lie past the end of the batch.  The
inputs and why they are what they are: tests/_mixed_waves.py; their properties on the oracle alone:
tests/test_mixed_waves_host.py.

What a failed STANDALONE sweep leaves behind (both kernels agree, include/aslr_to_amd.h states it): ST_BACKWARD_ERR in
TI_STATUS; TF_D1 / D2 / STOP untouched; the rows of K, k, Qu, Vx, Vxx of the knots ABOVE the failing one as a successful
sweep writes them (Vx / Vxx of the terminal knot included), the failing knot's rows and every row below it untouched.

Tolerances: 1e-8 relative on the outputs of a sweep, as test_backward_pass_matches_oracle (the surviving trajectories'
records are the ones that test uses); solves: counts, status words and every logged x_reg exactly, xs / us within 1e-6 of
the trajectory's size where that stays below 1e6, the bound and mask of test_backward_error_recovery_and_reg_max_match_oracle."""
import numpy as np
import pytest

import _gpu_case as gc
import _mixed_waves as mw
from aslr_to_amd import _abi, scenarios

pytestmark = pytest.mark.gpu

ROWS = ("K", "k", "Qu", "Vx", "Vxx")


def _decomposition(monkeypatch, hs=0, mfma=None):
    if hs:
        monkeypatch.setenv("ASLR_BWD_HS", str(hs))
    else:
        monkeypatch.delenv("ASLR_BWD_HS", raising=False)
    if mfma is not None:
        monkeypatch.setenv("ASLR_BLK_MFMA", mfma)


def _run_and_check(c, label):
    """One standalone sweep of the case into sentinel-filled outputs: the survivors against the oracle, the failed
    trajectories' leftovers, and that nothing of a survivor was left unwritten.  -> run_backward's dict, the survivors' mask"""
    low = c["low"]
    out = gc.run_backward(gc.engine(low), c["sp"], c["us"], c["deriv"], c["gaps"], c["xreg"], c["feasible"], k0=c["k0"],
                          prefill=mw.SENTINEL)
    print("%s: %d of %d trajectories fail" % (label, (c["ref"]["fail"] != 0).sum(), low.B))
    fddp = c["sp"].solver == _abi.SOLVER_FDDP
    # (the oracle's d1, d2 are dg, dq under SolverFDDP, gap terms included: the kernel's TF_DG / TF_DQ.  Only the comparison
    #  takes them under those names; the written / not written checks below read every raw row under its own.)
    ok = gc.assert_backward_matches_where_ok(dict(out, d1=out["dg"], d2=out["dq"]) if fddp else out, c["ref"], 1e-8)
    untouched_k = (lambda a, t, b: (a[t, b] == c["k0"][t, b]).all()) if c["k0"] is not None else None
    for name in ("d1", "d2", "stop") + (("dg", "dq") if fddp else ()):
        assert not gc.wrote(out[name], mw.SENTINEL)[~ok].any(), "%s of a failed trajectory was written" % name
        assert gc.wrote(out[name], mw.SENTINEL)[ok].all(), "%s of a surviving trajectory was not written" % name
    for name in ROWS:
        w = gc.wrote(out[name], mw.SENTINEL)
        if not (name == "k" and untouched_k):
            assert w[:, ok].all(), "%s of a surviving trajectory keeps the sentinel" % name
        for b in np.nonzero(~ok)[0]:
            tb = c["tb"][b]
            above = out[name][tb + 1:, b]       # (Vx / Vxx: up to the terminal knot T)
            if above.size:
                # (the oracle's rows above the failing knot are those of the untouched records: the host test)
                gc._assert_close("%s of failed trajectory %d above knot %d" % (name, b, tb), above, c["clean"][name][tb + 1:, b], 1e-8)
            for t in range(tb + 1):
                if name == "k" and untouched_k:
                    assert untouched_k(out[name], t, b), "k of failed trajectory %d, knot %d <= %d, was written" % (b, t, tb)
                else:
                    assert not w[t, b].any(), "%s of failed trajectory %d, knot %d <= %d, was written" % (name, b, t, tb)
    _check_vxxf(c, out, ok, fddp)
    return out, ok


def _check_vxxf(c, out, ok, fddp):
    """R_VXXF (`Vxx f`, what SolverFDDP's rollout reads): written only by SolverFDDP's sweep of an infeasible trajectory,
    there at the terminal knot and at every knot above the failing one (all of them on a survivor), within 1e-8 of the
    oracle's Vxx times the gap over 1 + |Vxx| |f| (the measure of test_gpu_forward_seam); everything else keeps the sentinel."""
    w = gc.wrote(out["Vxxf"], mw.SENTINEL)
    T = c["low"].T
    V = c["clean"]["Vxx"].astype(np.longdouble)
    want = np.einsum("tbij,tbj->tbi", V, c["gaps"].astype(np.longdouble)).astype(np.float64)
    sens = np.einsum("tbij,tbj->tbi", np.abs(V), np.abs(c["gaps"]).astype(np.longdouble)).astype(np.float64)
    worst = 0.0
    for b in range(c["low"].B):
        first = 0 if ok[b] else c["tb"][b] + 1       # first knot a sweep of this trajectory writes
        if not (fddp and c["feasible"][b] == 0):
            first = T + 1
        assert not w[:first, b].any(), "Vxx f of trajectory %d was written below knot %d" % (b, first)
        assert w[first:, b].all(), "Vxx f of trajectory %d keeps the sentinel at or above knot %d" % (b, first)
        if first <= T:
            worst = max(worst, (np.abs(out["Vxxf"][first:, b] - want[first:, b]) / (1.0 + sens[first:, b])).max())
    print("Vxx f relerr %.2e" % worst)
    assert worst < 1e-8


@pytest.mark.parametrize("scen,solver", mw.KERNEL_CASES)
@pytest.mark.parametrize("flags", ["a", "b"])
@pytest.mark.parametrize("hs", [0, 1, 2, 4])
def test_standalone_sweep_with_mixed_failures_matches_oracle(oracle, monkeypatch, scen, solver, flags, hs):
    """nx = 8, B = 19, T = 6: 3 of 19 ("ends") and 13 of 19 ("dense") trajectories fail, at the first, the last and a middle
    knot of the sweep, with x_reg 1e-3 / 1e-1 and the feasibility flags mixed inside the waves.  SolverBoxDDP: controls in the
    box, a random stored k; the infeasible trajectories carry gaps (SolverFDDP: with its expected-improvement terms)."""
    _decomposition(monkeypatch, hs)
    for mask_name in sorted(mw.MASKS):
        c = mw.kernel_case(oracle, scen, solver, flags, mask_name)
        _run_and_check(c, "%s %s flags %s hs %d mask %s" % (scen, solver, flags, hs, mask_name))


@pytest.mark.parametrize("vsa", [False, True])
def test_block_kernel_with_a_failing_trajectory_between_two_that_succeed(oracle, monkeypatch, vsa):
    """nx = 28, B = 3, T = 4, the block-per-trajectory kernel with the MFMA and the vector-FMA products: each against the oracle,
    and bit-equal to each other on the surviving trajectories (as test_gpu_vsa7 holds them on clean inputs)."""
    c = mw.arm_case(oracle, vsa)
    outs = []
    for mfma in ("1", "0"):
        _decomposition(monkeypatch, 0, mfma)
        out, ok = _run_and_check(c, "7-joint %s blk mfma %s" % ("VSA BoxDDP" if vsa else "SEA FDDP", mfma))
        outs.append(out)
    for name in gc.BACKWARD_FIELDS:
        np.testing.assert_array_equal(gc.per_trajectory(outs[0][name], ok), gc.per_trajectory(outs[1][name], ok), err_msg=name)


@pytest.mark.parametrize("hs", [1, 2])
def test_register_column_kernel_with_a_failing_trajectory_between_two_that_succeed(oracle, monkeypatch, hs):
    """The same SEA inputs through the register-column kernel at nx = 28 (one 32- or 64-lane team per wave)."""
    _decomposition(monkeypatch, hs)
    _run_and_check(mw.arm_case(oracle, False), "7-joint SEA FDDP hs %d" % hs)


@pytest.mark.parametrize("name", sorted(mw.SOLVE_CASES))
def test_retry_ladder_in_a_solve_matches_oracle_in_every_decomposition(oracle, monkeypatch, name):
    """Solves in which every sweep fails until x_reg has grown, by amounts that differ inside every wave (and, vsa_boxddp, with
    trajectories that stop at the ceiling beside ones that go on): exact counts, status words and logged x_reg."""
    sc, low, sp = mw.solve_case(name)
    ref = mw.solve_ref(oracle, name)
    mag = np.maximum(np.abs(ref["xs"]).max(axis=(0, 2)), np.abs(ref["us"]).max(axis=(0, 2)))
    tame = mag < 1e6
    assert tame.any()
    scale = np.maximum(1.0, mag)[tame]
    got = {}
    for hs in (1, 2, 4, 0):
        _decomposition(monkeypatch, hs)
        _, g = gc.solve_gpu(low, sp, log_cap=sp.maxiter)
        np.testing.assert_array_equal(g["traj_i"][_abi.TI_ITER], ref["traj_i"][_abi.TI_ITER])
        np.testing.assert_array_equal(g["traj_i"][_abi.TI_STATUS], ref["traj_i"][_abi.TI_STATUS])
        np.testing.assert_array_equal(g["log"][:, _abi.LOG_XREG], ref["log"][:, _abi.LOG_XREG])
        np.testing.assert_allclose(g["traj_f"][_abi.TF_XREG], ref["traj_f"][_abi.TF_XREG], rtol=0)
        dx = (np.abs(g["xs"] - ref["xs"])[:, tame].max(axis=(0, 2)) / scale).max()
        du = (np.abs(g["us"] - ref["us"])[:, tame].max(axis=(0, 2)) / scale).max()
        print("%s hs %d: %d tame trajectories, relerr xs %.2e us %.2e" % (name, hs, tame.sum(), dx, du))
        assert dx < 1e-6 and du < 1e-6
        got[hs] = g
    for hs in (2, 4, 0):
        for row in (_abi.TI_ITER, _abi.TI_STATUS):
            np.testing.assert_array_equal(got[hs]["traj_i"][row], got[1]["traj_i"][row])
        np.testing.assert_array_equal(got[hs]["log"][:, _abi.LOG_XREG], got[1]["log"][:, _abi.LOG_XREG])


GAIN_REGIONS = (_abi.R_KGAIN, _abi.R_KFF, _abi.R_VX, _abi.R_VXX)


def _columns(e, sel, regions):
    import torch
    idx = torch.as_tensor(np.nonzero(sel)[0], device=e.device)
    return [e.region(r).index_select(1, idx).clone() for r in regions]


SENTINEL_REGIONS = (_abi.R_KGAIN, _abi.R_VX, _abi.R_VXX)   # nothing reads these columns of a trajectory that is done


def _spoil_columns(e, sel):
    """the sentinel into the done trajectories' gains and value function: a sweep that stores anything for them -- even the
    bits it stored before, recomputed from the same records -- now shows"""
    import torch
    idx = torch.as_tensor(np.nonzero(sel)[0], device=e.device)
    for r in SENTINEL_REGIONS:
        e.region(r).index_fill_(1, idx, mw.SENTINEL)


def _columns_keep_the_sentinel(e, sel, what):
    for r, now in zip(SENTINEL_REGIONS, _columns(e, sel, SENTINEL_REGIONS)):
        assert not gc.wrote(gc.to_np(now), mw.SENTINEL).any(), "%s: region %d of a finished trajectory was written" % (what, r)


def _same_columns(e, sel, regions, saved, what):
    for r, now, s in zip(regions, _columns(e, sel, regions), saved):
        gc.same_bits(now, s, "%s: region %d of a finished trajectory changed" % (what, r))


@pytest.mark.parametrize("hs", [1, 2, 4])
def test_a_trajectory_stopped_at_reg_max_is_not_touched_by_its_retrying_neighbours(oracle, monkeypatch, hs):
    """vsa_boxddp: trajectory 12 stops at the ceiling in the backward sweep of its third iteration (TI_ITER = 2) while 13 (its
    pair, 5 iterations), 14 15 (its group of 4) and 8..11 go on.  Its columns of the gains, the value function, XS / US and TRAJ_F / TRAJ_I
    after that iteration are bit-equal after the next one; then its gains and value function are overwritten with a sentinel,
    which the two remaining iterations must leave in place (whatever rows its ride-along sweep computes before it fails again, only the
    store predicates keep them from being stored), with everything else still bit-equal."""
    _decomposition(monkeypatch, hs)
    sc, low, sp = mw.solve_case("vsa_boxddp")
    ref = mw.solve_ref(oracle, "vsa_boxddp")
    early = ((ref["traj_i"][_abi.TI_STATUS] & _abi.ST_REG_MAX) != 0) & (ref["traj_i"][_abi.TI_ITER] == 2)
    assert early.tolist() == [b == 12 for b in range(low.B)] and ref["traj_i"][_abi.TI_ITER][13] == 5
    e = gc.engine(low)
    e.set_candidate(None, None)
    e.iterate_n(sp, True, 3)
    gc.sync()
    done = gc.to_np(e.traj_i(_abi.TI_DONE)) != 0
    np.testing.assert_array_equal(done, early)      # (nothing else has finished yet on the oracle either)
    regions = GAIN_REGIONS + (_abi.R_XS, _abi.R_US, _abi.R_TRAJ_F, _abi.R_TRAJ_I)
    saved = _columns(e, early, regions)
    e.iterate_n(sp, False, 1)
    gc.sync()
    _same_columns(e, early, regions, saved, "hs %d" % hs)
    _spoil_columns(e, early)
    e.iterate_n(sp, False, 2)
    gc.sync()
    _columns_keep_the_sentinel(e, early, "hs %d" % hs)
    rest = [r for r in regions if r not in SENTINEL_REGIONS]
    _same_columns(e, early, rest, [s for r, s in zip(regions, saved) if r not in SENTINEL_REGIONS], "hs %d" % hs)
    np.testing.assert_array_equal(gc.to_np(e.traj_i(_abi.TI_ITER)), ref["traj_i"][_abi.TI_ITER])   # the neighbours did go on


# Iterations after which the warm trajectories below are done on the device, in every decomposition.  The oracle needs one:
# its own solution is gap-free for it.  Under the kernels' rounding the same candidate has gaps of an ulp, above th_gaptol =
# 1e-16, so the first iteration runs infeasible and the second converges.
N_DONE_WARM = 2


@pytest.mark.parametrize("hs", [1, 2, 4])
def test_a_converged_trajectory_is_not_touched_by_its_iterating_neighbours(oracle, monkeypatch, hs):
    """two_dof_sea under SolverFDDP, B = 19, T = 20: the even trajectories start from the oracle's converged solution and
    converge within an iteration or two, the odd ones start cold beside them and need more.  A converged trajectory's gains,
    value function and TRAJ_F / TRAJ_I (but TI_ACCEPTED) are final with the iteration in which it finishes; its accepted
    candidate is committed into XS / US, and TI_ACCEPTED reset, by the sweeps of the NEXT iteration, so those are taken one
    iteration later.  All of it is bit-equal after two more iterations of the neighbours; then the gains and value function
    are overwritten with a sentinel, which two further iterations must leave in place (the ride-along sweep of a converged
    trajectory succeeds on unchanged records: storing it again would rewrite the same bits and show in nothing else)."""
    import torch
    _decomposition(monkeypatch, hs)
    sc = scenarios.two_dof_sea(B=mw.SOLVE_B, T=mw.SOLVE_T, seed=1)
    low = scenarios.lower(sc)
    sp = scenarios.solver_params(sc, solver="SolverFDDP")
    full = oracle.solve(low, sp)
    assert ((full["traj_i"][_abi.TI_STATUS] & _abi.ST_CONVERGED) != 0).all()
    warm = np.arange(low.B) % 2 == 0
    xs, us = np.where(warm[None, :, None], full["xs"], 0.0), np.where(warm[None, :, None], full["us"], 0.0)
    ref = oracle.solve(low, sp, xs=xs, us=us)
    n_warm = int(ref["traj_i"][_abi.TI_ITER][warm].max())
    assert n_warm + 5 <= ref["traj_i"][_abi.TI_ITER][~warm].min()      # every cold neighbour still iterates at the end
    e = gc.engine(low)
    e.set_candidate(xs.transpose(1, 0, 2), us.transpose(1, 0, 2))
    # (a candidate that is gap-free for the oracle has gaps of an ulp under the kernels' rounding, above th_gaptol = 1e-16: the
    #  warm trajectories may need one iteration more than the oracle's n_warm to turn feasible and converge)
    for n_done in range(1, n_warm + 3):
        e.iterate_n(sp, n_done == 1, 1)
        gc.sync()
        if (gc.to_np(e.traj_i(_abi.TI_DONE))[warm] != 0).all():
            break
    print("hs %d: the warm trajectories are done after %d iterations (oracle: %d)" % (hs, n_done, n_warm))
    assert n_done == N_DONE_WARM
    np.testing.assert_array_equal(gc.to_np(e.traj_i(_abi.TI_DONE)) != 0, warm)
    assert ((gc.to_np(e.traj_i(_abi.TI_STATUS))[warm] & _abi.ST_CONVERGED) != 0).all()
    first = GAIN_REGIONS + (_abi.R_TRAJ_F,)
    saved = _columns(e, warm, first)
    rows = torch.as_tensor([r for r in range(_abi.TI_COUNT) if r != _abi.TI_ACCEPTED], device=e.device)
    saved_ti = _columns(e, warm, (_abi.R_TRAJ_I,))[0].index_select(0, rows)
    e.iterate_n(sp, False, 1)
    gc.sync()
    later = (_abi.R_XS, _abi.R_US, _abi.R_TRAJ_I)
    saved_later = _columns(e, warm, later)
    e.iterate_n(sp, False, 1)
    gc.sync()
    _same_columns(e, warm, first, saved, "hs %d" % hs)
    _same_columns(e, warm, later, saved_later, "hs %d" % hs)
    _spoil_columns(e, warm)
    e.iterate_n(sp, False, 2)
    gc.sync()
    _columns_keep_the_sentinel(e, warm, "hs %d" % hs)
    _same_columns(e, warm, (_abi.R_KFF, _abi.R_TRAJ_F), [saved[1], saved[4]], "hs %d" % hs)
    _same_columns(e, warm, later, saved_later, "hs %d" % hs)
    gc.same_bits(_columns(e, warm, (_abi.R_TRAJ_I,))[0].index_select(0, rows), saved_ti, "TRAJ_I of a converged trajectory changed")
    it = gc.to_np(e.traj_i(_abi.TI_ITER))
    assert (it[~warm] == n_done + 4).all() and (it[warm] <= n_done).all()
