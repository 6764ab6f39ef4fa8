"""The GPU side of tests/_mpc_plant.py: the assertion bodies that tests/test_gpu_mpc_plant.py (aslr_mpc_run_plant, 2 joints)
and tests/test_gpu_mpc_plant_team.py (aslr_mpc_run_plant_all, the 7-joint arms) share.  A test builds its case -- scenario,
`low`, `sp`, plants, disturbance, the reference -- and calls the check; nothing here depends on the model size.

`raw` is the suite's own `_raw`: ext.mpc_run_plant under the suite's entry point,
raw(e, sp, n, first, per, hold=1, pk=None, pb=None, dist=None, clamp=False, cost=True, failed=True)."""
import numpy as np

import _ext_call as ext
import _gpu_case as gc
import _mpc_plant as mp
import _parity
import _policy as pol
from aslr_to_amd import _abi, scenarios


def one_step_leaves_the_shifted_plan(e, twin, low, got, X, U, hold, clamp, row_before):
    """after ONE control step of `hold` knots on `e` (outputs `got`) and a plain solve on `twin` (plan X, U): the first
    records are the plan's knot 0; the shift, exactly: rows of the twin's plan, the last one repeated; x+ in xs[0], X0 and
    x_closed[N]; KFF, GAPS, VXXF zero; the twin's statistics; the reference row `hold` further"""
    ext.same(got["x"][0], X[0], "x_closed[0] is XS[0]")
    if not clamp:
        ext.same(got["u"][0], U[0], "u_closed[0] is US[0]")
    xs_want, us_want = mp.shifted(X, U, hold, got["x"][hold])
    XS, US = gc.to_np(e.region(_abi.R_XS)), gc.to_np(e.region(_abi.R_US))
    ext.same(XS[1:], xs_want[1:], "XS after the shift, away from row 0")
    ext.same(US, us_want, "US after the shift")
    ext.same(XS[0], got["x"][hold], "xs[0] = x_closed[N]")
    ext.same(gc.to_np(e.region(_abi.R_X0)), got["x"][hold], "X0 = x_closed[N]")
    for rid in (_abi.R_KFF, _abi.R_GAPS, _abi.R_VXXF):
        assert not gc.to_np(e.region(rid)).view(np.int64).any(), "region %d is not all zero" % rid
    tf, ti = gc.to_np(twin.region(_abi.R_TRAJ_F)), gc.to_np(twin.region(_abi.R_TRAJ_I))
    for i, row in enumerate((_abi.TF_COST, _abi.TF_STOP, _abi.TF_XREG, _abi.TF_STEP)):
        ext.same(got["stat_f"][0, i], tf[row], "stat_f[%d]" % i)
    ext.same(got["stat_i"][0, 0], ti[_abi.TI_ITER], "iterations")
    ext.same(got["stat_i"][0, 1], ti[_abi.TI_STATUS], "status")
    if getattr(low, "ref_path", None) is not None:
        assert e.reference_row == row_before + hold


def the_loop_is_its_own_step(raw, low, sp, n, hold, first, per, pk, pb, dist, label):
    """one call of n control steps against n calls of one on a twin handle: records, statistics and the regions bit for bit,
    the closed cost against the in-order sum of the steps' within 1e-12 -> (the handle, the twin)"""
    dev, twin = ext.fresh(low), ext.fresh(low)
    one = raw(dev, sp, n, first, per, hold, pk, pb, dist)
    parts = [raw(twin, sp, 1, first if s == 0 else per, per, hold, pk, pb, dist[s * hold:(s + 1) * hold]) for s in range(n)]
    for s, p in enumerate(parts):
        ext.same(one["x"][s * hold:(s + 1) * hold + 1], p["x"], "x_closed of step %d" % s)
        ext.same(one["u"][s * hold:(s + 1) * hold], p["u"], "u_closed of step %d" % s)
        ext.same(one["stat_f"][s], p["stat_f"][0], "stat_f of step %d" % s)
        ext.same(one["stat_i"][s], p["stat_i"][0], "stat_i of step %d" % s)
        assert (p["failed"] == -1).all()
    assert (one["failed"] == -1).all()
    for rid in ext.MPC_REGIONS:
        gc.same_bits(dev.region(rid), twin.region(rid), "region %d" % rid)
    total = np.zeros(low.B)
    for p in parts:
        total = total + p["cost"]
    err = np.abs(one["cost"] - total).max() / np.abs(total).max()
    print("%s: closed cost against the in-order sum of the %d steps: %.2e relative" % (label, n, err))
    assert (np.abs(one["cost"] - total) <= 1e-12 * np.abs(total)).all()
    assert np.abs(one["x"][1:] - one["x"][:-1]).max() > 0.0           # the states move
    assert (one["stat_i"][:, 0].max(axis=1) >= 1).all()                # every step iterates on some trajectory
    return dev, twin


def a_failing_trajectory_fails_alone(base, got, want_failed, before):
    """base: the run without the failures; got: the run with them; want_failed [B]; before = (rows, b): the records of
    trajectory b that precede its push.  The failed trajectories have a NaN cost; every other one has, bit for bit, the
    outputs of `base`."""
    want_failed = np.asarray(want_failed)
    assert (base["failed"] == -1).all() and np.isfinite(base["cost"]).all()
    np.testing.assert_array_equal(got["failed"], want_failed)
    assert np.isnan(got["cost"][np.flatnonzero(want_failed != -1)]).all()
    ok = np.flatnonzero(want_failed == -1)
    for k in ("x", "u"):
        ext.same(got[k][:, ok], base[k][:, ok], "%s of the other trajectories" % k)
    for k in ("stat_f", "stat_i"):
        ext.same(got[k][:, :, ok], base[k][:, :, ok], "%s of the other trajectories" % k)
    ext.same(got["cost"][ok], base["cost"][ok], "closed cost of the other trajectories")
    rows, b = before   # (and up to its failure a trajectory is what it was)
    ext.same(got["x"][:rows, b], base["x"][:rows, b], "trajectory %d before its push" % b)


def hold_one_matches_the_oracle_loop(oracle, row, host):
    """mp.loop_reference of the row against Engine.mpc_run_plant at hold = 1: iteration counts and status words exactly,
    states, controls and the final plan within 1e-6 of the trajectory's scale, step costs and the closed cost within 1e-4 of
    max(1, |cost|).  host: tests/test_mpc_host"""
    ref, pk, pb = mp.loop_reference(oracle, row, host)
    sc, sp, dist = host.parity_case(*row)
    e = ext.fresh(scenarios.lower(sc))
    r = e.mpc_run_plant(sp, host.N_STEPS, host.FIRST_MAXITER, host.ITERS_PER_STEP, 1, pk, pb, np.ascontiguousarray(dist.transpose(1, 0, 2)))
    xc, uc = gc.to_np(r.xs_closed).transpose(1, 0, 2), gc.to_np(e.pad_u(r.us_closed)).transpose(1, 0, 2)
    for s in range(host.N_STEPS):
        np.testing.assert_array_equal(gc.to_np(r.iters)[:, s], ref["iters"][s], err_msg="iterations of step %d" % s)
        _parity.assert_status_words_match(gc.to_np(r.status)[:, s], ref["status"][s])
    scale = np.maximum(1.0, np.maximum(np.abs(ref["x_closed"]).max(axis=(0, 2)), np.abs(ref["u_closed"]).max(axis=(0, 2))))
    dx = (np.abs(xc - ref["x_closed"]).max(axis=(0, 2)) / scale).max()
    du = (np.abs(uc - ref["u_closed"]).max(axis=(0, 2)) / scale).max()
    dc = (np.abs(gc.to_np(r.cost).T - ref["cost"]) / np.maximum(1.0, np.abs(ref["cost"]))).max()
    dp = (np.abs(gc.to_np(e.region(_abi.R_XS)) - ref["xs"]).max(axis=(0, 2)) / scale).max()
    dj = (np.abs(gc.to_np(r.closed_cost) - ref["closed_cost"]) / np.maximum(1.0, np.abs(ref["closed_cost"]))).max()
    print("%s %s: max rel |dx| %.2e |du| %.2e |dcost| %.2e, final plan %.2e, closed cost %.2e" % (row[0], row[1], dx, du, dc, dp, dj))
    assert dx < 1e-6 and du < 1e-6 and dp < 1e-6, (dx, du, dp)
    assert dc < 1e-4 and dj < 1e-4, (dc, dj)
    assert (gc.to_np(r.failed_knot) == -1).all()


def defaults_are_aslr_mpc_run(raw, low, sp, n, first, per):
    """hold = 1 and nothing asked of the plant: records, statistics and the regions of aslr_mpc_run, bit for bit"""
    dist = np.random.default_rng(7).uniform(-1e-3, 1e-3, (n, low.B, low.nx))
    a, b = ext.fresh(low), ext.fresh(low)
    got = raw(a, sp, n, first, per, 1, None, None, dist, False, cost=False, failed=False)
    r = b.mpc_run(sp, n, first, per, np.ascontiguousarray(dist.transpose(1, 0, 2)))
    gc.sync()
    ext.same(got["x"], gc.to_np(r.xs_closed).transpose(1, 0, 2), "x_closed")
    ext.same(got["u"], gc.to_np(b.pad_u(r.us_closed)).transpose(1, 0, 2), "u_closed")
    for i, k in enumerate(("cost", "stop", "x_reg", "step")):
        ext.same(got["stat_f"][:, i], gc.to_np(getattr(r, k)).T, k)
    ext.same(got["stat_i"][:, 0], gc.to_np(r.iters).T, "iters")
    ext.same(got["stat_i"][:, 1], gc.to_np(r.status).T, "status")
    for rid in ext.MPC_REGIONS:
        gc.same_bits(a.region(rid), b.region(rid), "region %d" % rid)
    assert int(r.iters[:, 0].min()) >= 1


def the_nominal_plant_is_neutral_and_a_plant_off_is_not(raw, low, sp, first, per, label):
    """ONE step with the trajectories' own K and B passed as plant arrays and the cost requested: x_closed[1] within 1e-11 of
    the trajectory's scale of aslr_mpc_run's; with the plant 20 % off it moves by more than 1e-6"""
    dist = np.random.default_rng(7).uniform(-1e-3, 1e-3, (1, low.B, low.nx))
    nom = lambda f: np.array([pol.nominal_diag(low, b, f) for b in range(low.B)])
    kn, bn = (nom("K") if low.dam == _abi.DAM_SEA else None), nom("B")
    base = ext.fresh(low).mpc_run(sp, 1, first, per, np.ascontiguousarray(dist.transpose(1, 0, 2)))
    want = gc.to_np(base.xs_closed).transpose(1, 0, 2)
    got = raw(ext.fresh(low), sp, 1, first, per, 1, kn, bn, dist)
    scale = np.maximum(1.0, np.abs(want).max(axis=(0, 2)))
    err = (np.abs(got["x"][1] - want[1]).max(axis=1) / scale).max()
    print("%s: x_closed[1] with the nominal plant given against aslr_mpc_run: %.2e of scale" % (label, err))
    assert err < 1e-11
    ext.same(got["x"][0], want[0], "x_closed[0]")
    assert np.isfinite(got["cost"]).all() and (got["failed"] == -1).all()
    off = raw(ext.fresh(low), sp, 1, first, per, 1, None if kn is None else 1.2 * kn, 1.2 * bn, dist)
    assert np.abs(off["x"][1] - want[1]).max() > 1e-6


def two_subshards_give_the_same_bits(raw, low, sp, n, first, per, hold, pk, pb, dist):
    """-> (the handle with one sub-shard, its outputs)"""
    e1, e2 = ext.fresh(low), ext.fresh(low, 2)
    r1, r2 = (raw(e, sp, n, first, per, hold, pk, pb, dist) for e in (e1, e2))
    ext.same(r1, r2, "two sub-shards")
    for rid in ext.MPC_REGIONS:
        gc.same_bits(e1.region(rid), e2.region(rid), "region %d with two sub-shards" % rid)
    return e1, r1


def the_head_of_a_batch_is_a_batch_of_its_own(e, r, e_head, r_head, k):
    """trajectories 0..k-1 of the run r on e against the run r_head of those k alone on e_head, bit for bit"""
    B = r["x"].shape[1]
    cut = {key: (v[:k] if key in ("cost", "failed") else v[:, :k] if key in ("x", "u") else v[:, :, :k]) for key, v in r.items()}
    ext.same(cut, r_head, "trajectories 0..%d of %d in a batch of %d" % (k - 1, B, k))
    for rid in (_abi.R_XS, _abi.R_US):
        gc.same_bits(e.region(rid)[:, :k], e_head.region(rid), "region %d of the first %d trajectories" % (rid, k))
    assert (r["stat_i"][:, 0].max(axis=1) >= 1).all()
