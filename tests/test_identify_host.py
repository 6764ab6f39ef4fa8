"""aslr_plant_identify (include/aslr_to_amd_identify.h) on a CPU: the contract of the extension header, the two closed forms of
the kernel against the definition of tests/_identify.py, and the reference loop on the oracle alone -- the conditions on the
cases the GPU tests reuse (tests/test_gpu_identify.py), a joint held still, recovery of the true plant, noisy data."""
import ctypes as C

import numpy as np
import pytest

import _identify as I
from aslr_to_amd import _abi


def test_a_null_handle_is_refused_by_name():
    lib = _abi.load_library()
    assert lib.aslr_workspace_bytes(None) < 0     # some other message is in the buffer first
    d = _abi.Identify()
    assert lib.aslr_plant_identify(None, C.byref(d), None) == _abi.E_INVALID
    msg = lib.aslr_last_error().decode()
    assert msg.startswith("aslr_plant_identify:") and "handle" in msg, msg


def closed_forms(oracle, c, theta, b, t):
    """r_t and Jz_t as the kernel forms them: from the oracle's Fx record and four words of Y / xnext"""
    low, Y, U, fields = c["low"], c["Y"], c["U"], c["fields"]
    nj, nx = low.nj, low.nx
    import _policy as pol
    mi = int(low.node_model[t])
    k, bm = I.full_diag(c, theta, b)
    lb = pol.plant_problem(low, b, k, bm)
    kn = oracle.knot(lb, mi, Y[t, b], U[t, b], diff=True)
    Fx = np.asarray(kn["Fx"]).reshape(nx, nx)
    xn, x = kn["xnext"], Y[t, b]
    dt = lb.desc.models[mi].dt
    cols = []
    eye = np.eye(nx)
    if "K" in fields:
        for j in range(nj):
            cols.append(-(x[j] - x[nj + j]) * (Fx[:, nj + j] - eye[nj + j]))
    if "B" in fields:
        for j in range(nj):
            cols.append(-(xn[3 * nj + j] - x[3 * nj + j]) * (dt * eye[nj + j] + eye[3 * nj + j]))
    return Y[t + 1, b] - xn, np.stack(cols, axis=1)


@pytest.mark.parametrize("name", sorted(I.CASES))
def test_the_closed_forms_are_the_definition(oracle, name):
    """Jz_t of the closed forms against the central differences of the definition at theta_0, every knot of every trajectory:
    1e-11 per trajectory and knot as max |a - b| / max |b|, the bound tests/test_plant_sens_host.py holds the same identities to"""
    c = I.case(oracle, name)
    worst = 0.0
    for b in range(c["low"].B):
        for t in range(c["low"].T):
            r0, J0 = I.jacobian(oracle, c, c["theta0"], b, t)
            r1, J1 = closed_forms(oracle, c, c["theta0"], b, t)
            np.testing.assert_array_equal(r0, r1)
            worst = max(worst, float(np.abs(J1 - J0).max() / np.abs(J0).max()))
    print("%s: closed forms against the definition %.2e" % (name, worst))
    assert worst < 1e-11, worst


@pytest.mark.parametrize("name", sorted(I.CASES))
def test_the_cases_are_conditioned_and_the_loop_accepts_rejects_and_recovers(oracle, name):
    c = I.case(oracle, name)
    r = I.reference_run(oracle, name)
    st, dec = r["state"], r["decision"]
    npar, B = c["theta0"].shape
    H = I.unpack(st["info"], npar)
    cond = max(np.linalg.cond(H[:, :, b]) for b in range(B))
    n = I.compared_steps(r)
    print("%s: cond(H) %.2e, %d of %d steps compared, decisions %s" % (name, cond, n, c["n_steps"], dec.T.tolist()))
    assert cond < 1e8, cond
    assert st["identifiable"].all()
    assert (dec[0] == 1).all() and (dec[1:n] == 1).any() and (dec[:n] == 0).any()
    assert 3 * n >= 2 * c["n_steps"], "more than the last third of the steps is not compared"
    m = r["margin"][1:n]
    assert (m[~np.isnan(m)] > I.MARGIN).all()
    # sse never rises over accepted steps; the bounds hold
    assert (np.diff(r["sse_acc"], axis=0) <= 0.0).all()
    assert (r["theta_hist"] >= c["lo"]).all() and (r["theta_hist"] <= c["hi"]).all()


@pytest.mark.parametrize("name", sorted(I.CASES))
def test_the_reference_recovers_the_true_plant_as_recorded(oracle, name):
    """N_RECOVER steps of the reference loop on noise-free data, with and without the dither: every parameter identifiable,
    cond(H) below 1e8, and the recovery error no larger than tests/_identify.RECOVERY records (which the GPU bound rests on)"""
    c = I.case(oracle, name)
    npar, B = c["theta0"].shape
    for (rec, st), recorded, what in zip(I.reference_recovery(oracle, name), I.RECOVERY[name], ("dithered", "plain")):
        cond = max(np.linalg.cond(I.unpack(st["info"], npar)[:, :, b]) for b in range(B))
        print("%s, %s data: recovery %.2e (recorded %.2e), cond(H) %.2e" % (name, what, rec, recorded, cond))
        assert st["identifiable"].all() and cond < 1e8
        assert rec <= recorded, rec


def test_a_joint_held_still_is_not_identifiable(oracle):
    """delta_1 = 0 at every knot (the motor angle of joint 1 is set to the link angle in the recorded states): the stiffness
    of joint 1 is reported as not identifiable and stays at theta_0; the other parameters move"""
    c = dict(I.case(oracle, "sea"))
    nj = c["low"].nj
    Y = c["Y"].copy()
    Y[:, :, nj + 1] = Y[:, :, 1]
    c["Y"] = Y
    r = I.run(lambda th: I.definition(oracle, c, th), c["theta0"], c["lo"], c["hi"], 4, **I.params(c))
    st = r["state"]
    assert (st["identifiable"][1] == 0).all() and (st["identifiable"][[0, 2, 3]] == 1).all()
    np.testing.assert_array_equal(r["theta_hist"][:, 1], np.broadcast_to(c["theta0"][1], r["theta_hist"][:, 1].shape))
    assert (st["theta"][[0, 2, 3]] != c["theta0"][[0, 2, 3]]).all()


def test_noisy_data_descends_inside_the_bounds(oracle):
    c = dict(I.case(oracle, "sea"))
    c["Y"] = c["Y"] + np.random.default_rng(7).normal(0.0, 1e-2, c["Y"].shape)
    r = I.run(lambda th: I.definition(oracle, c, th), c["theta0"], c["lo"], c["hi"], 8, **I.params(c))
    assert (np.diff(r["sse_acc"], axis=0) <= 0.0).all() and (r["sse_acc"][-1] < r["sse_acc"][0]).all()
    assert (r["theta_hist"] >= c["lo"]).all() and (r["theta_hist"] <= c["hi"]).all()
    assert (r["state"]["sse"] > 0.0).all()
