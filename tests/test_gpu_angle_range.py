"""Model kernels over the full angle range.  Every kernel takes the sines and cosines of its joint angles from sincos_fast
(csrc/aslr_device.hpp), which exists in two copies: the literal one (axis_angle, Chain3D::setup_world) and the SinCosK one
of ChainPlanar.  The other GPU suites draw every angle from U(-0.8, 0.8); here the inputs are the three families of
tests/_angle_range.py -- W (wound by up to 15915 turns), Q (all four quadrants, the frame-placement residual rotation kept
below pi - 0.1) and E (edges of the reduction and of the 1e5 switch to the library's sincos):

 a. frame placements against the 40-digit fixture tests/golden/angle_range_v1.npz (no oracle in the loop);
 b. the point evaluators dam_eval / dam_residuals against the oracle, which tests/test_angle_range_host.py holds to the
    40-digit reference at these angles; the residual vector keeps the frame cost visible where the state regulariser on a
    wound angle (~1e9) drowns it in the scalar cost;
 c. the calc / calcDiff sweeps;
 d. the forward pass of every step length: the kernels that loop over knots, where ChainPlanar takes the copy of the
    routine whose constants sit in registers, and the team kernels of the 7-joint arm;
 e. the policy roll-outs, whose plant steps have their own code.
Tolerances are those of the suites these tests extend, written at each assert."""
import importlib.util
import os

import numpy as np
import pytest

import _angle_range as ar
import _ext_call as ext
import _geometry_chains as chains
import _gpu_case as gc
import _policy as pol
import _policy_team as pt
from aslr_to_amd import _abi, scenarios

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _maker():
    spec = importlib.util.spec_from_file_location("make_angle_range", os.path.join(GOLDEN, "make_angle_range.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


MK = _maker()


@pytest.fixture(scope="module")
def golden():
    return np.load(MK.FILE)


# ---------------------------------------------------------------------------------------------
# a. frame placements against the fixture
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain,no_planar", [("asr_twodof", False), ("asr_twodof", True), ("general", False), ("talos_arm", False)])
def test_frame_placements_match_the_40_digit_fixture(golden, monkeypatch, chain, no_planar):
    """Engine.frame_placement for every frame at E in its three layouts, at Q and at W: atol 1e-13, the figure of
    tests/test_gpu_geometry.py; every output finite.  asr_twodof as created runs ChainPlanar (the SinCosK copy), under
    ASLR_NO_PLANAR=1 and on the other chains Chain3D (the literal copy).
    The world rotation of asr_twodof's "joint1" frame (identity on a joint whose placement rotation is the identity and
    whose axis is +z) is a single sine and cosine of q[0]: those entries are held to 2^-52 absolute -- 1.73 ulp of a
    value below 1 (at most 1.92e-16, the routine's measured worst case on a host replica) plus margin for the device's
    different contraction; the library path is held to the same figure."""
    import torch
    monkeypatch.setenv("ASLR_NO_PLANAR", "1" if no_planar else "0")     # (read when the handle is created)
    low = scenarios.lower(MK.problem(chain))
    e = gc.engine(low)
    single = []
    if chain == "asr_twodof":
        c = low.desc.chain
        assert np.array_equal(np.array(c.joint_R[0][:]), np.eye(3).ravel()) and tuple(c.axis[0][:]) == (0.0, 0.0, 1.0)
        single = [f for f in range(len(golden[chain + "/frame_joint"])) if golden[chain + "/frame_joint"][f] == 0
                  and np.array_equal(golden[chain + "/frame_R"][f], np.eye(3))]
        assert single
    worst, worst_single = 0.0, 0.0
    for key in MK.SETS:
        q = golden["%s/%s/q" % (chain, key)]
        xd = torch.as_tensor(q, device=e.device)
        for f, joint in enumerate(golden[chain + "/frame_joint"]):
            R, p = e.frame_placement(int(joint), golden[chain + "/frame_R"][f], golden[chain + "/frame_p"][f], xd)
            R, p = gc.to_np(R), gc.to_np(p)
            Rr, pr = golden["%s/%s/R" % (chain, key)][f], golden["%s/%s/p" % (chain, key)][f]
            assert np.isfinite(R).all() and np.isfinite(p).all(), (key, f)
            err = np.maximum(np.abs(R - Rr).max(axis=(1, 2)), np.abs(p - pr).max(axis=1))
            worst = max(worst, err.max())
            assert err.max() <= 1e-13, "%s frame %d: %.3e at point %d, q = %s" % (key, f, err.max(), err.argmax(), q[err.argmax()])
            if f in single:
                e1 = np.abs(R - Rr)[:, :2, :2].max(axis=(1, 2))
                worst_single = max(worst_single, e1.max())
                assert e1.max() <= 2.0 ** -52, "%s: sin / cos of q[0] off by %.3e at q[0] = %r" % (key, e1.max(), q[e1.argmax(), 0])
    print("%s%s: placements within %.2e of the fixture (1e-13); single sin / cos within %.2e (2.22e-16)"
          % (chain, " (general path)" if no_planar else "", worst, worst_single))


# ---------------------------------------------------------------------------------------------
# b. point evaluators against the oracle
# ---------------------------------------------------------------------------------------------
def _point_problem(name):
    if name.startswith("general_"):
        return chains.problem("general", name.split("_")[1], B=1, T=1, seed=2)
    return scenarios.SCENARIOS[name](T=1) if name == "double_pendulum" else scenarios.SCENARIOS[name](B=1, T=1, seed=2)


POINT_MODELS = ["two_dof_sea", "two_dof_vsa_boxddp", "double_pendulum", "talos_arm_sea", "general_sea", "general_vsa"]
STATE_KEYS, DERIV_KEYS = ("xout", "cost"), ("Fx", "Fu", "Lx", "Lu", "Lxx", "Lxu", "Luu")


@pytest.mark.parametrize("name", POINT_MODELS)
def test_point_evaluators_match_the_oracle_at_wound_quadrant_and_edge_angles(oracle, name):
    """dam_eval and dam_residuals of the running and the terminal model at W, Q and the three layouts of E, with the
    per-entry tolerances of test_model_level_entry_points_on_the_general_chain: 1e-11 on xout, cost and residuals, 1e-9 on
    the derivative blocks (max |a - b| / (1 + |b|))."""
    low = scenarios.lower(_point_problem(name))
    fref = ar._ref_of(low, 0)
    rot = lambda q: ar.point_rotation(oracle, low, q)
    sets = {"W": ar.wound_states(low, 9, 70)[:2]}
    sets["Q"] = ar.states_at(low, ar.quadrant_points(oracle, low, 9, 70)[0], 10)
    for k in ar.EDGE_LAYOUTS:
        sets["E_" + k] = ar.states_at(low, ar.edge_points(k, low.nj, rot), 11)
    e = gc.engine(low)
    worst = {}
    for key, (x, u) in sets.items():
        assert max(rot(xi[:low.nj]) for xi in x) <= ar.ROT_BOUND
        for mi in range(low.desc.nmodels):
            got = e.dam_eval(mi, x, u)
            res = e.dam_residuals(mi, x, u)
            ref = [oracle.dam(low, mi, x[b], u[b], frame_ref=fref) for b in range(len(x))]
            rres = np.array([oracle.dam_residuals(low, mi, x[b], u[b], frame_ref=fref) for b in range(len(x))])
            for k in STATE_KEYS + DERIV_KEYS + ("residuals",):
                g = res if k == "residuals" else got[k]
                w = rres if k == "residuals" else np.array([r[k] for r in ref]).reshape(g.shape)
                assert np.isfinite(g).all(), (key, mi, k)
                err = np.abs(g - w) / (1.0 + np.abs(w))
                b = int(np.argmax(err.reshape(len(x), -1).max(axis=1)))
                tol = 1e-9 if k in DERIV_KEYS else 1e-11
                worst[k] = max(worst.get(k, 0.0), err.max())
                assert err.max() < tol, "%s model %d %s: %.3e at point %d, q = %s" % (key, mi, k, err.max(), b, x[b, :low.nj])
    print(name, " ".join("%s %.1e" % kv for kv in worst.items()))


# ---------------------------------------------------------------------------------------------
# c. sweeps, d. forward passes
# ---------------------------------------------------------------------------------------------
CASES = ["two_dof_vsa_boxddp", "two_dof_sea", "double_pendulum", "talos_arm_sea"]      # the four of tests/test_gpu_parity.py
BATCH = {"two_dof_vsa_boxddp": 70, "two_dof_sea": 70, "talos_arm_sea": 5}


def _problem(name, T):
    if name.startswith("general_"):
        return chains.problem("general", name.split("_")[1], B=70, T=T, seed=3)
    return scenarios.SCENARIOS[name](T=T) if name == "double_pendulum" else scenarios.SCENARIOS[name](B=BATCH[name], T=T)


def _candidate(oracle, low, family, seed):
    return ar.wound_candidate(low, seed)[:2] if family == "W" else ar.quadrant_candidate(oracle, low, seed)[:2]


@pytest.mark.parametrize("family", ["W", "Q"])
@pytest.mark.parametrize("name", CASES + ["general_sea", "general_vsa"])
def test_sweeps_match_the_oracle(oracle, name, family):
    """calcDiff, calc alone and calcDiff at a second point (gc.check_calc_and_calc_diff's sequence) from a W and a Q
    candidate, T = 5, through gc.assert_records_match at its defaults: 1e-11 on xnext and cost, 1e-9 on the DERIV record."""
    low = scenarios.lower(_problem(name, 5))
    e = gc.engine(low)
    xs, us = _candidate(oracle, low, family, 1)
    ref = oracle.calc_diff(low, xs, us)
    gc.assert_records_match(*gc.run_calc_diff(e, xs, us), ref=ref)
    gc.assert_records_match(*gc.run_calc(e), None, ref=ref)
    xs2, us2 = _candidate(oracle, low, family, 5)
    ref2 = oracle.calc_diff(low, xs2, us2)
    assert np.abs(ref2[2] - ref[2]).max() > 1e-3        # the point really changed
    gc.assert_records_match(*gc.run_calc_diff(e, xs2, us2), ref=ref2)


@pytest.mark.parametrize("family", ["W", "Q"])
@pytest.mark.parametrize("name", CASES)
def test_forward_pass_matches_the_oracle_for_every_alpha(oracle, name, family):
    """rollout_kernel / rollout_and_cost_kernel / trial_cost_kernel (the team kernels at nj = 7) of every step length, T = 20,
    through gc.assert_forward_matches, and more than half of the roll-outs of every step length finite.
    at 1e-9 for both families.
    Q: gains by gc.forward_inputs on the Q candidate.
    W: ar.wound_forward_case -- gains of the unwound candidate, so that no roll-out runs away; candidate and x0 wound.  A
    roll-out from angles of 1e5 is defined to a few 1e-9 only in float64 (tests/test_angle_range_host.py: the oracle is
    1.6e-9 from the same roll-out at 40 digits), but kernel and oracle round the wound angles alike, and 1e-9 holds
    (measured: 7e-12)."""
    sc = _problem(name, 20)
    if family == "W":
        sc, low, sp, xs, us, K, k = ar.wound_forward_case(oracle, sc)
    else:
        low, sp = scenarios.lower(sc), scenarios.solver_params(sc)
        xs, us, K, k, _ = gc.forward_inputs(oracle, low, sp, 5, False, candidate=_candidate(oracle, low, family, 5))
    e = gc.run_forward(low, sp, xs, us, K, k, None, 1)
    oks, _ = gc.assert_forward_matches(*gc.forward_outputs(e), lambda alpha: oracle.forward_pass(low, sp, alpha, xs, us, K, k), tol=1e-9)
    assert all(ok.mean() > 0.5 for ok in oks)


# ---------------------------------------------------------------------------------------------
# e. the plant steps of the policy roll-outs
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,export", [("sea_plain", "aslr_policy_rollout"), ("arm_sea_plain", "aslr_policy_rollout_all")])
def test_policy_rollouts_match_the_definition_from_wound_states(oracle, key, export):
    """tests/test_gpu_policy.py's sea_plain and tests/test_gpu_policy_team.py's arm_sea_plain with x0 wound as in W; the
    nominal states are the oracle's open-loop roll-out from the wound x0, so they are wound with it.  The references of
    tests/_policy.py and their tolerance: 1e-9."""
    c = pol.case(oracle, key) if key in pol.CASES else pt.case(oracle, key)
    low0 = c["low"]
    B, T, nj = low0.B, low0.T, low0.nj
    sc = dict(c["sc"])
    sc["x0"] = ar.wind(np.asarray(sc["x0"], dtype=np.float64), ar.turns(B, nj, 31), nj)
    low = scenarios.lower(sc)
    zx, zk = np.zeros((T + 1, low.nx)), np.zeros((T, low.nu, low.nx))
    xs = np.stack([pol.rollout_one(oracle, low, b, zx, c["us"][:, b], zk)["xs"] for b in range(B)], axis=1)
    assert np.abs(xs[..., :nj]).max() > 15915 * 2 * np.pi - 1.0 and np.abs(xs[..., :2 * nj]).max() < ar.FAST_LIMIT
    c = dict(c, sc=sc, low=low, xs=xs)
    e, K = ext.with_gains(c)
    got = ext.policy_rollout(e, export, c["S"], c["pert"], c["clamp"])
    want = pol.rollout(oracle, low, xs, c["us"], K, c["S"], clamp=c["clamp"], **c["pert"])
    assert (want["failed_knot"] == -1).all()
    np.testing.assert_array_equal(got["failed_knot"], want["failed_knot"])
    assert np.abs(want["xs"] - xs.transpose(1, 0, 2)[:, None]).max() > 1e-3   # the perturbations moved the loop
    for k in pol.OUTPUTS:
        gc._assert_close("%s %s" % (key, k), got[k], want[k], 1e-9)
