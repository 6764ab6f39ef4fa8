"""CPU side of the angle-range suite (tests/_angle_range.py, tests/golden/angle_range_v1.npz): the fixture regenerates to
the committed file, the three input families have the properties the GPU tests rely on, and the CPU oracle -- the checker of
the GPU tests -- is itself held to the 40-digit reference at those angles: frame placements of every frame of the planar
arm, the general chain and the 7-joint arm at 1e-13 (the figure of tests/test_gpu_geometry.py), joint-space inertia,
nonlinear effects and RNEA derivatives of the two-joint chains at the 1e-12 of tests/test_oracle_geometry.py."""
import importlib.util
import os

import numpy as np
import pytest

import _angle_range as ar
import _geometry_chains as chains
import _gpu_case as gc
from aslr_to_amd import scenarios

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


def test_the_fixture_regenerates_to_the_committed_file(oracle, golden):
    pytest.importorskip("mpmath")
    made = MK.build(oracle)
    assert sorted(made) == sorted(golden.files)
    for k, v in made.items():
        want = golden[k]
        assert v.shape == want.shape and v.dtype == want.dtype, k
        np.testing.assert_array_equal(v.view(np.uint64) if v.dtype == np.float64 else v,
                                      want.view(np.uint64) if want.dtype == np.float64 else want, err_msg=k)


# ---------------------------------------------------------------------------------------------
# input properties
# ---------------------------------------------------------------------------------------------
SWEEP_CASES = [("two_dof_vsa_boxddp", dict(B=70, T=5)), ("two_dof_sea", dict(B=70, T=5)), ("talos_arm_sea", dict(B=5, T=5))]


@pytest.mark.parametrize("name,kw", SWEEP_CASES)
def test_wound_candidates_move_the_wrapped_angle_by_rounding_only(name, kw):
    low = scenarios.lower(scenarios.SCENARIOS[name](**kw))
    nj = low.nj
    base, us0 = gc.random_candidate(low, 1)
    xs, us, k = ar.wound_candidate(low, 1)
    assert np.array_equal(us, us0) and np.array_equal(xs[..., 2 * nj:], base[..., 2 * nj:])
    assert set(np.unique(k).tolist()) <= set(ar.K_TURNS)
    if low.B * nj >= 4 * len(ar.K_TURNS):
        assert set(np.unique(k).tolist()) == set(ar.K_TURNS)
    ang, ang0 = xs[..., :2 * nj], base[..., :2 * nj]
    assert np.abs(ang).max() < ar.FAST_LIMIT                       # every angle stays on the fast path
    assert np.abs(ang).max() > 15915 * 2 * np.pi - 1.0             # ... and the largest turn count is there
    ulp = np.spacing(1.0e5)
    two_pi = 2 * np.longdouble("3.14159265358979323846264338327950288")
    k2 = np.concatenate([k, k], axis=1)                            # link and motor angle of a joint share their k
    moved = np.abs((ang.astype(np.longdouble) - two_pi * k2) - ang0).astype(np.float64)
    assert moved.max() <= ulp, moved.max()                         # (2 pi k rounds once, the sum once)
    defl, defl0 = ang[..., nj:] - ang[..., :nj], ang0[..., nj:] - ang0[..., :nj]
    assert np.abs(defl - defl0).max() <= 2 * ulp                   # the spring deflection stays
    # the second term of the reduction is in play: fn = rint(2 x / pi) reaches tens of thousands
    assert np.abs(np.rint(ang * 2 / np.pi)).max() > 60000


@pytest.mark.parametrize("name,kw", SWEEP_CASES + [("double_pendulum", dict(T=20))])
def test_quadrant_candidates_stay_within_the_rotation_bound_and_reach_every_quadrant(oracle, name, kw):
    low = scenarios.lower(scenarios.SCENARIOS[name](**kw))
    nj = low.nj
    base, us0 = gc.random_candidate(low, 1)
    xs, us, share = ar.quadrant_candidate(oracle, low, 1)
    assert np.array_equal(us, us0) and np.array_equal(xs[..., 2 * nj:], base[..., 2 * nj:])   # velocities as in the base
    q = xs[..., :nj]
    assert np.abs(q).max() < np.pi and np.abs(xs[..., nj:2 * nj] - q).max() <= 0.3
    assert 0.0 <= share < 0.3
    worst = max(ar.residual_rotation(oracle, low, int(low.node_model[t]), q[t, b], ar._ref_of(low, b))
                for t in range(low.T + 1) for b in range(low.B))
    assert worst <= ar.ROT_BOUND
    if name != "double_pendulum":
        assert worst > 2.5                                          # the bound is not vacuous
    assert ar.missing_quadrants(q.reshape(-1, nj)) == []


def test_quadrant_classes_are_all_there_are():
    """on (-pi, pi) the switch value 3 comes from negative angles only and 1 from positive ones only"""
    q = np.linspace(-np.pi, np.pi, 20001)[1:-1]
    have = set(zip(np.where(np.signbit(q), -1, 1).tolist(), ar.quadrant(q).tolist()))
    assert have == set(ar.QUADRANT_CLASSES)


def test_edge_values_are_the_nearest_doubles_to_multiples_and_ties_of_half_pi():
    mp = pytest.importorskip("mpmath")
    fast, library = ar.edge_values()
    allv = set(np.concatenate([fast, library]).tolist())
    with mp.workdps(60):
        for num, den, ks, width in ((1, 2, ar.EDGE_MULTIPLES, 2), (1, 4, [2 * k + 1 for k in ar.EDGE_TIES], 1)):
            for k in ks:
                for s in (1, -1):
                    target = s * k * mp.pi * num / den
                    x = float(target)                               # mpmath rounds to nearest
                    for y in (np.nextafter(x, np.inf), np.nextafter(x, -np.inf)):
                        assert abs(mp.mpf(x) - target) <= abs(mp.mpf(float(y)) - target)
                    for v in ar._around(x, width):
                        assert v in allv, (k, s, v)
    assert 63661 * np.pi / 2 < ar.FAST_LIMIT < 63662 * np.pi / 2
    for v in (0.0, 5e-324, 1e-300, np.nextafter(1e5, 0), 1e5, np.nextafter(1e5, np.inf), 1e6, 1e9, 2.0 ** 53):
        assert v in allv and -v in allv
    assert any(v == 0 and np.signbit(v) for v in fast) and any(v == 0 and not np.signbit(v) for v in fast)
    assert (np.abs(fast) < 1e5).all() and (np.abs(library) >= 1e5).all()
    assert sorted(np.abs(library).tolist()) == sorted([1e5, 1e5, np.nextafter(1e5, np.inf), np.nextafter(1e5, np.inf), 1e6, 1e6, 1e9, 1e9, 2.0 ** 53, 2.0 ** 53])


@pytest.mark.parametrize("chain", MK.CHAINS)
def test_edge_layouts_and_fixture_points(oracle, golden, chain):
    """the three layouts of E as the fixture holds them, and the fixture's Q and W points"""
    fast, library = ar.edge_values()
    low = scenarios.lower(MK.problem(chain))
    pts = {k: golden["%s/%s/q" % (chain, k)] for k in MK.SETS}
    on_fast = {k: np.abs(v) < ar.FAST_LIMIT for k, v in pts.items()}
    for k, v in pts.items():
        assert v.shape[1] == low.nj and v.shape[0] in (70, 130) and v.shape[0] % 64 != 0      # a partial last wave
        assert max(ar.point_rotation(oracle, low, q) for q in v) <= ar.ROT_BOUND
    assert on_fast["E_fast"].all() and not on_fast["E_library"].any()
    m = on_fast["E_mixed"]
    assert (m[1:] != m[:-1]).all()                                  # the paths alternate along the lanes, on every joint
    assert set(fast.tolist()) <= set(pts["E_mixed"][:, 0].tolist()) | set(pts["E_fast"][:, 0].tolist())
    assert set(library.tolist()) <= set(pts["E_library"][:, 0].tolist())
    seen = np.concatenate([pts["E_mixed"].ravel(), pts["E_fast"].ravel(), pts["E_library"].ravel()])
    assert set(fast.tolist()) | set(library.tolist()) == set(seen.tolist())
    assert on_fast["Q"].all() and on_fast["W"].all() and np.abs(pts["Q"]).max() < np.pi
    assert ar.missing_quadrants(pts["Q"]) == []
    assert np.abs(pts["W"]).max() > 15915 * 2 * np.pi - 1.0
    assert float(golden[chain + "/Q_redrawn"]) < 0.3


# ---------------------------------------------------------------------------------------------
# the oracle against the 40-digit reference
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", MK.CHAINS)
def test_oracle_frame_placements_match_the_fixture(oracle, golden, chain):
    """every frame at every E, Q and W point, atol 1e-13; the oracle takes libm's sin and cos, so the library-path points
    are held to the same figure"""
    c = scenarios.lower(MK.problem(chain)).desc.chain
    worst = 0.0
    for key in MK.SETS:
        q = golden["%s/%s/q" % (chain, key)]
        for f, joint in enumerate(golden[chain + "/frame_joint"]):
            fR, fp = golden[chain + "/frame_R"][f], golden[chain + "/frame_p"][f]
            for i in range(len(q)):
                R, p = oracle.frame_placement(c, q[i], joint, fR, fp)
                err = max(np.abs(R - golden["%s/%s/R" % (chain, key)][f, i]).max(), np.abs(p - golden["%s/%s/p" % (chain, key)][f, i]).max())
                worst = max(worst, err)
                assert np.isfinite(R).all() and err <= 1e-13, (key, f, i, q[i], err)
    print("%s: oracle placements within %.2e of the fixture" % (chain, worst))


@pytest.mark.parametrize("chain", ["asr_twodof", "general"])
def test_oracle_rigid_body_terms_match_the_reference_at_wound_and_quadrant_angles(oracle, golden, chain):
    """crba, nle and rnea_derivatives at 3 W and 3 Q points of the fixture, 1e-12 as in tests/test_oracle_geometry.py.
    The reference gets the very float64 angle the oracle gets (a wound angle is not its unwound one plus 2 pi k)."""
    pytest.importorskip("mpmath")
    import _hp_geometry as hp
    model = MK.problem(chain)["terminal"].state.pinocchio
    c = model.to_struct()
    rng = np.random.default_rng(5)
    wound = golden[chain + "/W/q"]
    far = np.argsort(-np.abs(wound).min(axis=1))[:3]                # the points whose every joint is wound furthest
    for q in list(wound[far]) + list(golden[chain + "/Q/q"][:3]):
        v, a = rng.uniform(-3, 3, 2), rng.uniform(-5, 5, 2)
        ref = hp.rigid_body_terms(model, q, v, a)
        dq, dv = oracle.rnea_derivatives(c, q, v, a)
        for what, got, want in (("M", oracle.crba(c, q), ref["M"]), ("nle", oracle.nle(c, q, v), ref["nle"]),
                                ("dtau/dq", dq, ref["dtau_dq"]), ("dtau/dv", dv, ref["dtau_dv"])):
            err, scale = np.abs(got - want).max(), max(1.0, np.abs(want).max())
            assert err <= 1e-12 * scale, "%s at q = %s: max |diff| %.3e > 1e-12 x %.3e" % (what, q, err, scale)


@pytest.mark.parametrize("name,kw,alphas", [("two_dof_sea", dict(B=70, T=20), range(10)), ("two_dof_vsa_boxddp", dict(B=70, T=20), range(10)),
                                            ("talos_arm_sea", dict(B=5, T=20), (0,))])
def test_oracle_forward_pass_from_wound_states_is_within_its_stated_error_of_the_40_digit_rollout(oracle, name, kw, alphas):
    """ar.FORWARD_ORACLE_ERROR -- how well a float64 roll-out from angles of 1e5 is defined at all -- measured again: the
    oracle's roll-out against ar.hp_rollout at the most sensitive trajectory of every step length (the 7-joint arm, 8 s
    per roll-out at 40 digits: the longest step only).  No roll-out of the case fails or runs away, and the figure is not
    generous: the two-joint cases reach at least a quarter of it."""
    pytest.importorskip("mpmath")
    case = ar.wound_forward_case(oracle, scenarios.SCENARIOS[name](**kw))
    sc, low, sp, xs, us, K, k = case
    for a in range(10):
        xs_try, _, _, fail = oracle.forward_pass(low, sp, 0.5 ** a, xs, us, K, k)
        assert not fail.any() and np.abs(xs_try - xs).max() < 1e3
    assert np.abs(xs[..., :low.nj]).max() > 15915 * 2 * np.pi - 1.0
    err = ar.oracle_rollout_error(oracle, case, alphas)
    print("%s: oracle against the 40-digit roll-out %.3e (stated %.2e)" % (name, err, ar.FORWARD_ORACLE_ERROR[name]))
    assert err <= ar.FORWARD_ORACLE_ERROR[name]
    if low.nj == 2:
        assert err >= 0.25 * ar.FORWARD_ORACLE_ERROR[name]
