"""The oracle's geometry against the 40-digit reference of tests/_hp_geometry.py (which shares none of its formulas):
joint-space inertia, nonlinear effects, RNEA derivatives, frame placements and LOCAL frame Jacobians of two-joint chains
with general 3-D geometry, and the SE(3) log and its Jacobian in every branch of Pinocchio's formulas.  CPU only."""
import numpy as np
import pytest

import _geometry_chains as gc
import _hp_geometry as hp

TAYLOR = 2.0 ** -13          # Pinocchio's TaylorSeriesExpansion<double>::precision<3>() = eps^(1/4): log3 / log6 switch


def _close(got, ref, rel, what):
    err = np.abs(np.asarray(got) - np.asarray(ref)).max()
    scale = max(1.0, np.abs(ref).max())
    assert err <= rel * scale, "%s: max |diff| %.3e > %.1e x %.3e" % (what, err, rel, scale)


@pytest.mark.parametrize("name", gc.CHAINS)
def test_rigid_body_terms_match_the_lagrangian_reference(oracle, name):
    """crba, nle, rnea_derivatives, frame_placement and frame_jacobian (LOCAL) at 7 random states per chain (21 in all),
    every frame of the chain (the welded end effector with its rotated origin included), to 1e-12 relative: the oracle's
    recursions round ~10 times per entry (measured: ~6e-16)."""
    model = gc.chain(name)
    c = model.to_struct()
    frames = [(f.parent, f.placement.rotation, f.placement.translation) for f in model.frames if f.parent >= 0]
    rng = np.random.default_rng(11 + gc.CHAINS.index(name))
    for _ in range(7):
        q, v, a = rng.uniform(-np.pi, np.pi, 2), rng.uniform(-3, 3, 2), rng.uniform(-5, 5, 2)
        ref = hp.rigid_body_terms(model, q, v, a, frames)
        _close(oracle.crba(c, q), ref["M"], 1e-12, "M")
        _close(oracle.nle(c, q, v), ref["nle"], 1e-12, "nle")
        dq, dv = oracle.rnea_derivatives(c, q, v, a)
        _close(dq, ref["dtau_dq"], 1e-12, "dtau/dq")
        _close(dv, ref["dtau_dv"], 1e-12, "dtau/dv")
        for (joint, fR, fp), (R, p, J) in zip(frames, ref["frames"]):
            Ro, po = oracle.frame_placement(c, q, joint, fR, fp)
            _close(Ro, R, 1e-12, "oMf.R")
            _close(po, p, 1e-12, "oMf.p")
            _close(oracle.frame_jacobian(c, q, joint, fR, fp), J, 1e-12, "LOCAL frame Jacobian")


def test_the_general_chain_is_really_three_dimensional():
    """The general chain loads the joints about x and z as well as y (gravity has three non-zero components, the axes
    are not parallel, the inertia tensors are full): without this the test above would not reach the 3-D terms."""
    model = gc.chain("general")
    assert np.all(model.gravity.linear != 0.0)
    a0, a1 = model.joints[0].axis, model.joints[1].axis
    assert abs(np.dot(a0, model.joints[1].placement.rotation.dot(a1))) < 0.9
    for j in model.joints:
        assert np.all(j.inertia[~np.eye(3, dtype=bool)] != 0.0)
    ee = model.frames[model.getFrameId("EE")]
    assert np.abs(ee.placement.rotation - np.eye(3)).max() > 0.1


# (angle, |log6 diff| allowed, |Jlog6 diff| allowed, what limits Pinocchio's formula there); diffs are absolute on
# entries of size ~1 (translations up to sqrt(3))
BANDS = [
    ("zero", lambda: 0.0, 1e-15, 1e-15,
     "trace exactly 3: theta = 0, the Taylor series at 0 is exact"),
    ("1e-9", lambda: 1e-9, 1e-15, 1e-15,
     "the trace rounds to 3 (theta = 0); w comes from the antisymmetric part, exact to eps"),
    ("below 2^-13", lambda: TAYLOR * (1 - 1e-3), 1e-12, 1e-12,
     "log3's Taylor branch takes theta / sin(theta) as 1: w is off by theta^3 / 6 = 3e-13"),
    ("above 2^-13", lambda: TAYLOR * (1 + 1e-3), 1e-14, 1e-11,
     "1 / theta^2 - sin / (2 theta (1 - cos)) cancels ~8 digits in Jlog6's beta and its derivative (measured 1e-12)"),
    ("1e-3", lambda: 1e-3, 1e-14, 5e-12,
     "the same cancellation, ~6 digits (measured 4e-13)"),
    ("0.7", lambda: 0.7, 1e-14, 1e-14, "generic angle: a few roundings"),
    ("2.5", lambda: 2.5, 1e-14, 1e-14, "generic angle: a few roundings"),
    ("pi - 2e-2", lambda: np.pi - 2e-2, 2e-12, 2e-12,
     "acos of the trace near -1: theta is off by eps / sin(theta) ~ 1e-14, scaled up by theta / sin(theta) ~ 1.6e2"),
    ("switch - 1e-9", lambda: np.pi - 1e-2 - 1e-9, 1e-11, 5e-12,
     "the same at sin(theta) = 1e-2, the last angle of the general branch (measured 3e-12)"),
    ("switch + 1e-9", lambda: np.pi - 1e-2 + 1e-9, 1e-12, 1e-12,
     "first angle of the near-pi branch: square roots of diagonal terms of size ~|axis_i|^2 (measured 1e-14)"),
    ("pi - 1e-4", lambda: np.pi - 1e-4, 1e-11, 1e-8,
     "sin(theta) = 1e-4 is taken from theta = acos(...), which is off by eps / sin(theta) = 1e-12: 1e-8 relative in "
     "Jlog3's theta sin / (1 - cos) term (measured 1.4e-9)"),
]


@pytest.mark.parametrize("band", BANDS, ids=[b[0] for b in BANDS])
def test_log6_and_jlog6_in_every_band_match_the_matrix_logarithm(oracle, band):
    """log6 against mpmath's logm of the 4x4 matrix, Jlog6 against central differences of that log under right
    perturbations, on placements exp([w^ v; 0 0]) with random axes and translations; the tolerance of each band is what
    Pinocchio's formula delivers there (the reason is stated with it)."""
    name, angle, tol_log, tol_jlog, why = band
    rng = np.random.default_rng(100 + [b[0] for b in BANDS].index(name))
    for k in range(2):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        R, p = hp.se3_from_twist(rng.uniform(-1, 1, 3), angle() * axis)
        ref = hp.log6(R, p)
        err = np.abs(oracle.log6(R, p) - ref).max()
        assert err <= tol_log, "log6 at %s: %.3e > %.1e (%s)" % (name, err, tol_log, why)
        if k == 0:
            err = np.abs(oracle.jlog6(R, p) - hp.jlog6(R, p)).max()
            assert err <= tol_jlog, "Jlog6 at %s: %.3e > %.1e (%s)" % (name, err, tol_jlog, why)


def test_log6_at_exactly_pi_is_right_up_to_the_sign_of_w(oracle):
    """A half turn has two logs, w and -w: only |w| = pi, the axis of w, the translation part that goes with the w the
    oracle chose, and the cost 1/2 |r|^2 (the same for both: V(-w) = V(w)^T, a scaled rotation about the axis) are
    compared.  R = 2 a a^T - I rounded to float64 has a trace within 4 eps of -1: theta is pi to within sqrt(8 eps) ~ 4e-8,
    and the near-pi branch's square roots cost ~sqrt(eps) relative on the components of w.
    Pinocchio's near-pi branch takes the sign of each component of w on its own, from R[7] > R[5], R[2] > R[6],
    R[3] > R[1]; a symmetric R (exactly pi) ties all three, and every component comes out negative.  That is a log of R
    only when the axis has no components of opposite signs, so the magnitudes |w_i| = pi |a_i| are checked for every
    axis, and the direction, translation and cost for the axes where the answer is a log."""
    rng = np.random.default_rng(5)
    axes = (np.array([1.0, 0.0, 0.0]), np.array([0.0, 0.6, 0.8]), np.abs(rng.normal(size=3)),
            -np.abs(rng.normal(size=3)), np.array([0.48, -0.6, 0.64]))
    for axis in axes:
        axis = axis / np.linalg.norm(axis)
        R = 2.0 * np.outer(axis, axis) - np.eye(3)
        p = rng.uniform(-1, 1, 3)
        r = oracle.log6(R, p)
        w = r[3:]
        assert np.abs(np.abs(w) - np.pi * np.abs(axis)).max() < 1e-7
        if (axis >= 0).all() or (axis <= 0).all():
            assert abs(np.linalg.norm(w) - np.pi) < 1e-7
            assert np.linalg.norm(np.cross(w / np.linalg.norm(w), axis)) < 1e-7
            v_ref = hp.translation_log_for(R, p, w)
            assert np.abs(r[:3] - v_ref).max() < 1e-7
            v_other = hp.translation_log_for(R, p, -w)
            cost, cost_ref = 0.5 * r.dot(r), 0.5 * (v_other.dot(v_other) + np.pi ** 2)
            assert abs(cost - cost_ref) < 1e-7 * cost_ref
        else:   # opposite signs: the tie gives a sign pattern that is not a log of R (w is not along the axis)
            assert np.linalg.norm(np.cross(w / np.linalg.norm(w), axis)) > 0.1
