"""Inputs that take the joint angles out of the first quadrant, shared by tests/test_angle_range_host.py,
tests/test_gpu_angle_range.py and tests/golden/make_angle_range.py.  Every kernel gets the sines and cosines of its joint
angles from sincos_fast (csrc/aslr_device.hpp): a two-term reduction by pi/2, a quadrant switch on rint(2 x / pi) & 3, and
the library's sincos from |x| >= 1e5 on.  gc.random_candidate draws every angle from U(-0.8, 0.8), where the quadrant is 0
on 98 % of the draws and never 2 or 3.  Everything here is chosen on the CPU from seeded draws.  Three families:

 W, wound      gc.random_candidate's state with 2 pi k added to the link AND the motor angle of a joint (so the spring
               deflection stays), k per (trajectory, joint) from K_TURNS.  15915 * 2 pi = 99996.9 < 1e5: every angle
               stays on the fast path.  The wrapped angle moves by rounding only, so the conditioning is that of the
               unwound state and the tolerances of the existing suites carry over.
 Q, quadrants  link angles U(-pi, pi) per joint, motor angle = link angle + U(-0.3, 0.3), velocities as in the base.  A
               state whose frame-placement residual rotation exceeds ROT_BOUND = pi - 0.1 is redrawn: near pi the SE(3)
               log is ill-conditioned and kernel and oracle legitimately differ (tests/test_oracle_geometry.py).
 E, edges      for the point evaluators only (they take arbitrary points): the doubles at and next to multiples of pi/2
               and ties of rint, zeros and denormals, the doubles around the 1e5 switch, and large arguments; in three
               layouts: fast-path and library-path angles alternating inside a wave, waves wholly on either path.
"""
from fractions import Fraction

import numpy as np

import _gpu_case as gc
from aslr_to_amd import _abi

K_TURNS = (0, 1, -1, 7, -7, 100, -100, 1000, -1000, 15915, -15915)
ROT_BOUND = np.pi - 0.1
FAST_LIMIT = 1.0e5          # sincos_fast: the library path from here on
# pi to 60 digits: the doubles nearest to multiples of pi/2 are rounded once from exact rationals
_PI = Fraction(int("3141592653589793238462643383279502884197169399375105820974944"), 10 ** 60)
EDGE_MULTIPLES = (1, 2, 3, 4, 63661)          # k of k pi/2, both signs (63661 pi/2 = 99998.5: the last one below 1e5)
EDGE_TIES = (0, 1, 2, 5, 1000, 63660)         # k of (k + 1/2) pi/2, the ties of rint(2 x / pi), both signs
EDGE_LAYOUTS = {"mixed": 130, "fast": 70, "library": 70}   # points per layout: a partial last wave each


def _nearest(fr):
    return float(fr)    # (Fraction.__float__ rounds correctly)


def _around(x, n):
    """x and its n neighbours on each side, ascending"""
    lo, hi = [x], [x]
    for _ in range(n):
        lo.append(np.nextafter(lo[-1], -np.inf))
        hi.append(np.nextafter(hi[-1], np.inf))
    return lo[:0:-1] + hi


def edge_values():
    """-> (fast, library): the E angles that take sincos_fast's own reduction and those that take the library path"""
    v = []
    for k in EDGE_MULTIPLES:
        for s in (1, -1):
            v += _around(_nearest(s * k * _PI / 2), 2)
    for k in EDGE_TIES:
        for s in (1, -1):
            v += _around(_nearest(s * (2 * k + 1) * _PI / 4), 1)
    for a in (0.0, 5e-324, 1e-300, np.nextafter(FAST_LIMIT, 0.0), FAST_LIMIT, np.nextafter(FAST_LIMIT, np.inf), 1e6, 1e9, 2.0 ** 53):
        v += [a, -a]
    v = np.array(v, dtype=np.float64)
    fast = np.abs(v) < FAST_LIMIT
    return v[fast], v[~fast]


def quadrant(q):
    """rint(2 q / pi) & 3 with sincos_fast's own constant: the value its switch takes"""
    return np.rint(np.asarray(q) * 6.36619772367581382433e-01).astype(np.int64) & 3


# ---------------------------------------------------------------------------------------------
# the residual rotation of the frame-placement costs
# ---------------------------------------------------------------------------------------------
def residual_rotation(oracle, low, mi, q, frame_ref=None):
    """max over the frame-placement costs of model mi of |oracle.log6(rMf)[3:]|, rMf = Mref^-1 oMf(q); 0 without such a
    cost.  frame_ref: the 12 words that override the cost's own reference (a trajectory's row of low.frame_ref)."""
    worst = 0.0
    m = low.desc.models[mi]
    for ci in range(m.ncosts):
        ct = m.costs[ci]
        if ct.type != _abi.COST_FRAME_PLACEMENT:
            continue
        ref = np.array(ct.ref[:12]) if frame_ref is None else np.asarray(frame_ref, dtype=np.float64)
        Rr, pr = ref[:9].reshape(3, 3), ref[9:]
        R, p = oracle.frame_placement(low.desc.chain, q, ct.frame_joint, np.array(ct.frame_R[:]), np.array(ct.frame_p[:]))
        worst = max(worst, float(np.linalg.norm(oracle.log6(Rr.T.dot(R), Rr.T.dot(p - pr))[3:])))
    return worst


def _ref_of(low, b):
    return None if low.frame_ref is None else low.frame_ref[b]


def point_rotation(oracle, low, q):
    """residual_rotation over every model of `low` at trajectory 0's reference: what the point evaluators see"""
    return max(residual_rotation(oracle, low, mi, q, _ref_of(low, 0)) for mi in range(low.desc.nmodels))


# ---------------------------------------------------------------------------------------------
# W and Q candidates (xs [T+1, B, nx], us [T, B, nu], the layout of gc.random_candidate)
# ---------------------------------------------------------------------------------------------
def turns(B, nj, seed):
    """k [B, nj], drawn from K_TURNS: a seeded shuffle of the set, repeated over the batch and shuffled again, so that a
    batch of a few trajectories already sees most of the values"""
    rng = np.random.default_rng(seed)
    k = np.resize(rng.permutation(K_TURNS), B * nj)
    return rng.permutation(k).reshape(B, nj)


def wind(x, k, nj):
    """x [..., B, nx] with 2 pi k [B, nj] added to link and motor angles (a copy)"""
    x = np.array(x, dtype=np.float64)
    x[..., :nj] += 2.0 * np.pi * k
    x[..., nj:2 * nj] += 2.0 * np.pi * k
    return x


def wound_candidate(low, seed):
    """-> xs, us, k: gc.random_candidate(low, seed) wound by turns(low, seed + 100)"""
    xs, us = gc.random_candidate(low, seed)
    k = turns(low.B, low.nj, seed + 100)
    return wind(xs, k, low.nj), us, k


def wound_points(nj, seed, n):
    """-> q [n, nj], k: link angles U(-0.8, 0.8) (gc.random_candidate's range) wound by turns(n, nj, seed + 100)"""
    k = turns(n, nj, seed + 100)
    return np.random.default_rng(seed).uniform(-0.8, 0.8, (n, nj)) + 2.0 * np.pi * k, k


def wound_states(low, seed, n):
    """-> x [n, nx], u [n, nu], k for the point evaluators: states and controls drawn as gc.random_candidate draws them, link
    and motor angles wound by turns(n, nj, seed + 100)"""
    x, u = states_at(low, np.random.default_rng(seed).uniform(-0.8, 0.8, (n, low.nj)), seed + 1)
    x[:, low.nj:2 * low.nj] = np.random.default_rng(seed + 2).uniform(-0.8, 0.8, (n, low.nj))   # deflections up to 1.6, as in the base
    k = turns(n, low.nj, seed + 100)
    return wind(x, k, low.nj), u, k


def _draw_within_bound(rng, nj, rotation):
    """-> q ~ U(-pi, pi)^nj with rotation(q) <= ROT_BOUND, the number of draws that were thrown away"""
    for tries in range(1000):
        q = rng.uniform(-np.pi, np.pi, nj)
        if rotation(q) <= ROT_BOUND:
            return q, tries
    raise AssertionError("no state within the bound in 1000 draws")


def quadrant_candidate(oracle, low, seed):
    """-> xs, us, share of redrawn states.  The state of knot t, trajectory b is checked on the model of knot t against
    trajectory b's reference."""
    xs, us = gc.random_candidate(low, seed)
    rng = np.random.default_rng(seed + 200)
    nj = low.nj
    redrawn = 0
    for t in range(low.T + 1):
        for b in range(low.B):
            q, tries = _draw_within_bound(rng, nj, lambda q: residual_rotation(oracle, low, int(low.node_model[t]), q, _ref_of(low, b)))
            redrawn += tries > 0
            xs[t, b, :nj] = q
            xs[t, b, nj:2 * nj] = q + rng.uniform(-0.3, 0.3, nj)
    share = redrawn / float((low.T + 1) * low.B)
    print("Q candidate of %d states: %.1f %% redrawn" % ((low.T + 1) * low.B, 100.0 * share))
    return xs, us, share


def quadrant_points(oracle, low, seed, n):
    """-> q [n, nj] of the Q family for the point evaluators (every model of `low`, trajectory 0's reference), share of
    redrawn points"""
    rng = np.random.default_rng(seed + 300)
    drawn = [_draw_within_bound(rng, low.nj, lambda q: point_rotation(oracle, low, q)) for _ in range(n)]
    share = sum(tries > 0 for _, tries in drawn) / float(n)
    print("Q points, %d: %.1f %% redrawn" % (n, 100.0 * share))
    return np.array([q for q, _ in drawn]), share


# What "every quadrant, for positive and for negative angles" can mean on (-pi, pi): fn = rint(2 q / pi) takes -2 ... 2, so
# n = fn & 3 = 3 comes from negative angles only (fn = -1) and n = 1 from positive ones only (fn = 1); n = 0 and n = 2 come
# from both signs.  These six (sign, n) pairs are all there are, and each must occur on every joint.
QUADRANT_CLASSES = ((1, 0), (1, 1), (1, 2), (-1, 0), (-1, 3), (-1, 2))


def missing_quadrants(q):
    """(joint, sign, n) of QUADRANT_CLASSES that the link angles q [n, nj] do not reach"""
    q = np.asarray(q)
    out = []
    for j in range(q.shape[1]):
        have = set(zip(np.where(np.signbit(q[:, j]), -1, 1).tolist(), quadrant(q[:, j]).tolist()))
        out += [(j,) + c for c in QUADRANT_CLASSES if c not in have]
    return out


# ---------------------------------------------------------------------------------------------
# E points
# ---------------------------------------------------------------------------------------------
def edge_points(layout, nj, rotation=None):
    """link angles [EDGE_LAYOUTS[layout], nj].  Point i, joint j takes value number i + 11 j of its list (cyclically, so a
    7-joint chain sees the set spread over its joints); "mixed" alternates the lists along the lanes, shifted by one per
    joint.  rotation: q -> residual rotation; a point beyond ROT_BOUND moves the values of its joints >= 1 on by one
    until it is within the bound (the pairing of the values is free, the values are not)."""
    fast, library = edge_values()
    n = EDGE_LAYOUTS[layout]

    def point(i, shift):
        q = np.zeros(nj)
        for j in range(nj):
            s = shift if j else 0
            lib = layout == "library" or (layout == "mixed" and (i + j) % 2 == 1)
            vals, step = (library, i // 2 if layout == "mixed" else i) if lib else (fast, i // 2 if layout == "mixed" else i + 60)
            q[j] = vals[(step + 11 * j + s) % len(vals)]
        return q
    out = np.zeros((n, nj))
    for i in range(n):
        for shift in range(200):
            out[i] = point(i, shift)
            if rotation is None or rotation(out[i]) <= ROT_BOUND:
                break
        else:
            raise AssertionError("no pairing of E values within the bound at point %d" % i)
    return out


def states_at(low, q, seed):
    """x [n, nx], u [n, nu] for the point evaluators at link angles q [n, nj]: motor angle = link angle + U(-0.3, 0.3),
    velocities and controls drawn as gc.random_candidate draws them"""
    rng = np.random.default_rng(seed)
    n, nj = q.shape
    x = rng.uniform(-0.8, 0.8, (n, low.nx))
    u = rng.uniform(-1.0, 1.0, (n, low.nu))
    if low.dam == _abi.DAM_VSA:
        u[:, low.nu // 2:] = rng.uniform(0.1, 5.0, (n, low.nu // 2))
    x[:, :nj] = q
    x[:, nj:2 * nj] = q + rng.uniform(-0.3, 0.3, (n, nj))
    return x, u


# ---------------------------------------------------------------------------------------------
# wound forward passes
# ---------------------------------------------------------------------------------------------
# An angle of 1e5 has an ulp of 1.5e-11, 1e5 times that of an unwound angle, so every knot's q + dt v and every spring
# deflection q_l - q_m round by that much, and the motor inertia (1e-3) turns it into 1e-8 of acceleration: a roll-out
# of 20 knots from a wound state is only defined to a few 1e-9 in float64.  FORWARD_ORACLE_ERROR is the oracle's own
# distance (max |a - b| / (1 + |b|) over xs_try and us_try) from hp_rollout, the same roll-out at 40 digits, taken per
# step length at the trajectory that moves most when x0's angles go to neighbouring doubles (oracle_rollout_error;
# tests/test_angle_range_host.py repeats the measurement).  The kernels round the wound angles as the oracle does, so the
# GPU test still holds them to the oracle at the 1e-9 of the unwound suites.
FEEDFORWARD_DAMPING = 0.25     # on top of gc.forward_inputs' 0.05: with the full term one VSA roll-out reaches 1e22
# measured over all ten step lengths, B = 70 (the arm: 5), T = 20: 1.637e-9, 1.510e-9, 1.571e-9, rounded up
FORWARD_ORACLE_ERROR = {"two_dof_sea": 1.64e-9, "two_dof_vsa_boxddp": 1.52e-9, "talos_arm_sea": 1.58e-9}


def wound_forward_case(oracle, sc, seed=5):
    """-> sc, low, sp, xs, us, K, k of a forward pass from a wound candidate on which no roll-out runs away: the gains are
    those of gc.forward_inputs on the UNWOUND candidate (on the wound one the state regulariser's gradient, weight x 1e5,
    makes the feed-forward term so large that up to a third of the roll-outs reach 1e24), the feed-forward term damped by
    FEEDFORWARD_DAMPING; candidate and x0 are then wound by the same k (the roll-out starts at the problem's x0)."""
    from aslr_to_amd import scenarios
    low = scenarios.lower(sc)
    sp = scenarios.solver_params(sc)
    xs, us, K, k, _ = gc.forward_inputs(oracle, low, sp, seed, False)
    k_turns = turns(low.B, low.nj, seed + 100)
    sc = dict(sc, x0=wind(np.asarray(sc["x0"], dtype=np.float64), k_turns, low.nj))
    return sc, scenarios.lower(sc), sp, wind(xs, k_turns, low.nj), us, K, FEEDFORWARD_DAMPING * k


def hp_rollout(sc, low, sp, b, alpha, xs, us, K, k):
    """The roll-out of trajectory b (DDP / BoxDDP forward pass, Euler step of the SEA / VSA models) at 40 digits, written
    from the model equations: u = us - alpha k - K (x - xs), clipped to the box under SolverBoxDDP; M a_l = -nle - K_s (q_l
    - q_m), B a_m = tau_m + K_s (q_l - q_m); q += v dt + a dt^2, v += a dt.  -> xs_try [T+1, nx], us_try [T, nu], rounded
    once."""
    import mpmath as mp
    import _hp_geometry as hp
    nj, nu = low.nj, low.nu
    with mp.workdps(hp.DPS):
        ch = hp.Chain(sc["terminal"].state.pinocchio)
        x = hp._vec(low.x0[b])
        X, U = [x], []
        for t in range(low.T):
            m = low.desc.models[int(low.node_model[t])]
            dt = mp.mpf(m.dt)
            u = hp._vec(us[t, b]) - hp._vec(k[t, b]) * mp.mpf(alpha) - hp._mpf_matrix(K[t, b]) * (x - hp._vec(xs[t, b]))
            if sp.solver == _abi.SOLVER_BOXDDP and m.has_u_limits:
                u = mp.matrix([min(max(u[i], mp.mpf(m.u_lb[i])), mp.mpf(m.u_ub[i])) for i in range(nu)])
            ql, qm, vl = x[0:nj], x[nj:2 * nj], x[2 * nj:3 * nj]
            if low.dam == _abi.DAM_VSA:
                spring = mp.matrix([u[nj + i] * (ql[i] - qm[i]) for i in range(nj)])
                tau_m = mp.matrix([u[i] for i in range(nj)])
            else:
                spring = hp._mpf_matrix(np.array(m.K[:nj * nj]).reshape(nj, nj)) * (ql - qm)
                tau_m = hp._mpf_matrix(np.array(m.S[:nj * nu]).reshape(nj, nu)) * u
            a = list(mp.lu_solve(ch.mass_matrix(ql), -ch.nle(ql, vl) - spring))
            a += list(mp.lu_solve(hp._mpf_matrix(np.array(m.B[:nj * nj]).reshape(nj, nj)), tau_m + spring))
            xn = mp.matrix(4 * nj, 1)
            for i in range(2 * nj):
                xn[i] = x[i] + x[2 * nj + i] * dt + a[i] * dt * dt
                xn[2 * nj + i] = x[2 * nj + i] + a[i] * dt
            U.append(u)
            X.append(xn)
            x = xn
        return np.array([hp.to_np(v) for v in X]), np.array([hp.to_np(v) for v in U])


def oracle_rollout_error(oracle, case, alpha_indices):
    """-> the worst distance of the oracle's roll-out from hp_rollout over the given step lengths, each taken at the
    trajectory whose oracle roll-out moves most when the angles of x0 go to neighbouring doubles"""
    from aslr_to_amd import scenarios
    sc, low, sp, xs, us, K, k = case
    nj = low.nj
    x0 = np.array(low.x0, dtype=np.float64)
    x0[:, :2 * nj] = np.nextafter(x0[:, :2 * nj], x0[:, :2 * nj] + np.random.default_rng(6).normal(size=(low.B, 2 * nj)))
    low_next = scenarios.lower(dict(sc, x0=x0))
    worst = 0.0
    for a in alpha_indices:
        ref, nxt = (oracle.forward_pass(l, sp, 0.5 ** a, xs, us, K, k) for l in (low, low_next))
        assert not ref[3].any() and not nxt[3].any()
        b = int(np.argmax([gc.relerr(nxt[0][:, i], ref[0][:, i]) for i in range(low.B)]))
        X, U = hp_rollout(sc, low, sp, b, 0.5 ** a, xs, us, K, k)
        worst = max(worst, gc.relerr(ref[0][:, b], X), gc.relerr(ref[1][:, b], U))
    return worst
