"""High-precision reference for the geometry of a fixed-base revolute chain and the SE(3) log (mpmath, 40 digits).

Written from first principles, not from the oracle's formulas:
- the SE(3) log is mpmath's matrix logarithm of the 4x4 homogeneous matrix, read as [v; w] (taken of the matrix's
  principal square root and doubled, which keeps logm on the principal branch near a half turn);
- Jlog6 is the central difference of that log under right perturbations M expm(d^);
- joint rotations are exponentials of the joint axis' skew matrix (the series summed in closed form);
- M(q) is built from body Jacobians (angular columns: world joint axes, linear columns: axis x (c - p_joint));
- the gravity torque is dV/dq, nle(q, v) comes from the Lagrangian, Mdot v - 1/2 d(v^T M v)/dq + dV/dq, and the RNEA
  derivatives are differences of tau = M a + nle, all with mp.diff;
- the LOCAL frame Jacobian is read off the derivative of the frame placement: [R^T dp/dq_j ; vee(R^T dR/dq_j)].
Test infrastructure only; slow (pure Python), so callers keep point counts small.
"""
import numpy as np
import mpmath as mp

DPS = 40


def _mpf_matrix(a):
    a = np.asarray(a, dtype=float)
    return mp.matrix([[mp.mpf(float(v)) for v in row] for row in np.atleast_2d(a)])


def _vec(a):
    return mp.matrix([mp.mpf(float(v)) for v in np.asarray(a, dtype=float).ravel()])


def _skew(w):
    return mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


def _vee(W):
    return mp.matrix([(W[2, 1] - W[1, 2]) / 2, (W[0, 2] - W[2, 0]) / 2, (W[1, 0] - W[0, 1]) / 2])


def _cross(a, b):
    return mp.matrix([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def _dot(a, b):
    return sum(a[i] * b[i] for i in range(len(a)))


def to_np(m):
    """mpmath matrix -> float64 array (each entry rounded once); a column comes back as a vector."""
    a = np.array([[float(m[i, j]) for j in range(m.cols)] for i in range(m.rows)])
    return a[:, 0] if m.cols == 1 else a


def _rotation(axis, t):
    """exp(t [axis]x) for a unit axis, summed in closed form (the exponential series of a skew matrix)."""
    K = _skew(axis)
    return mp.eye(3) + mp.sin(t) * K + (1 - mp.cos(t)) * (K * K)


def _real(m):
    return mp.matrix([[mp.re(m[i, j]) for j in range(m.cols)] for i in range(m.rows)])


# ---------------------------------------------------------------------------------------------
# SE(3) log and its Jacobian
# ---------------------------------------------------------------------------------------------
def homogeneous(R, p):
    """4x4 mpmath matrix of (R, p) given in float64 (taken exactly)."""
    H = mp.zeros(4, 4)
    Rm, pm = _mpf_matrix(np.asarray(R).reshape(3, 3)), _vec(p)
    for i in range(3):
        for j in range(3):
            H[i, j] = Rm[i, j]
        H[i, 3] = pm[i]
    H[3, 3] = 1
    return H


def _half(H):
    """The principal square root of a homogeneous matrix: rotation block S = Q diag(sqrt(lambda)) Q^-1 from the
    eigenvectors of R, translation y from S y + y = p.  mpmath's logm finds its square roots by a Denman-Beavers
    iteration, which leaves the principal branch when R turns by nearly pi (eigenvalues near -1); at half the angle it
    does not."""
    E, Q = mp.eig(H[0:3, 0:3])
    S = _real(Q * mp.diag([mp.sqrt(e) for e in E]) * mp.inverse(Q))
    y = mp.lu_solve(S + mp.eye(3), H[0:3, 3])
    Hh = mp.eye(4)
    for i in range(3):
        for j in range(3):
            Hh[i, j] = S[i, j]
        Hh[i, 3] = y[i]
    return Hh


def _log_of_h(H):
    """[v; w] of log(H) = 2 logm(H^(1/2))."""
    L = 2 * _real(mp.logm(_half(H)))
    w = _vee(L[0:3, 0:3])
    return mp.matrix([L[0, 3], L[1, 3], L[2, 3], w[0], w[1], w[2]])


def _hat6(d):
    X = mp.zeros(4, 4)
    S = _skew([d[3], d[4], d[5]])
    for i in range(3):
        for j in range(3):
            X[i, j] = S[i, j]
        X[i, 3] = d[i]
    return X


def log6(R, p):
    """pinocchio.log6(M).vector of the float64 placement (R, p): [v; w] as float64."""
    with mp.workdps(DPS):
        return to_np(_log_of_h(homogeneous(R, p)))


def jlog6(R, p, h="1e-15"):
    """d log6(M expm(d^)) / dd at d = 0, by central differences with |d| = h at DPS digits (truncation ~h^2)."""
    with mp.workdps(DPS):
        H = homogeneous(R, p)
        h = mp.mpf(h)
        J = mp.zeros(6, 6)
        for k in range(6):
            d = mp.zeros(6, 1)
            d[k] = h
            lp = _log_of_h(H * mp.expm(_hat6(d)))
            lm = _log_of_h(H * mp.expm(_hat6(-d)))
            for i in range(6):
                J[i, k] = (lp[i] - lm[i]) / (2 * h)
        return to_np(J)


def se3_from_twist(v, w):
    """(R, p) of expm([w^ v; 0 0]) at DPS digits, rounded to float64 (test inputs: an exact group element)."""
    with mp.workdps(DPS):
        E = mp.expm(_hat6(list(_vec(v)) + list(_vec(w))))
        return to_np(E[0:3, 0:3]), to_np(mp.matrix([E[0, 3], E[1, 3], E[2, 3]]))


def translation_log_for(R, p, w):
    """The v of the log [v; w] of (R, p) for a GIVEN rotation vector w (at a rotation by pi both w and -w are logs of
    R): expm([w^ v; 0 0]) has translation V v, V linear in v, so v = V^-1 p with V's columns from expm(e_k)."""
    with mp.workdps(DPS):
        wm = _vec(w)
        V = mp.zeros(3, 3)
        for k in range(3):
            e = [mp.mpf(0)] * 3
            e[k] = mp.mpf(1)
            E = mp.expm(_hat6(e + list(wm)))
            for i in range(3):
                V[i, k] = E[i, 3]
        return to_np(mp.lu_solve(V, _vec(p)))


# ---------------------------------------------------------------------------------------------
# Rigid-body terms of a serial revolute chain (aslr_to_amd.pinocchio.ChainModel)
# ---------------------------------------------------------------------------------------------
class Chain(object):
    """A ChainModel's constants as mpmath values (exact images of the float64 tables)."""

    def __init__(self, model):
        self.nj = model.njoints
        self.g = _vec(model.gravity.linear)
        self.Rp = [_mpf_matrix(j.placement.rotation) for j in model.joints]
        self.pp = [_vec(j.placement.translation) for j in model.joints]
        self.axis = [_vec(j.axis) for j in model.joints]
        self.mass = [mp.mpf(float(j.mass)) for j in model.joints]
        self.com = [_vec(j.com) for j in model.joints]
        self.inertia = [_mpf_matrix(j.inertia) for j in model.joints]

    def kinematics(self, q):
        """world placements (R_i, p_i) of the joint frames (after the joint rotation)."""
        R, p = mp.eye(3), mp.zeros(3, 1)
        out = []
        for i in range(self.nj):
            p = p + R * self.pp[i]
            R = R * self.Rp[i] * _rotation(self.axis[i], q[i])
            out.append((R, p))
        return out

    def mass_matrix(self, q):
        kin = self.kinematics(q)
        n = self.nj
        M = mp.zeros(n, n)
        for i in range(n):
            Ri, pi = kin[i]
            c = pi + Ri * self.com[i]
            Jv, Jw = mp.zeros(3, n), mp.zeros(3, n)
            for j in range(i + 1):
                Rj, pj = kin[j]
                z = Rj * self.axis[j]
                lin = _cross(z, c - pj)
                for k in range(3):
                    Jw[k, j], Jv[k, j] = z[k], lin[k]
            Iw = Ri * self.inertia[i] * Ri.T
            M += self.mass[i] * (Jv.T * Jv) + Jw.T * Iw * Jw
        return M

    def potential(self, q):
        kin = self.kinematics(q)
        V = mp.mpf(0)
        for i in range(self.nj):
            Ri, pi = kin[i]
            V -= self.mass[i] * _dot(self.g, pi + Ri * self.com[i])
        return V

    # ---- derivatives by mp.diff (one cached function of one coordinate) ----
    @staticmethod
    def _partial(f, x, k):
        """d f(x) / d x_k for a function returning an mpmath matrix or scalar: mp.diff per entry, the evaluations of f
        shared between the entries."""
        cache = {}

        def at(s):
            if s not in cache:
                y = list(x)
                y[k] = s
                cache[s] = f(y)
            return cache[s]

        y0 = f(list(x))
        if isinstance(y0, mp.matrix):
            D = mp.zeros(y0.rows, y0.cols)
            for i in range(y0.rows):
                for j in range(y0.cols):
                    D[i, j] = mp.diff(lambda s: at(s)[i, j], x[k])
            return D
        return mp.diff(at, x[k])

    def gravity_torque(self, q):
        return mp.matrix([self._partial(self.potential, q, k) for k in range(self.nj)])

    def nle(self, q, v):
        """Mdot v - 1/2 d(v^T M v)/dq + dV/dq."""
        n = self.nj
        out = self.gravity_torque(q)
        for k in range(n):
            dM = self._partial(self.mass_matrix, q, k)
            out += (dM * v) * v[k]
            out[k] -= (v.T * dM * v)[0] / 2
        return out

    def tau(self, q, v, a):
        return self.mass_matrix(q) * a + self.nle(q, v)

    def tau_derivatives(self, q, v, a):
        n = self.nj
        dq, dv = mp.zeros(n, n), mp.zeros(n, n)
        for j in range(n):
            cq = self._partial(lambda y: self.tau(mp.matrix(y), v, a), list(q), j)
            cv = self._partial(lambda y: self.tau(q, mp.matrix(y), a), list(v), j)
            for i in range(n):
                dq[i, j], dv[i, j] = cq[i], cv[i]
        return dq, dv

    def frame_placement(self, q, joint, fR, fp):
        Rj, pj = self.kinematics(q)[joint]
        return Rj * fR, pj + Rj * fp

    def frame_jacobian_local(self, q, joint, fR, fp):
        n = self.nj
        R, _ = self.frame_placement(q, joint, fR, fp)
        J = mp.zeros(6, n)
        for j in range(n):
            dR = self._partial(lambda y: self.frame_placement(y, joint, fR, fp)[0], list(q), j)
            dp = self._partial(lambda y: self.frame_placement(y, joint, fR, fp)[1], list(q), j)
            lin, ang = R.T * dp, _vee(R.T * dR)
            for k in range(3):
                J[k, j], J[3 + k, j] = lin[k], ang[k]
        return J


def rigid_body_terms(model, q, v, a, frames=()):
    """float64 results of the reference at one state: dict(M, nle, dtau_dq, dtau_dv, frames=[(R, p, J_local)])
    for `frames` given as (joint, fR, fp)."""
    with mp.workdps(DPS):
        ch = Chain(model)
        qm, vm, am = _vec(q), _vec(v), _vec(a)
        out = dict(M=to_np(ch.mass_matrix(qm)), nle=to_np(ch.nle(qm, vm)))
        dq, dv = ch.tau_derivatives(qm, vm, am)
        out["dtau_dq"], out["dtau_dv"] = to_np(dq), to_np(dv)
        fr = []
        for joint, fR, fp in frames:
            fRm, fpm = _mpf_matrix(fR), _vec(fp)
            R, p = ch.frame_placement(qm, joint, fRm, fpm)
            fr.append((to_np(R), to_np(p), to_np(ch.frame_jacobian_local(qm, joint, fRm, fpm))))
        out["frames"] = fr
        return out
