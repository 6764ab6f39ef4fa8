"""Shared by tests/test_model_switch_host.py and tests/test_gpu_model_switch.py, imported like _gpu_case (`import _model_switch
as ms`): horizons whose knots take THREE distinct running action models, so that every kernel's per-knot model switch
(node_model_at) is taken at every kind of seam, and the inputs and oracle answers of the kernel-level cases built on them.

The models differ in everything a sweep kernel reads per model:
  A  the scenario's running model with a control box (its own for two_dof_vsa_boxddp, the tight one for the 7-joint VSA,
     torques in +-0.6 for the SEA arms);
  B  dt x 0.5, NO control limits, uReg weight x 5 and, for SEA without a table, diag K x 1.5 and diag motor inertia x 0.8;
  C  dt x 2, a narrower box (torques +-0.3; stiffness commands in [2, 20] at 7 joints, [0.5, 4] at 2), xReg weight x 3.
With a per-trajectory table (SEA only here) the models differ in dt, box presence and weights; K, B and the box of every
boxed knot come from the table's rows, whose torque boxes +-U(0.3, 0.6) are narrower than A's.

SEQ7 places them so that a sweep meets a switch after the first knot, a repeat, a return to model 0 (the `m_loaded` path of
the rollouts) and a switch into the last running knot (the first record the backward sweeps prefetch); SEQ_CYCLE switches
at every knot, so every seam of a split rollout falls on a switch.  shifted() rolls the running part of the node table by
one knot: the references of a kernel that is one knot off, which tests/test_model_switch_host.py holds apart from the true
ones on the oracle alone.

The cases are computed once and shared, read-only, by both suites."""
import copy
import ctypes as C

import numpy as np

import _gpu_case as gc
import _traj_oracle
from aslr_to_amd import _abi, scenarios
from aslr_to_amd.lowering import LoweredProblem

SEQ7 = (0, 1, 1, 2, 0, 2, 1)
SEED = 5        # of the candidates (on the oracle alone no rollout of any forward case fails or exceeds |x| = 3e3 with it)
K0_SEED = 5     # of the backward sweeps' stored k, the box QP's warm start
XREG = 1e-3
SEA_BOX_A, TORQUE_BOX_C = 0.6, 0.3
STIFFNESS_BOX_C = {7: (2.0, 20.0), 2: (0.5, 4.0)}
TABLE_BOX = (0.3, 0.6)   # the table's torque boxes: +-U(0.3, 0.6) per trajectory and control


def SEQ_CYCLE(T):
    return tuple(t % 3 for t in range(T))


def scenario(name, B, T, seq, table=False, seed=4):
    """scenarios.SCENARIOS[name] with its running list replaced by the models A, B, C placed by `seq` (sc["seq"])"""
    seq = tuple(seq)
    assert len(seq) == T and set(seq) == {0, 1, 2} and seq.index(0) < seq.index(1) < seq.index(2)   # (numbered as lowered)
    kw = dict(tight=True) if name == "talos_arm_vsa" else {}
    sc = scenarios.SCENARIOS[name](B=B, T=T, seed=seed, **kw)
    a = sc["running"][0]
    nu, nj = a.nu, a.state.pinocchio.nv
    vsa = a.differential.dam == _abi.DAM_VSA
    assert not (table and vsa), "a table is built for the SEA scenarios only"
    if not vsa:
        a.u_lb, a.u_ub = np.full(nu, -SEA_BOX_A), np.full(nu, SEA_BOX_A)
    assert a.has_control_limits
    memo = lambda: {id(a.state): a.state, id(a.state.pinocchio): a.state.pinocchio}   # same robot model object
    b, c = copy.deepcopy(a, memo()), copy.deepcopy(a, memo())
    b.dt = 0.5 * a.dt
    b.u_lb, b.u_ub = np.full(nu, -np.inf), np.full(nu, np.inf)
    b.differential.costs.costs["uReg"].weight = 5.0 * a.differential.costs.costs["uReg"].weight
    if not vsa and not table:
        b.differential.K = np.array(a.differential.K) * (1.0 + 0.5 * np.eye(nj))
        b.differential.B = np.array(a.differential.B) * (1.0 - 0.2 * np.eye(nj))
    c.dt = 2.0 * a.dt
    c.u_lb, c.u_ub = np.full(nu, -TORQUE_BOX_C), np.full(nu, TORQUE_BOX_C)
    if vsa:
        c.u_lb[nu // 2:], c.u_ub[nu // 2:] = STIFFNESS_BOX_C[nj]
    c.differential.costs.costs["xReg"].weight = 3.0 * a.differential.costs.costs["xReg"].weight
    models = (a, b, c)
    sc["running"] = [models[i] for i in seq]
    sc["seq"] = tuple(seq)
    if table:
        sc = scenarios.with_traj_params(sc, seed=seed + 1)
        w = np.random.default_rng(seed + 2).uniform(TABLE_BOX[0], TABLE_BOX[1], (B, nu))
        sc["traj_params"]["u_lb"], sc["traj_params"]["u_ub"] = -w, w
    return sc


def lowered(sc):
    low = scenarios.lower(sc)
    assert low.desc.nmodels == 4 and list(low.node_model) == list(sc["seq"]) + [3]
    has = [int(low.desc.models[i].has_u_limits) for i in range(4)]
    assert has == [1, 0, 1, 0], has
    return low


def shifted(low):
    """the same lowered problem with the running part of its node table rolled by one knot (knot t takes the model of knot
    t - 1, knot 0 that of the last running knot).  For the oracle only."""
    desc = _abi.ProblemDesc()
    C.memmove(C.byref(desc), C.byref(low.desc), C.sizeof(desc))
    node_model = np.ascontiguousarray(np.concatenate([np.roll(low.node_model[:low.T], 1), low.node_model[low.T:]]).astype(np.int32))
    assert (node_model[:low.T] != low.node_model[:low.T]).any()
    desc.node_model = node_model.ctypes.data_as(C.POINTER(C.c_int32))
    out = LoweredProblem(desc, node_model, low.x0, low.frame_ref, low.nj, low.nx, low.nu, low.dam, low.nu_user, low.traj_params)
    out.ref_path = low.ref_path
    return out


class _TableOracle(object):
    """the calls of oracle.pyoracle the cases make, through the per-trajectory loop of tests/_traj_oracle.py"""

    def __init__(self, oracle):
        self.oracle = oracle

    def calc_diff(self, low, xs, us):
        return _traj_oracle.calc_diff(self.oracle, low, xs, us)

    def backward_pass(self, low, sp, deriv, gaps, us, xreg, feasible, kff0=None):
        assert np.ndim(feasible) == 0
        kff0 = np.zeros((low.T, low.B, low.nu)) if kff0 is None else kff0
        return _traj_oracle.backward_pass(self.oracle, low, sp, deriv, gaps, us, xreg, feasible, kff0)

    def forward_pass(self, low, sp, alpha, xs, us, K, k, gaps=None, feasible=None):
        assert gaps is None and feasible is None
        return _traj_oracle.forward_pass(self.oracle, low, sp, alpha, xs, us, K, k)


def oracle_for(oracle, low):
    """the oracle that honours the problem's table where it has one"""
    return _TableOracle(oracle) if low.traj_params else oracle


def bounds(low):
    """-> lb, ub [T, B, nu]: each running knot's own box (the table's rows on a boxed knot where it has them), +-inf where
    the knot's model has none"""
    T, B, nu = low.T, low.B, low.nu
    lb, ub = np.full((T, B, nu), -np.inf), np.full((T, B, nu), np.inf)
    tp = low.traj_params or {}
    for t in range(T):
        m = low.desc.models[int(low.node_model[t])]
        if m.has_u_limits:
            lb[t] = tp["u_lb"] if "u_lb" in tp else np.array(m.u_lb[:nu])
            ub[t] = tp["u_ub"] if "u_ub" in tp else np.array(m.u_ub[:nu])
    return lb, ub


def knots_of(low, mi):
    """mask [T] of the running knots of model mi"""
    return np.asarray(low.node_model[:low.T]) == mi


def candidate(low, seed=SEED):
    """gc.random_candidate with the controls clipped per knot to that knot's box where it has one"""
    xs, us = gc.random_candidate(low, seed)
    return xs, np.clip(us, *bounds(low))


_CASES = {}


def _cached(key, make):
    if key not in _CASES:
        _CASES[key] = make()
    return _CASES[key]


def problem(name, B, T, seq, table=False):
    """-> (sc, low) of one horizon, built once"""
    def make():
        sc = scenario(name, B, T, seq, table)
        return sc, lowered(sc)
    return _cached(("problem", name, B, T, tuple(seq), table), make)


# (a) calc / calcDiff: (scenario, B, table), T = 7 with SEQ7
CALC_CASES = [("two_dof_sea", 70, False), ("two_dof_vsa_boxddp", 70, False), ("talos_arm_sea", 5, False),
              ("talos_arm_vsa", 5, False), ("two_dof_sea", 70, True), ("talos_arm_sea", 5, True)]

# (b) backward pass: (scenario, B, solver), T = 7 with SEQ7; the GPU suite adds the decompositions
BACKWARD_CASES = [("talos_arm_sea", 5, "SolverBoxDDP"), ("talos_arm_sea", 5, "SolverDDP"), ("talos_arm_vsa", 5, "SolverBoxDDP"),
                  ("two_dof_vsa_boxddp", 70, "SolverBoxDDP"), ("two_dof_sea", 70, "SolverFDDP")]


def backward_case(oracle, name, B, solver, feasible):
    """Inputs and the oracle's answer of one backward case: oracle-made records of the per-knot clipped candidate, gaps (zero
    when feasible, as in the existing box tests), a random stored k, x_reg = 1e-3."""
    def make():
        sc, low = problem(name, B, 7, SEQ7)
        sp = scenarios.solver_params(sc, solver=solver)
        xs, us, deriv, gaps = gc.backward_inputs(oracle, low, SEED, candidate=candidate(low))
        if feasible:
            gaps = np.zeros_like(gaps)
        k0 = np.random.default_rng(K0_SEED).uniform(-0.5, 0.5, us.shape)
        ref = oracle.backward_pass(low, sp, deriv, gaps, us, XREG, feasible, kff0=k0)
        return dict(low=low, sp=sp, xs=xs, us=us, deriv=deriv, gaps=gaps, k0=k0, feasible=feasible, ref=ref,
                    boxed=solver == "SolverBoxDDP" and bool(feasible))
    return _cached(("backward", name, B, solver, feasible), make)


def clamped_share(low, qu, mi):
    """share of the (knot, control) pairs on the knots of model mi whose Qu is exactly 0: the box QP clamped them"""
    return float((qu[knots_of(low, mi)] == 0.0).mean())


# (c) forward pass: (scenario, B, T, solver, table); T = 7 with SEQ7, T = 17 with SEQ_CYCLE (the split rollout)
FORWARD_CASES = [("talos_arm_sea", 5, 7, "SolverFDDP", False), ("talos_arm_sea", 5, 7, "SolverBoxDDP", False),
                 ("talos_arm_vsa", 5, 7, "SolverBoxDDP", False), ("talos_arm_sea", 5, 7, "SolverBoxDDP", True),
                 ("two_dof_vsa_boxddp", 70, 17, "SolverBoxDDP", False), ("two_dof_sea", 70, 17, "SolverFDDP", False)]


X_BOUND = 3e3
# The one forward case whose rollouts do not all stay within X_BOUND, whatever the seed (80 tried, 8 - 23 of the 70 trajectories
# leave it each time): on the planar VSA arm model B leaves the STIFFNESS commands without limits, and once x - xs has grown
# (motor inertia 1e-3: the motor velocities gain ~10 per knot) the feedback term takes them below zero on a B knot, from where the
# step diverges.  The suites compare the trajectories that stay within it (c["keep"]) and hold their number from below.
UNBOUNDED_FORWARD_CASES = {("two_dof_vsa_boxddp", 70, 17, "SolverBoxDDP", False): 0.6}


def forward_case(oracle, name, B, T, solver, table):
    """Inputs and the oracle's answers for every step length of one forward case (the recipe of tests/test_gpu_forward_seam.py:
    mild gains from the oracle's backward pass; FDDP: odd trajectories feasible, even ones not)."""
    def make():
        sc, low = problem(name, B, T, SEQ7 if T == 7 else SEQ_CYCLE(T), table)
        orc = oracle_for(oracle, low)
        sp = scenarios.solver_params(sc, solver=solver)
        fddp = solver == "SolverFDDP"
        feasible = (np.arange(low.B) % 2).astype(np.int32) if fddp else 1
        xs, us, K, k, gaps, ref_b = gc.forward_inputs(orc, low, sp, SEED, fddp, feasible=feasible if fddp else None, full=True,
                                                      candidate=candidate(low))
        c = dict(low=low, sp=sp, fddp=fddp, feasible=feasible, xs=xs, us=us, K=K, k=k, gaps=gaps,
                 boxed=solver == "SolverBoxDDP", vxxf=np.einsum("tbij,tbj->tbi", ref_b["Vxx"], gaps))
        c["ref"] = [forward_ref(orc, c, low, 0.5 ** a) for a in range(_abi.NALPHA)]
        # the trajectories no step length takes beyond |x| = X_BOUND: the ones a comparison to rounding error makes sense on
        c["keep"] = np.all([(np.abs(r[0]).max(axis=(0, 2)) < X_BOUND) & (r[3] == 0) for r in c["ref"]], axis=0)
        return c
    return _cached(("forward", name, B, T, solver, table), make)


def forward_ref(orc, c, low, alpha):
    """the oracle's forward pass of the case's inputs on `low` (the case's own problem, or shifted() of it)"""
    if c["fddp"]:
        return orc.forward_pass(low, c["sp"], alpha, c["xs"], c["us"], c["K"], c["k"], c["gaps"], c["feasible"])
    return orc.forward_pass(low, c["sp"], alpha, c["xs"], c["us"], c["K"], c["k"])


def on_bound(low, us_try):
    """bool [T, B, nu]: the control sits on a bound of its own knot's box"""
    lb, ub = bounds(low)
    return (us_try == lb) | (us_try == ub)


# (d) extension kernels: (scenario, B, table), T = 7 with SEQ7
EXT_CASES = [("two_dof_sea", 70, False), ("two_dof_sea", 70, True), ("talos_arm_sea", 5, False), ("talos_arm_sea", 5, True)]
POLICY_S = 3   # samples per trajectory of the policy roll-out


def ext_case(oracle, name, B, table):
    """-> dict(sc, low, sp, xs, us): seeded controls inside each knot's box and their open-loop roll-out on the oracle (the
    candidate of tests/_covariance.candidate), SolverBoxDDP for the gains"""
    def make():
        import _policy as pol
        sc, low = problem(name, B, 7, SEQ7, table)
        us = np.clip(np.random.default_rng(3).uniform(-1.0, 1.0, (low.T, low.B, low.nu)), *bounds(low))
        zx, zk = np.zeros((low.T + 1, low.nx)), np.zeros((low.T, low.nu, low.nx))
        xs = np.stack([pol.rollout_one(oracle, low, b, zx, us[:, b], zk)["xs"] for b in range(low.B)], axis=1)
        return dict(sc=sc, low=low, xs=xs, us=us, sp=scenarios.solver_params(sc, solver="SolverBoxDDP"))
    return _cached(("ext", name, B, table), make)


def policy_perturbations(low, S, seed=17):
    """seeded, batch-major dx0 and disturbance in the ranges of tests/_policy.perturbations; no plant arrays, so that every
    knot runs on its own model's K and B"""
    rng = np.random.default_rng(seed)
    return dict(dx0=rng.uniform(-1e-2, 1e-2, (low.B, S, low.nx)), disturbance=rng.uniform(-1e-3, 1e-3, (low.B, S, low.T, low.nx)))


# (e) full solves: (scenario, solver), B = 3, T = 30 with SEQ_CYCLE(30), cold start
SOLVE_CASES = [("talos_arm_sea", "SolverBoxDDP"), ("talos_arm_vsa", "SolverBoxDDP")]
SOLVE_B, SOLVE_T, SOLVE_MAXITER = 3, 30, 40


def solve_case(oracle, name, solver, maxiter=SOLVE_MAXITER):
    def make():
        sc, low = problem(name, SOLVE_B, SOLVE_T, SEQ_CYCLE(SOLVE_T))
        sp = scenarios.solver_params(sc, solver=solver, maxiter=maxiter)
        return dict(sc=sc, low=low, sp=sp, ref=oracle.solve(low, sp))
    return _cached(("solve", name, solver, maxiter), make)


def perturbed_solve(oracle, c, rel):
    """the oracle's solve of the case from x0 (1 + rel): the reference against itself"""
    low = c["low"]
    desc = _abi.ProblemDesc()
    C.memmove(C.byref(desc), C.byref(low.desc), C.sizeof(desc))
    x0 = np.ascontiguousarray(low.x0 * (1.0 + rel))
    desc.x0 = x0.ctypes.data_as(C.POINTER(C.c_double))
    lp = LoweredProblem(desc, low.node_model, x0, low.frame_ref, low.nj, low.nx, low.nu, low.dam, low.nu_user)
    return oracle.solve(lp, c["sp"])
