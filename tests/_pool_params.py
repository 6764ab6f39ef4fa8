"""The seeded design sweeps of the pool-with-parameters tests (aslr_solve_pool_params): P problems of one scenario, each with
its own x0 and target (the scenario's batch inputs) AND its own stiffness, motor inertia and control box.

Draws, from default_rng(seed) in this order -- stiffness (SEA only), motor inertia, box (scenarios with limits only):
  stiffness, motor inertia   the scenario's constants times a factor log-uniform in [1/2, 2], per problem and joint;
                             talos_arm_sea draws its motor inertia's factor in [32, 128] instead (as wide, 64x up): at the
                             maxiter = 12 of that case no seed converges on 90 % of the problems with B around the
                             scenario's 1e-3, with B in 0.03 .. 0.13 most seeds do (the scans are in DESIGN.md section 4.13);
  u_lb, u_ub                 the scenario's box, both bounds of an entry scaled by ONE factor uniform in [0.6, 1], per
                             problem and control (lb <= ub is kept: a bound pair keeps its signs and its order).
The yardstick of the GPU tests is ONE batched solve of the same P problems on a handle whose parameter table holds the same
rows (tests/test_gpu_traj_params.py holds that path to the per-trajectory oracle), so the draws only have to make that
comparison worth something: tests/test_pool_params_host.py asserts, on the CPU oracle alone, that each case converges on
>= 90 % of its problems and that its iteration counts differ."""
import numpy as np

from aslr_to_amd import scenarios

FACTOR = (0.5, 2.0)       # stiffness and motor inertia, log-uniform
BOX_FACTOR = (0.6, 1.0)   # control box, uniform

# scenario -> constructor arguments, solver, P, slots, T, maxiter (None: the scenario's), the fields the pool is given,
# the (refill_every, subshards) pairs the GPU test runs, the seed of the scenario's batch inputs and the seed of the draws,
# the range of the motor inertia's factor where it is not FACTOR
CASES = {
    "two_dof_sea": dict(make=scenarios.two_dof_sea, kw={}, solver="SolverFDDP", P=150, slots=40, T=25, maxiter=60,
                        fields=("stiffness", "motor_inertia"), runs=((1, 1), (3, 2)), seed=6, draw_seed=21),
    "two_dof_vsa_boxddp": dict(make=scenarios.two_dof_vsa_boxddp, kw={}, solver="SolverBoxDDP", P=200, slots=64, T=20,
                               maxiter=None, fields=("motor_inertia", "u_lb", "u_ub"), runs=((1, 1), (3, 2)), seed=4,
                               draw_seed=22),
    "talos_arm_sea": dict(make=scenarios.talos_arm_sea, kw={}, solver="SolverFDDP", P=14, slots=6, T=20, maxiter=12,
                          fields=("stiffness", "motor_inertia"), runs=((2, 1),), seed=9, draw_seed=23,
                          inertia_factor=(32.0, 128.0)),
    "talos_arm_vsa": dict(make=scenarios.talos_arm_vsa, kw=dict(tight=True), solver="SolverBoxDDP", P=10, slots=4, T=12,
                          maxiter=None, fields=("motor_inertia", "u_lb", "u_ub"), runs=((2, 1),), seed=3, draw_seed=24),
}


def draw(sc, seed, factor=FACTOR, box_factor=BOX_FACTOR, inertia_factor=None):
    """-> dict(stiffness, motor_inertia, u_lb, u_ub): [P, nj] / [P, nu] arrays for the P problems of scenario `sc`, None
    where the scenario has nothing to vary (stiffness for VSA, bounds without limits).  inertia_factor: the range of the
    motor inertia's factor where it is not `factor`."""
    rng = np.random.default_rng(seed)
    P = np.atleast_2d(sc["x0"]).shape[0]
    m = sc["running"][0]
    low = m.lower()
    nj, nu = m.state.pinocchio.nv, m.nu
    Kd = np.array(low.K[:nj * nj]).reshape(nj, nj).diagonal()
    Bd = np.array(low.B[:nj * nj]).reshape(nj, nj).diagonal()
    logu = lambda r, n: np.exp(rng.uniform(np.log(r[0]), np.log(r[1]), (P, n)))
    out = dict(stiffness=None, motor_inertia=None, u_lb=None, u_ub=None)
    if low.dam == 0:
        out["stiffness"] = Kd * logu(factor, nj)
    out["motor_inertia"] = Bd * logu(factor if inertia_factor is None else inertia_factor, nj)
    if low.has_u_limits:
        f = rng.uniform(box_factor[0], box_factor[1], (P, nu))
        out["u_lb"] = np.asarray(m.u_lb, dtype=float)[None] * f
        out["u_ub"] = np.asarray(m.u_ub, dtype=float)[None] * f
    return out


def case(name, P=None, T=None, fields=None):
    """-> dict: sc (the scenario with B = P problems), sp, params (the drawn fields the case gives the pool, by name), table
    (the same as a traj_params dict for scenarios.lower: fields not given are None), slots, runs.  P, T, fields override the
    case's (the smaller tests)."""
    c = CASES[name]
    P, T = c["P"] if P is None else P, c["T"] if T is None else T
    fields = c["fields"] if fields is None else fields
    sc = c["make"](B=P, T=T, seed=c["seed"], **c["kw"])
    kw = dict(solver=c["solver"])
    if c["maxiter"] is not None:
        kw["maxiter"] = c["maxiter"]
    sp = scenarios.solver_params(sc, **kw)
    drawn = draw(sc, c["draw_seed"], inertia_factor=c.get("inertia_factor"))
    table = {k: (drawn[k] if k in fields else None) for k in drawn}
    params = {k: v for k, v in table.items() if v is not None}
    return dict(sc=sc, sp=sp, params=params, table=table, P=P, T=T, slots=c["slots"], runs=c["runs"])


def batch_scenario(c):
    """the P problems as one batch with the parameter table: the yardstick's input"""
    return dict(c["sc"], traj_params=c["table"])


def slot_scenario(c, slots=None):
    """an engine of `slots` trajectories of the same structure (its own problems are the first `slots` of the pool)"""
    n = c["slots"] if slots is None else slots
    return dict(c["sc"], x0=c["sc"]["x0"][:n], frame_refs=c["sc"]["frame_refs"][:n])
