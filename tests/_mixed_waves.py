"""Inputs that make the trajectories of ONE wave of the backward sweep part ways: some fail and retry (or give up) while
their neighbours publish, finish or ride along.  At nx = 8 a wave holds TPW = 2, 4 or 8 trajectories (teams of 32, 16, 8
lanes: ASLR_BWD_HS = 4, 2, 1) that share ballots, DPP rows, LDS slots and one retry loop; only store predicates keep a
team that is done quiet.  Everything here is chosen on the CPU oracle alone; tests/test_mixed_waves_host.py asserts the
properties the choices rest on, tests/test_gpu_mixed_waves.py runs the kernels on them.

Kernel level.  gc.backward_inputs records; on the trajectories of a failure mask, C_B is subtracted from the diagonal of
the Luu block of ONE knot t_b.  Quu = Luu + Fu^T Vxx Fu + x_reg there turns negative definite by a wide margin (the
unmodified diagonal is 0.1 or 0.01, x_reg at most 1e-1), so the sweep of such a trajectory fails in the gains of knot t_b
whatever x_reg in [0.5, 2] times its value, and the others are as well conditioned as in test_backward_pass_matches_oracle
(their records are untouched), so its tolerance of 1e-8 carries over.  Knots above t_b are computed from untouched records:
the oracle's rows there are what a kernel may have stored before it failed.

Solve level.  The recipe of test_backward_error_recovery_and_reg_max_match_oracle: a negative uReg weight makes Quu
indefinite, every sweep fails until x_reg has grown enough, and how far it must grow differs between trajectories."""
import numpy as np

import _gpu_case as gc
import _traj_oracle
from aslr_to_amd import _abi, scenarios

B, T = 19, 6                 # 8 + 8 + 3 = 4 * 4 + 3 = 2 * 9 + 1: full waves and a partial last one for every TPW
TPWS = (2, 4, 8)
C_B = 10.0                   # taken off the Luu diagonal of a failing trajectory at its knot t_b
SENTINEL = float(np.frombuffer(np.array([0x7FF8DEAD0000BEEF], dtype=np.uint64).tobytes(), dtype=np.float64)[0])  # a NaN no kernel computes


def _mask(*idx):
    m = np.zeros(B, dtype=bool)
    m[list(idx)] = True
    return m


# Failure masks over the 19 trajectories.  Between them every pattern occurs in a full group of TPW adjacent trajectories
# for TPW = 2, 4, 8 (patterns() below names them; the host test asserts the table):
#   "ends":   trajectory 0 (first of its group for every TPW), 15 (last of its group for every TPW), 17 (inside the
#             partial last wave of TPW = 4 and 8, last of a full pair at TPW = 2)
#   "dense":  0..7 but 3 (all but one of the first group of 8 and of 4, i.e. 0..3 but 3), 8 10 12 14 (alternating in the second group of
#             8, in the groups of 4 and in every pair), 16 and 18 (the partial last wave: at TPW = 2 trajectory 18 is alone
#             in it and fails, with the wave's other team past B riding along)
MASKS = {"ends": _mask(0, 15, 17), "dense": _mask(0, 1, 2, 4, 5, 6, 7, 8, 10, 12, 14, 16, 18)}


def fail_knots(mask):
    """-> t_b per trajectory (-1: none): the failing ones take T - 1 (fails at once, nothing stored), 0 (fails at the end,
    every row above already stored) and T // 2 in turn."""
    tb = np.full(B, -1)
    tb[np.nonzero(mask)[0]] = np.resize([T - 1, 0, T // 2], int(mask.sum()))
    return tb


def xregs():
    """1e-3 and 1e-1 with period 3 against the groups' 2, 4, 8: mixed inside every group of 4 and 8 and two pairs of three"""
    return np.where(np.arange(B) % 3 == 1, 1e-1, 1e-3)


def feasible_flags(kind):
    """"a" / "b": two complementary mixes (period 3 again); an int: that value for all"""
    if kind == "a":
        return (np.arange(B) % 3 != 0).astype(np.int32)
    if kind == "b":
        return (np.arange(B) % 3 == 0).astype(np.int32)
    return np.full(B, int(kind), dtype=np.int32)


def groups(tpw, n=B):
    """-> the slices of the waves: full groups of tpw adjacent trajectories, then the partial one (if any)"""
    return [slice(g, min(g + tpw, n)) for g in range(0, n, tpw)]


def patterns(fail, tpw):
    """-> the set of pattern names that occur in `fail` (bool per trajectory) for waves of tpw trajectories"""
    fail = np.asarray(fail, dtype=bool)
    found = set()
    gs = groups(tpw, fail.size)
    full = [g for g in gs if g.stop - g.start == tpw]
    for g in full:
        f = fail[g]
        if f[0] and not f[1:].any():
            found.add("only the first")
        if f[-1] and not f[:-1].any():
            found.add("only the last")
        if f.sum() == tpw - 1:
            found.add("all but one")
        if (f[::2].all() and not f[1::2].any()) or (f[1::2].all() and not f[::2].any()):
            found.add("alternating")
    if len(gs) > len(full):      # mixed failures in the partial last wave or in the full group next to it
        last, prev = fail[gs[-1]], fail[full[-1]]
        if last.any() and prev.any() and not prev.all() and not np.concatenate([prev, last]).all():
            found.add("next to the partial last wave")
    return found


PATTERNS = {"only the first", "only the last", "all but one", "alternating", "next to the partial last wave"}

# (scenario, solver) of the standalone sweeps at nx = 8: the variable-stiffness arm (nu = 4: the DPP-row gains and box QP at
# HS = 2 and 4) under every solver, and the series-elastic one (nu = 2: the per-lane gains) under SolverFDDP
KERNEL_CASES = [("two_dof_vsa_boxddp", "SolverDDP"), ("two_dof_vsa_boxddp", "SolverFDDP"),
                ("two_dof_vsa_boxddp", "SolverBoxDDP"), ("two_dof_sea", "SolverFDDP")]

_cache = {}


def spoil(low, deriv, tb, c=C_B):
    """-> a copy of the records with c off the Luu diagonal of knot tb[b] on every trajectory with tb[b] >= 0"""
    deriv = np.array(deriv).reshape(low.T + 1, low.B, low.rec)
    o = _abi.record_offsets(low.nx, low.nu)["Luu"]
    for b in np.nonzero(np.asarray(tb) >= 0)[0]:
        deriv[tb[b], b, o:o + low.nu * low.nu:low.nu + 1] -= c
    return deriv


def kernel_case(oracle, scen, solver, flags, mask_name, seed=3):
    """One standalone sweep with mixed failures, computed once and shared (callers must not write into it):
    -> dict(low, sp, us, deriv, gaps, xreg, feasible, k0, tb, ref, clean); ref: the oracle's backward pass on the spoiled
    records, clean: on the untouched ones (no failure anywhere)."""
    key = (scen, solver, str(flags), mask_name, seed)
    if key in _cache:
        return _cache[key]
    sc = scenarios.SCENARIOS[scen](B=B, T=T, seed=1)
    low = scenarios.lower(sc)
    sp = scenarios.solver_params(sc, solver=solver)
    clip, k0 = None, None
    if solver == "SolverBoxDDP":     # as test_backward_pass_with_the_wave_box_qp_matches_oracle: controls in the box, a random stored k
        m = low.desc.models[0]
        clip = (np.array(m.u_lb[:low.nu]), np.array(m.u_ub[:low.nu]))
        k0 = np.random.default_rng(seed + 2).uniform(-0.5, 0.5, (low.T, low.B, low.nu))
    _, us, deriv0, gaps = gc.backward_inputs(oracle, low, seed, clip=clip)
    tb = fail_knots(MASKS[mask_name])
    deriv = spoil(low, deriv0, tb)
    feasible, xreg = feasible_flags(flags), xregs()
    ref = oracle.backward_pass(low, sp, deriv, gaps, us, xreg, feasible, kff0=k0)
    clean = oracle.backward_pass(low, sp, deriv0, gaps, us, xreg, feasible, kff0=k0)
    case = dict(low=low, sp=sp, us=us, deriv=deriv, deriv0=deriv0, gaps=gaps, xreg=xreg, feasible=feasible, k0=k0, tb=tb,
                ref=ref, clean=clean)
    _cache[key] = case
    return case


def arm_case(oracle, vsa, seed=3):
    """nx = 28, B = 3, T = 4: trajectory 1 fails at knot 1 (of 0..3) between two that succeed.  vsa: talos_arm_vsa(tight)
    under SolverBoxDDP (feasible, controls in the box, a random stored k); else talos_arm_sea under SolverFDDP, infeasible."""
    key = ("arm", vsa, seed)
    if key in _cache:
        return _cache[key]
    sc = scenarios.talos_arm_vsa(B=3, T=4, seed=2, tight=True) if vsa else scenarios.talos_arm_sea(B=3, T=4, seed=2)
    low = scenarios.lower(sc)
    sp = scenarios.solver_params(sc, solver="SolverBoxDDP" if vsa else "SolverFDDP")
    clip, k0, feasible = None, None, 0
    if vsa:
        m = low.desc.models[0]
        clip = (np.array(m.u_lb[:low.nu]), np.array(m.u_ub[:low.nu]))
        k0 = np.random.default_rng(seed + 2).uniform(-0.5, 0.5, (low.T, low.B, low.nu))
        feasible = 1
    _, us, deriv0, gaps = gc.backward_inputs(oracle, low, seed, clip=clip)
    tb = np.array([-1, 1, -1])
    deriv = spoil(low, deriv0, tb)
    xreg = np.full(3, 1e-3)
    ref = oracle.backward_pass(low, sp, deriv, gaps, us, xreg, feasible, kff0=k0)
    clean = oracle.backward_pass(low, sp, deriv0, gaps, us, xreg, feasible, kff0=k0)
    case = dict(low=low, sp=sp, us=us, deriv=deriv, deriv0=deriv0, gaps=gaps, xreg=xreg, feasible=np.full(3, feasible, dtype=np.int32),
                k0=k0, tb=tb, ref=ref, clean=clean)
    _cache[key] = case
    return case


# ---------------------------------------------------------------------------------------------
# solve level
# ---------------------------------------------------------------------------------------------
# name -> (scenario, solver, seed, uReg weight, maxiter, solver-parameter overrides, seed of scenarios.with_traj_params or
# None).  Found by a search over seeds, weights, reg_max and parameter tables on the oracle alone (seeds 0..11, weights -5e-3
# .. -1, reg_max 1e-3 .. 1e9); the host test asserts what each is here for.  On the oracle:
#   vsa_boxddp: x_reg parts inside groups of 2, 4 and 8 in 5 of the 6 iterations; trajectory 12 stops at reg_max = 0.1 in the
#               backward sweep of its third iteration, 3 4 5 10 13 16 17 stop there later, the others run all 6.
#   sea_*:      with a stiffness / inertia table the 19 arms need different x_reg (parts in 2 iterations for every group
#               size); no seed, weight or reg_max of the search gave the two-joint SEA arm a trajectory at ST_REG_MAX
#               beside one that goes on, so that condition rests on vsa_boxddp alone.
SOLVE_CASES = {
    "vsa_boxddp": ("two_dof_vsa_boxddp", "SolverBoxDDP", 1, -5e-3, 6, dict(reg_max=0.1), None),
    "sea_fddp": ("two_dof_sea", "SolverFDDP", 2, -1e-2, 6, {}, 2),
    "sea_ddp": ("two_dof_sea", "SolverDDP", 2, -1e-2, 6, {}, 2),
}
SOLVE_B, SOLVE_T = 19, 20


def solve_case(name, x0_factor=1.0):
    """-> sc, low, sp of a solve-level case (x0 scaled by x0_factor: the host test's perturbation)"""
    scen, solver, seed, weight, maxiter, over, tp_seed = SOLVE_CASES[name]
    sc = scenarios.SCENARIOS[scen](B=SOLVE_B, T=SOLVE_T, seed=seed)
    sc["running"][0].differential.costs.costs["uReg"].weight = weight
    if tp_seed is not None:
        sc = scenarios.with_traj_params(sc, seed=tp_seed)
    if x0_factor != 1.0:
        sc = dict(sc)
        sc["x0"] = np.asarray(sc["x0"]) * x0_factor
    return sc, scenarios.lower(sc), scenarios.solver_params(sc, solver=solver, maxiter=maxiter, **over)


def solve_ref(oracle, name, x0_factor=1.0):
    key = ("solve", name, x0_factor)
    if key not in _cache:
        sc, low, sp = solve_case(name, x0_factor)
        _cache[key] = (_traj_oracle.solve(oracle, low, sp, log_cap=sp.maxiter) if low.traj_params
                       else oracle.solve(low, sp, log_cap=sp.maxiter))
    return _cache[key]


def xreg_parts_in_groups(log, tpw):
    """-> the iterations in which the logged x_reg differs inside some full group of tpw adjacent trajectories (both
    values logged, i.e. both trajectories still iterating)"""
    x = log[:, _abi.LOG_XREG]
    its = []
    for it in range(x.shape[0]):
        for g in groups(tpw, x.shape[1]):
            v = x[it, g]
            v = v[~np.isnan(v)]
            if g.stop - g.start == tpw and v.size > 1 and v.min() != v.max():
                its.append(it)
                break
    return its


def reg_max_beside_a_running_neighbour(ref, tpw):
    """-> [(b, neighbour, iterations of b)]: trajectory b ended with ST_REG_MAX and some trajectory of its group of tpw counts
    at least two iterations more, i.e. ran at least one whole iteration with b done beside it whether b stopped in a
    backward sweep (which does not count the iteration it abandons) or in the line search (which does)"""
    st, it = ref["traj_i"][_abi.TI_STATUS], ref["traj_i"][_abi.TI_ITER]
    out = []
    for g in groups(tpw, st.size):
        for b in range(g.start, g.stop):
            if st[b] & _abi.ST_REG_MAX:
                for n in range(g.start, g.stop):
                    if n != b and it[n] >= it[b] + 2:
                        out.append((b, n, int(it[b])))
                        break
    return out
