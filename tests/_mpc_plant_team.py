"""Shared by tests/test_mpc_plant_team_host.py and tests/test_gpu_mpc_plant_team.py: the seeded 7-joint cases of
aslr_mpc_run_plant_all (include/aslr_to_amd_mpc_plant_all.h).  The reference is tests/_mpc_plant.py as it stands --
plant_phase(), shifted(), plants() and oracle_loop() do not depend on the model size; this file only builds the cases.

Shapes: mpc_plant_team_kernel runs a team of 8 lanes per trajectory and one wave of 8 teams per block, so B = 3 leaves
five idle teams, B = 9 crosses a wave and a block with one live team behind it; T = 4 is the shortest horizon on which
hold = 1, 2 and T differ and on which a reference path of 4 rows from row 2 both advances and holds its last row."""
import numpy as np

import _policy_team as pt
import _ref_path
from aslr_to_amd import _abi, scenarios

NAME = _abi.MPC_PLANT_ALL_SYMBOLS[0]    # the entry point these cases are for: without it there is nothing to condition

# the oracle-loop rows (hold = 1): the two arm rows of tests/test_mpc_host.ROWS
ROWS = [("talos_arm_sea", "SolverFDDP", 4, 20, 0),
        ("talos_arm_vsa", "SolverBoxDDP", 4, 20, 0)]
ROW_IDS = ["%s-%s" % r[:2] for r in ROWS]

PLANT_RANGE, PLANT_SEED = 0.3, 21       # the one-step cases: plants within +-30 % of the trajectory's nominal K and B
DIST, DIST_SEED = 1e-3, 7               # ... and a disturbance U(-1e-3, 1e-3)
SCENARIO_SEED = 4                       # (tests/_policy_team.scenario's)

# key -> (scenario, B, T, hold, table, path, narrowed box and clamp, plant arrays given)
ONE_STEP = {
    "sea_B3_hold1": ("talos_arm_sea", 3, 4, 1, False, False, False, True),
    "sea_B3_hold2": ("talos_arm_sea", 3, 4, 2, False, False, False, True),
    "sea_B3_hold4": ("talos_arm_sea", 3, 4, 4, False, False, False, True),
    "sea_B9_hold2": ("talos_arm_sea", 9, 4, 2, False, False, False, True),
    "sea_table": ("talos_arm_sea", 3, 4, 2, True, False, False, False),
    "sea_table_and_plants": ("talos_arm_sea", 3, 4, 2, True, False, False, True),
    "sea_path": ("talos_arm_sea", 3, 4, 2, False, True, False, True),
    "vsa_plain": ("talos_arm_vsa", 3, 4, 2, False, False, False, True),
    "vsa_box": ("talos_arm_vsa", 3, 6, 6, True, False, True, True),
}
# vsa_box: the narrowed box of _policy_team.box(7), T = 6, hold = 6 = T.  The shape was chosen on the REFERENCE's `bound` alone
# (mp.plant_phase fed a plain device solve's plan and gains): after three BoxDDP iterations the controls on the box have zero
# gain rows and the free ones sit inside it, so at T = 4 the narrowed box moves no control of the reference at hold = 2 and
# hold = 3 for any of the scenario seeds 0..23 (hold = 2: at one seed of 0..119, number 103, by 1.3e-3; hold = 3 and hold = 4:
# at about one seed in ten, always on one trajectory, by 1e-3 .. 5e-3).  Five feedback knots on T = 6 reach the box at every
# one of the seeds 0..119; _policy_team.scenario's own seed 4 is kept: the box binds on trajectory 0 and not on the others,
# and the clamped controls differ from the free ones by 4.3e-3.


def scenario(name, B, T, table=False, path=False, box=False, seed=SCENARIO_SEED):
    """the recipe of tests/_policy_team.scenario: the table of seed 5, the narrowed box of _policy_team.box(7), a reference
    path of 4 rows from row 2"""
    sc = scenarios.SCENARIOS[name](B=B, T=T, seed=seed)
    if table:
        sc = scenarios.with_traj_params(sc, seed=5)
        if box:
            lb, ub = pt.box(7)
            sc["traj_params"]["u_lb"] = np.tile(lb, (B, 1))
            sc["traj_params"]["u_ub"] = np.tile(ub, (B, 1))
    if path:
        sc = _ref_path.with_path(sc, _ref_path.random_path(sc, 4, 13), row0=2)
    return sc


def one_step(key):
    """-> dict(sc, low, sp, hold, clamp, pk, pb, dist): three SolverFDDP (SEA) / SolverBoxDDP (VSA) iterations; pk, pb batch-
    major [B, nj] or None; dist time-major [hold, B, nx]"""
    import _mpc_plant as mp
    name, B, T, hold, table, path, box, arrays = ONE_STEP[key]
    sc = scenario(name, B, T, table, path, box)
    low = scenarios.lower(sc)
    assert low.nj == 7
    sp = scenarios.solver_params(sc, solver="SolverBoxDDP" if low.dam == _abi.DAM_VSA else "SolverFDDP", maxiter=3)
    pk, pb = mp.plants(low, seed=PLANT_SEED, rng_range=PLANT_RANGE) if arrays else (None, None)
    dist = np.random.default_rng(DIST_SEED).uniform(-DIST, DIST, (hold, B, low.nx))
    return dict(sc=sc, low=low, sp=sp, hold=hold, clamp=box, pk=pk, pb=pb, dist=dist, table=table, arrays=arrays)


def reference(oracle, c, X, U, K, clamp=None, plants=True):
    """mp.plant_phase of every trajectory of the case on the plan X [T+1, B, nx], U [T, B, nu] and gains K [T, B, nu, nx]
    -> dict(x [hold+1, B, nx], u [hold, B, nu], cost [B], failed [B], bound [B]); plants=False: without the plant arrays"""
    import _mpc_plant as mp
    low, hold = c["low"], c["hold"]
    pick = lambda a, b: None if a is None or not plants else a[b]
    ref = [mp.plant_phase(oracle, low, b, X[:, b], U[:, b], K[:, b], hold, pick(c["pk"], b), pick(c["pb"], b), c["dist"][:, b],
                          c["clamp"] if clamp is None else clamp) for b in range(low.B)]
    return dict(x=np.stack([r["x"] for r in ref], axis=1), u=np.stack([r["u"] for r in ref], axis=1),
                cost=np.array([r["cost"] for r in ref]), failed=np.array([r["failed"] for r in ref], dtype=np.int32),
                bound=np.array([r["bound"] for r in ref]))
