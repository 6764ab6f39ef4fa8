"""Shared by tests/test_policy_team_host.py and tests/test_gpu_policy_team.py: the seeded 7-joint cases of
aslr_policy_rollout_all (include/aslr_to_amd_policy_all.h).  The reference is tests/_policy.py as it stands -- rollout(),
perturbations() and oracle_gains() do not depend on the model size; this file only builds the cases, with the recipe of
_policy.case: the candidate is seeded controls and the oracle's open-loop roll-out of them from x0.

Shapes: policy_rollout_team_kernel runs 16 samples of one trajectory per block, 8 per wave, so S = 17 leaves a second
sample group with one live team and S = 9 a second wave with one live team; B = 3 is more than one block along the other
grid axis; T = 4 is the shortest horizon on which a reference path of 4 rows from row 2 both advances and holds its last row
and on which a second running model takes over mid-horizon."""
import copy

import numpy as np

import _policy as pol
import _ref_path
from aslr_to_amd import _abi, scenarios

# (scenario, table, path, B, S, T, two running models, clamp)
CASES = {
    "arm_sea_table": ("talos_arm_sea", True, False, 3, 17, 4, False, False),
    "arm_sea_plain": ("talos_arm_sea", False, False, 3, 9, 4, False, False),
    "arm_sea_path": ("talos_arm_sea", True, True, 3, 17, 4, False, False),
    "arm_sea_one": ("talos_arm_sea", False, False, 1, 1, 1, False, False),
    "arm_sea_two_models": ("talos_arm_sea", False, False, 3, 9, 4, True, False),
    "arm_vsa_box": ("talos_arm_vsa", True, False, 3, 17, 4, False, True),
    "arm_vsa_plain": ("talos_arm_vsa", False, False, 2, 9, 4, False, False),
}
# The narrowed box of arm_vsa_box (torques, stiffnesses).  The seeded candidate draws torques from U(-1, 1) and stiffnesses
# from U(0.1, 5) and is clipped to the box.  A control that sits ON the box leaves it in about every second sample, and with
# 14 controls on 4 knots a box inside the drawn ranges would bind on every sample; this one lies just outside them, so that
# only the feedback term of the larger perturbations reaches it (tests/test_policy_team_host.py checks that it binds on some
# samples and not on all, and that the clamp moves the controls by more than 1e-3).
BOX_TORQUE, BOX_STIFFNESS = (-1.0, 1.0), (0.1, 5.0)
SECOND_MODEL_DT = 2.0   # arm_sea_two_models: the time step of the second running model, relative to the first


def box(nj):
    return (np.array([BOX_TORQUE[0]] * nj + [BOX_STIFFNESS[0]] * nj), np.array([BOX_TORQUE[1]] * nj + [BOX_STIFFNESS[1]] * nj))


def scenario(key):
    """key: a name of CASES, or a tuple of the same fields"""
    name, table, path, B, S, T, two, clamp = CASES[key] if isinstance(key, str) else key
    sc = scenarios.SCENARIOS[name](B=B, T=T, seed=4)
    if two:   # knots 0, 1 on the scenario's running model, knots 2, 3 on a copy with another time step
        second = copy.copy(sc["running"][0])
        second.dt = SECOND_MODEL_DT * sc["running"][0].dt
        sc["running"] = [sc["running"][0]] * (T // 2) + [second] * (T - T // 2)
    if table:
        sc = scenarios.with_traj_params(sc, seed=5)
        if clamp:
            lb, ub = box(7)
            sc["traj_params"]["u_lb"] = np.tile(lb, (B, 1))
            sc["traj_params"]["u_ub"] = np.tile(ub, (B, 1))
    if path:  # 4 rows from row 2 on: knots 0 and 1 read rows 2 and 3, the others hold the last row
        sc = _ref_path.with_path(sc, _ref_path.random_path(sc, 4, 13), row0=2)
    return sc


def case(oracle, key):
    """-> dict(sc, low, xs, us, pert, S, clamp, three_d, sp), the fields of _policy.case"""
    name, table, path, B, S, T, two, clamp = CASES[key] if isinstance(key, str) else key
    sc = scenario(key)
    low = scenarios.lower(sc)
    assert low.nj == 7 and (not two or low.desc.nmodels >= 3)
    rng = np.random.default_rng(3)
    us = rng.uniform(-1.0, 1.0, (T, B, low.nu))
    if low.dam == _abi.DAM_VSA:
        us[..., low.nu // 2:] = rng.uniform(0.1, 5.0, (T, B, low.nu // 2))
        if clamp:
            us = np.clip(us, *box(7))
    zx, zk = np.zeros((T + 1, low.nx)), np.zeros((T, low.nu, low.nx))
    xs = np.stack([pol.rollout_one(oracle, low, b, zx, us[:, b], zk)["xs"] for b in range(B)], axis=1)
    return dict(sc=sc, low=low, xs=xs, us=us, pert=pol.perturbations(low, S, 17), S=S, clamp=clamp, three_d=False,
                sp=scenarios.solver_params(sc))
