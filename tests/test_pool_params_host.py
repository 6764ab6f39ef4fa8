"""Pool solves with per-problem parameters (aslr_solve_pool_params), host side: the exported symbol and its binding, the
Python-side lowering of the [P, .] arrays, the host-side validation, and -- on the CPU oracle alone -- whether the seeded
draws of tests/_pool_params.py are fit for the GPU tests that use them."""
import ctypes as C
import os

import numpy as np
import pytest

import _pool_params as pp
import _traj_oracle
from aslr_to_amd import _abi, scenarios
from aslr_to_amd.lowering import lower_traj_params, param_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_exported_and_declared():
    assert _abi.POOL_PARAMS_SYMBOLS == ["aslr_solve_pool_params"]
    lib = _abi.load_library()
    f = lib.aslr_solve_pool_params
    assert f.restype is C.c_int and f.argtypes[3] is C.POINTER(_abi.PoolParams)
    assert C.sizeof(_abi.PoolParams) == 5 * C.sizeof(C.c_void_p)
    assert [n for n, _ in _abi.PoolParams._fields_] == ["stiffness", "motor_inertia", "u_lb", "u_ub", "params_dev"]
    header = open(os.path.join(ROOT, "include", "aslr_to_amd_pool_params.h")).read()
    for word in ("aslr_solve_pool_params", "aslr_pool_params_t", "params_dev", '#include "aslr_to_amd.h"'):
        assert word in header, word
    # the base header, its symbol list, the struct indices of aslr_sizeof and the version are what they were
    base = open(os.path.join(ROOT, "include", "aslr_to_amd.h")).read()
    assert "int aslr_solve_pool_params" not in base and "aslr_solve_pool_params" not in _abi.EXPORTED_SYMBOLS
    assert "#define ASLR_ABI_VERSION %d" % _abi.ABI_VERSION in base
    assert lib.aslr_sizeof(6) == C.sizeof(_abi.Pool) and lib.aslr_sizeof(9) < 0


def test_refusals_that_need_no_device():
    """the entry point names itself in what it refuses before it touches a device: a NULL handle with a field given; with
    no field given the call is aslr_solve_pool, which says so"""
    lib = _abi.load_library()
    sp = _abi.default_solver_params(_abi.SOLVER_FDDP)
    pool, par = _abi.Pool(), _abi.PoolParams()
    a = np.ones((3, 2))
    par.motor_inertia = a.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.aslr_solve_pool_params(None, C.byref(sp), C.byref(pool), C.byref(par), 4, 16, None, None) == _abi.E_INVALID
    assert lib.aslr_last_error().decode() == "aslr_solve_pool_params: the problem handle p is NULL"
    for ppar in (None, C.byref(_abi.PoolParams())):
        assert lib.aslr_solve_pool_params(None, C.byref(sp), C.byref(pool), ppar, 4, 16, None, None) == _abi.E_INVALID
        assert lib.aslr_last_error().decode() == "aslr_solve_pool: the problem handle p is NULL"


def _lowered(name, P, B=4, T=5, **fields):
    sc = {"sea": scenarios.two_dof_sea, "vsa": scenarios.two_dof_vsa_boxddp}[name](B=B, T=T, seed=1)
    low = scenarios.lower(sc)
    return low, lower_traj_params(low.desc, low.nj, low.nu, low.nu_user, low.dam, rows=P, **fields)


def test_rows_are_lowered_to_the_table_the_library_builds():
    """[P, .] arrays -> the fields the ABI takes ([P][nj] / [P][nu], C-contiguous) and, by param_table, the row-major
    [2 nj + 2 nu][P] table: K, the reciprocal of B, the box; a field left out repeats the models' constant"""
    P = 7
    rng = np.random.default_rng(0)
    K, Bm = rng.uniform(0.5, 2.0, (P, 2)), rng.uniform(1e-3, 1e-2, (P, 2))
    low, tp = _lowered("sea", P, stiffness=K, motor_inertia=Bm)
    assert set(tp) == {"stiffness", "motor_inertia"} and all(v.shape == (P, 2) and v.flags["C_CONTIGUOUS"] for v in tp.values())
    tab = param_table(low.desc, low.nj, low.nu, low.dam, tp, P)
    assert tab.shape == (8, P) and tab.flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(tab[0:2], K.T)
    np.testing.assert_array_equal(tab[2:4], (1.0 / Bm).T)
    np.testing.assert_array_equal(tab[4:], 0.0)   # (SEA scenario: no limits)
    # one field: the other repeats model 0's constant (K = 1, B = 1e-2 in two_dof_sea)
    low, tp = _lowered("sea", P, motor_inertia=Bm)
    tab = param_table(low.desc, low.nj, low.nu, low.dam, tp, P)
    np.testing.assert_array_equal(tab[0:2], 1.0)
    np.testing.assert_array_equal(tab[2:4], (1.0 / Bm).T)
    # VSA: K rows are zero, bounds given or the models'
    lb = np.tile([-50.0, -60.0, 0.0, 0.002], (P, 1))
    low, tp = _lowered("vsa", P, u_lb=lb)
    tab = param_table(low.desc, low.nj, low.nu, low.dam, tp, P)
    assert tab.shape == (12, P)
    np.testing.assert_array_equal(tab[0:2], 0.0)
    np.testing.assert_array_equal(tab[2:4], 1.0 / 1e-3)
    np.testing.assert_array_equal(tab[4:8], lb.T)
    np.testing.assert_array_equal(tab[8:12], 100.0)
    # no field: nothing to lower (the old call path)
    assert _lowered("sea", P)[1] is None
    # the table of B columns is the shard's own (rows = None keeps the meaning lower_traj_params had)
    low, tp = _lowered("sea", None, motor_inertia=Bm[:4])
    assert tp["motor_inertia"].shape == (4, 2)


def test_one_command_pendulum_bounds_are_padded_per_problem():
    sc = scenarios.double_pendulum_nu1(T=4)
    sc["running"][0].u_lb, sc["running"][0].u_ub = np.array([-5.0]), np.array([5.0])
    low = scenarios.lower(sc)
    assert low.nu == 2 and low.nu_user == 1 and low.B == 1
    tp = lower_traj_params(low.desc, low.nj, low.nu, low.nu_user, low.dam, u_lb=[[-2.0], [-1.5], [-0.5]],
                           u_ub=[[3.0], [2.0], [1.0]], rows=3)
    np.testing.assert_array_equal(tp["u_lb"], [[-2.0, -1.0], [-1.5, -1.0], [-0.5, -1.0]])
    np.testing.assert_array_equal(tp["u_ub"], [[3.0, 1.0], [2.0, 1.0], [1.0, 1.0]])
    tab = param_table(low.desc, low.nj, low.nu, low.dam, tp, 3)
    np.testing.assert_array_equal(tab[4:6], tp["u_lb"].T)
    np.testing.assert_array_equal(tab[6:8], tp["u_ub"].T)


@pytest.mark.parametrize("name, tp, msg", [
    ("sea", dict(stiffness=np.ones((4, 2))), "one row per pool problem"),     # B rows where P = 7 are wanted
    ("sea", dict(stiffness=np.ones((7, 3))), "entries per pool problem"),
    ("sea", dict(stiffness=-np.ones((7, 2))), "stiffness entries"),
    ("sea", dict(motor_inertia=np.zeros((7, 2))), "motor_inertia entries"),
    ("sea", dict(motor_inertia=np.full((7, 2), np.nan)), "motor_inertia entries"),
    ("sea", dict(u_lb=np.zeros((7, 2)), u_ub=np.ones((7, 2))), "no action model of the problem has control limits"),
    ("vsa", dict(stiffness=np.ones((7, 2))), "VSA"),
    ("vsa", dict(u_lb=np.ones((7, 4)), u_ub=np.zeros((7, 4))), "u_lb <= u_ub"),
    ("vsa", dict(u_lb=np.full((7, 4), 200.0)), "u_lb <= u_ub"),
])
def test_validation_errors(name, tp, msg):
    with pytest.raises(ValueError, match=msg):
        _lowered(name, 7, **tp)


def test_draws_are_seeded_and_in_range():
    for name, c in pp.CASES.items():
        a, b = pp.case(name, P=12, T=4), pp.case(name, P=12, T=4)
        sc = a["sc"]
        const = scenarios.constant_traj_params(sc)
        full = pp.draw(sc, c["draw_seed"], inertia_factor=c.get("inertia_factor"))
        for k, v in full.items():
            assert (v is None) == (const[k] is None), (name, k)
            if v is None:
                continue
            f = v / np.where(const[k] == 0.0, 1.0, const[k])
            lo, hi = pp.BOX_FACTOR if k in ("u_lb", "u_ub") else pp.FACTOR
            if k == "motor_inertia" and c.get("inertia_factor"):
                lo, hi = c["inertia_factor"]
                np.testing.assert_array_equal(v, a["params"][k])   # (the case draws with its own range)
            assert (v[const[k] == 0.0] == 0.0).all() and f[const[k] != 0.0].min() >= lo and f[const[k] != 0.0].max() <= hi
        if full["u_lb"] is not None:
            assert (full["u_lb"] <= full["u_ub"]).all()
        assert set(a["params"]) == set(c["fields"])
        for k in a["params"]:
            np.testing.assert_array_equal(a["params"][k], b["params"][k])


@pytest.mark.parametrize("name", sorted(pp.CASES))
def test_the_draws_are_fit_for_the_gpu_test(oracle, name):
    """On the oracle alone (the per-trajectory loop of tests/_traj_oracle.py): each drawn case converges on >= 90 % of its
    problems, and its iteration counts are not all equal -- a comparison of a pool with a batch says little about problems
    that stop at maxiter together.

    What the oracle gives (seeds: scenario / draw): two_dof_sea (6 / 21) 148 of 150, 8 .. 60 iterations; two_dof_vsa_boxddp
    (4 / 22) 198 of 200, 6 .. 400; talos_arm_vsa (3 / 24) 10 of 10, 18 .. 182; talos_arm_sea (9 / 23) 14 of 14, 4 .. 11.
    talos_arm_sea runs at maxiter = 12, and with the ranges of the other cases it cannot meet the share: motor inertia x
    [1/2, 2] around the scenario's 1e-3 gives at best 7 of 14 over scenario seeds 0 .. 59 (left to run, its problems need
    9 .. 100 iterations, median 15 - 17).  As the rule for a failing draw allows, its RANGE was changed, not the conditions:
    motor inertia x [32, 128] (as wide; B in 0.03 .. 0.13), stiffness x [1/2, 2] as before; 25 of the scenario seeds 0 .. 39
    then reach 13 of 14, and seed 9 is the lowest on which all 14 converge."""
    c = pp.case(name)
    ref = _traj_oracle.solve(oracle, scenarios.lower(pp.batch_scenario(c)), c["sp"])
    it, st = ref["traj_i"][_abi.TI_ITER], ref["traj_i"][_abi.TI_STATUS]
    conv = int(((st & _abi.ST_CONVERGED) != 0).sum())
    print("%s: oracle converged on %d of %d, iterations %d .. %d" % (name, conv, c["P"], it.min(), it.max()))
    assert it.min() < it.max()
    assert conv >= 0.9 * c["P"]
