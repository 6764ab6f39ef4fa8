"""Per-trajectory parameter table (stiffness, motor inertia, control box), host side: lowering, validation, the ABI's
self-description, and the per-trajectory oracle loop the GPU tests compare against (tests/_traj_oracle.py)."""
import ctypes as C

import numpy as np
import pytest

import _traj_oracle
from aslr_to_amd import _abi, crocoddyl, scenarios
from aslr_to_amd.lowering import lower_problem, shard_rows


def _sea(B=6, T=5):
    return scenarios.two_dof_sea(B=B, T=T, seed=1)


def _vsa(B=6, T=5):
    return scenarios.two_dof_vsa_boxddp(B=B, T=T, seed=1)


def _lower(sc, **tp):
    return lower_problem(sc["x0"], sc["running"], sc["terminal"], sc["frame_refs"], **tp)


def test_lowering_round_trips_the_arrays():
    sc = scenarios.with_traj_params(_sea(), seed=3)
    low = scenarios.lower(sc)
    for k in ("stiffness", "motor_inertia"):
        np.testing.assert_array_equal(low.traj_params[k], sc["traj_params"][k])
        assert low.traj_params[k].flags["C_CONTIGUOUS"] and low.traj_params[k].shape == (6, 2)
    assert set(low.traj_params) == {"stiffness", "motor_inertia"}
    assert scenarios.lower(_sea()).traj_params is None
    v = scenarios.with_traj_params(_vsa(), seed=3, stiffness_floors=(0.0, 0.002))
    lv = scenarios.lower(v)
    assert set(lv.traj_params) == {"motor_inertia", "u_lb", "u_ub"}
    np.testing.assert_array_equal(lv.traj_params["u_lb"][:3, 2:], 0.0)
    np.testing.assert_array_equal(lv.traj_params["u_lb"][3:, 2:], 0.002)


def test_arrays_are_sliced_by_rank_like_frame_refs():
    sc = scenarios.with_traj_params(_sea(B=7), seed=2)
    tp = sc["traj_params"]
    for rank in range(3):
        p = crocoddyl.ShootingProblem(sc["x0"], sc["running"], sc["terminal"], frame_refs=sc["frame_refs"], rank=rank,
                                      world_size=3, stiffness=tp["stiffness"], motor_inertia=tp["motor_inertia"])
        lo, hi = shard_rows(7, rank, 3)
        np.testing.assert_array_equal(p.lowered.traj_params["stiffness"], tp["stiffness"][lo:hi])
        np.testing.assert_array_equal(p.lowered.traj_params["motor_inertia"], tp["motor_inertia"][lo:hi])
        np.testing.assert_array_equal(p.lowered.frame_ref, np.asarray(sc["frame_refs"])[lo:hi])


def test_one_command_pendulum_bounds_are_padded():
    sc = scenarios.double_pendulum_nu1(T=4)
    sc["running"][0].u_lb, sc["running"][0].u_ub = np.array([-5.0]), np.array([5.0])
    low = _lower(sc, u_lb=[[-2.0]], u_ub=[[3.0]])
    assert low.nu == 2 and low.nu_user == 1
    np.testing.assert_array_equal(low.traj_params["u_lb"], [[-2.0, -1.0]])
    np.testing.assert_array_equal(low.traj_params["u_ub"], [[3.0, 1.0]])


@pytest.mark.parametrize("make, tp, msg", [
    (_sea, dict(stiffness=np.ones((5, 2))), "one row per trajectory"),
    (_sea, dict(stiffness=np.ones((6, 3))), "entries per trajectory"),
    (_sea, dict(motor_inertia=np.ones((6, 4))), "entries per trajectory"),
    (_sea, dict(stiffness=-np.ones((6, 2))), "stiffness entries"),
    (_sea, dict(stiffness=np.full((6, 2), np.nan)), "stiffness entries"),
    (_sea, dict(motor_inertia=np.zeros((6, 2))), "motor_inertia entries"),
    (_sea, dict(motor_inertia=np.full((6, 2), np.inf)), "motor_inertia entries"),
    (_sea, dict(u_lb=np.zeros((6, 2)), u_ub=np.ones((6, 2))), "no action model of the problem has control limits"),
    (_vsa, dict(stiffness=np.ones((6, 2))), "VSA"),
    (_vsa, dict(u_lb=np.ones((6, 4)), u_ub=np.zeros((6, 4))), "u_lb <= u_ub"),
    (_vsa, dict(u_lb=np.full((6, 4), 200.0)), "u_lb <= u_ub"),
    (_vsa, dict(u_ub=np.ones((6, 3))), "entries per trajectory"),
])
def test_validation_errors(make, tp, msg):
    with pytest.raises(ValueError, match=msg):
        _lower(make(), **tp)


def test_non_diagonal_model_matrices_are_rejected():
    sc = _sea()
    d = sc["running"][0].differential
    for name in ("K", "B"):
        attr = [a for a in ("K", "B", "_K", "_B") if hasattr(d, a) and a.lstrip("_") == name][0]
        old = np.array(getattr(d, attr), dtype=float)
        bad = old.copy()
        bad[0, 1] = bad[1, 0] = 1e-3
        setattr(d, attr, bad)
        try:
            with pytest.raises(ValueError, match="diagonal"):
                _lower(sc, motor_inertia=np.ones((6, 2)))
        finally:
            setattr(d, attr, old)


def test_symbol_sizeof_and_region_are_declared():
    assert "aslr_set_trajectory_params" in _abi.EXPORTED_SYMBOLS
    assert _abi.R_TRAJ_PARAMS == _abi.R_COUNT - 1
    assert C.sizeof(_abi.TrajParams) == 4 * C.sizeof(C.c_void_p)
    header = open(__file__.rsplit("/tests/", 1)[0] + "/include/aslr_to_amd.h").read()
    for word in ("aslr_set_trajectory_params", "ASLR_R_TRAJ_PARAMS", "aslr_traj_params_t", "7 traj_params"):
        assert word in header, word
    assert "#define ASLR_ABI_VERSION %d" % _abi.ABI_VERSION in header


def _regions_without_desc(low, with_table):
    """sum of the 256-byte aligned sizes of every workspace region but DESC (include/aslr_to_amd.h: the shapes under
    'Named regions'), with or without TRAJ_PARAMS"""
    B, T, nx, nu, nj, rec = low.B, low.T, low.nx, low.nu, low.nj, low.rec
    T1, D = T + 1, 8
    slab = lambda w: ((B + 3) // 4) * 4 * w if (w % 2 == 0 and w <= 8) else B * w
    dyn = ((2 * nj + nj * nj + 1) // 2 * 2 + nj * ((3 * nj + 1) // 2 * 2)) if nj > 2 else 0
    sizes = [T1 * B * nx * D, T * B * nu * D, T1 * B * nx * D, T1 * B * D, T1 * B * rec * D, T1 * B * nx * D,
             T * B * nu * nx * D, T * B * nu * D, T * B * nu * D, T1 * B * nx * D, T1 * B * nx * nx * D,
             _abi.NALPHA * T1 * slab(nx) * D, _abi.NALPHA * T * slab(nu) * D, _abi.TF_COUNT * B * D, _abi.TI_COUNT * B * 4,
             B * nx * D, B * 12 * D, T1 * B * nx * D, T1 * 4, _abi.NALPHA * T1 * B * D, T1 * B * dyn * D,
             B * (nx + 12) * D]
    assert len(sizes) == _abi.R_COUNT - 2  # all but DESC and TRAJ_PARAMS
    if with_table:
        sizes.append((2 * nj + 2 * nu) * B * D)
    return sum((v + 255) // 256 * 256 for v in sizes)


def test_library_exports_the_entry_point_and_sizes_the_region():
    """aslr_sizeof(7), and aslr_workspace_bytes grown by exactly the table: the total minus every other region (computed
    here from the documented shapes) leaves the DESC region, one size for every problem; without the table's
    (2 nj + 2 nu) B doubles in the sum the remainder would change with B and nu.  No GPU needed."""
    lib = _abi.load_library()
    assert hasattr(lib, "aslr_set_trajectory_params")
    assert lib.aslr_sizeof(7) == C.sizeof(_abi.TrajParams)
    rest, rest_no_table = set(), set()
    for sc in (_sea(B=100), _sea(B=37), _vsa(B=100), _vsa(B=4096, T=100), scenarios.talos_arm_vsa(B=3, T=4),
               scenarios.talos_arm_sea(B=130, T=7)):
        low = scenarios.lower(sc)
        total = lib.aslr_workspace_bytes(C.byref(low.desc))
        rest.add(total - _regions_without_desc(low, True))
        rest_no_table.add(total - _regions_without_desc(low, False))
    assert len(rest) == 1, rest           # = the aligned size of the device description
    desc_bytes = rest.pop()
    assert desc_bytes % 256 == 0 and 0 < desc_bytes - C.sizeof(_abi.Chain) - _abi.MAX_MODELS * C.sizeof(_abi.Model) < 8192
    assert len(rest_no_table) > 1         # (the harness: leaving the table out is noticed)


@pytest.mark.parametrize("make", [_sea, _vsa])
def test_oracle_loop_with_the_constants_is_the_batched_oracle(oracle, make):
    """Pins the harness: every row of the table equal to the models' constants -> the per-trajectory loop returns what
    the plain batched oracle returns, bit for bit (same code on the same numbers)."""
    sc = make(B=4, T=8)
    plain = scenarios.lower(sc)
    sc2 = dict(sc)
    sc2["traj_params"] = scenarios.constant_traj_params(sc)
    low = scenarios.lower(sc2)
    rng = np.random.default_rng(0)
    xs = rng.uniform(-0.5, 0.5, (low.T + 1, low.B, low.nx))
    us = rng.uniform(0.1, 1.0, (low.T, low.B, low.nu))
    for a, b in zip(_traj_oracle.calc_diff(oracle, low, xs, us), oracle.calc_diff(plain, xs, us)):
        np.testing.assert_array_equal(a, b)
    sp = scenarios.solver_params(sc, maxiter=15)
    ref, got = oracle.solve(plain, sp), _traj_oracle.solve(oracle, low, sp)
    for k in ("xs", "us", "traj_f", "traj_i"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)


def test_oracle_loop_sees_the_table(oracle):
    sc = scenarios.with_traj_params(_sea(B=3, T=6), seed=5)
    low, plain = scenarios.lower(sc), scenarios.lower(_sea(B=3, T=6))
    rng = np.random.default_rng(1)
    xs, us = rng.uniform(-0.5, 0.5, (7, 3, 8)), rng.uniform(-1, 1, (6, 3, 2))
    a, b = _traj_oracle.calc_diff(oracle, low, xs, us)[0], oracle.calc_diff(plain, xs, us)[0]
    assert np.abs(a - b).max() > 1e-6


@pytest.mark.parametrize("scen", ["two_dof_vsa_boxddp", "talos_arm_sea"])
def test_oracle_is_stable_on_the_full_solve_cases(oracle, scen):
    """The criterion by which the full-solve cases of tests/test_gpu_traj_params.py were chosen, on the oracle alone: it
    converges on >= 90 % of the batch, and a 1e-14 relative perturbation of x0 moves none of its iteration counts and
    its converged xs by far less than the 1e-6 the GPU is held to (the two-joint SEA case converges in few iterations and is
    left out for time)."""
    import test_gpu_traj_params as G
    sc, sp = G.full_solve_case(scen)
    ref = _traj_oracle.solve(oracle, scenarios.lower(sc), sp)
    sc2 = dict(sc)
    sc2["x0"] = sc["x0"] * (1.0 + 1e-14)
    per = _traj_oracle.solve(oracle, scenarios.lower(sc2), sp)
    conv = (ref["traj_i"][_abi.TI_STATUS] & _abi.ST_CONVERGED) != 0
    assert conv.sum() >= 0.9 * conv.size
    np.testing.assert_array_equal(per["traj_i"][_abi.TI_ITER], ref["traj_i"][_abi.TI_ITER])
    dx = np.abs(per["xs"] - ref["xs"]).max(axis=(0, 2))[conv].max()
    print("%s: %d of %d converge, xs move by %.1e" % (scen, conv.sum(), conv.size, dx))
    assert dx < 1e-8
