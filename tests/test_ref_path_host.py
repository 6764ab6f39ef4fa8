"""Time-varying reference placements (aslr_set_reference_path), host side: the ABI's self-description, lowering and its
validation, the seeded scenario helpers, and the oracle-only conditions by which the full-solve cases of
tests/test_gpu_ref_path.py were chosen."""
import ctypes as C
import os

import numpy as np
import pytest

import _ref_path as RP
from aslr_to_amd import _abi, crocoddyl, scenarios
from aslr_to_amd.lowering import lower_reference_path, shard_rows
from aslr_to_amd.pinocchio import SE3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_python_and_library_agree_on_version_5():
    header = open(os.path.join(ROOT, "include", "aslr_to_amd.h")).read()
    assert _abi.ABI_VERSION == 5
    assert "#define ASLR_ABI_VERSION 5" in header
    for word in ("int aslr_set_reference_path(aslr_problem_t *p, const double *path, int32_t n_rows, int32_t row0, void *stream);",
                 "int aslr_reference_row(const aslr_problem_t *p, int32_t *row0);"):
        assert word in header, word
    assert "needs per-knot references" not in header
    lib = _abi.load_library()
    assert lib.aslr_abi_version() == 5


def test_both_symbols_are_exported():
    lib = _abi.load_library()
    for sym in ("aslr_set_reference_path", "aslr_reference_row"):
        assert sym in _abi.EXPORTED_SYMBOLS
        assert hasattr(lib, sym)
    # callable without a GPU and without a handle: NULL is declined, not dereferenced
    assert lib.aslr_set_reference_path(None, None, 1, 0, None) == _abi.E_INVALID
    assert lib.aslr_reference_row(None, None) == _abi.E_INVALID
    # the workspace does not grow with the feature: the path is the caller's buffer (sizes pinned for version 4 by
    # tests/test_traj_params_host.py, which still passes)
    assert lib.aslr_sizeof(8) == C.sizeof(_abi.Mpc) and lib.aslr_sizeof(9) == -1


def _sea(B=6, T=5):
    return scenarios.two_dof_sea(B=B, T=T, seed=1)


def test_lowering_uploads_time_major():
    sc = _sea()
    path = RP.random_path(sc, 4, seed=2)
    low = scenarios.lower(RP.with_path(sc, path, row0=3))
    tm, row0 = low.ref_path
    assert row0 == 3 and tm.shape == (4, 6, 12) and tm.flags["C_CONTIGUOUS"] and tm.dtype == np.float64
    np.testing.assert_array_equal(tm, path.transpose(1, 0, 2))
    assert scenarios.lower(sc).ref_path is None
    # nested lists of SE3
    se3 = [[SE3(path[b, i, :9].reshape(3, 3), path[b, i, 9:]) for i in range(4)] for b in range(6)]
    np.testing.assert_array_equal(lower_reference_path(low.desc, se3), tm)


def test_paths_are_sliced_by_rank_like_frame_refs():
    sc = _sea(B=7)
    path = RP.random_path(sc, 3, seed=2)
    for rank in range(3):
        p = crocoddyl.ShootingProblem(sc["x0"], sc["running"], sc["terminal"], frame_refs=sc["frame_refs"], rank=rank,
                                      world_size=3, frame_ref_path=path)
        lo, hi = shard_rows(7, rank, 3)
        np.testing.assert_array_equal(p.lowered.ref_path[0], path[lo:hi].transpose(1, 0, 2))
        assert p.reference_row == 0
        p.set_reference_path(path, row0=2)
        assert p.reference_row == 2 and p.lowered.ref_path[1] == 2
        p.set_reference_path(None)
        assert p.lowered.ref_path is None and p.reference_row == 0


@pytest.mark.parametrize("make_path, row0, msg", [
    (lambda p: p[:5], 0, r"shape \[B=6, n_rows, 12\]"),
    (lambda p: p[:, :, :11], 0, r"shape \[B=6, n_rows, 12\]"),
    (lambda p: p[0], 0, r"shape \[B=6, n_rows, 12\]"),
    (lambda p: p[:, :0], 0, "n_rows must be >= 1"),
    (lambda p: np.where(np.arange(12) == 10, np.nan, p), 0, "entries must be finite"),
    (lambda p: np.where(np.arange(12) == 0, np.inf, p), 0, "entries must be finite"),
    (lambda p: p, 4, r"row0 must lie in \[0, n_rows\)"),
    (lambda p: p, -1, r"row0 must lie in \[0, n_rows\)"),
])
def test_lowering_rejects(make_path, row0, msg):
    sc = _sea()
    path = RP.random_path(sc, 4, seed=2)
    with pytest.raises(ValueError, match=msg):
        scenarios.lower(RP.with_path(sc, make_path(path), row0))
    with pytest.raises(ValueError, match=msg):
        crocoddyl.ShootingProblem(sc["x0"], sc["running"], sc["terminal"], frame_refs=sc["frame_refs"]).set_reference_path(make_path(path), row0)


def test_lowering_rejects_a_problem_without_a_frame_placement_cost():
    sc = scenarios.double_pendulum(T=4)
    path = np.tile(np.concatenate([np.eye(3).reshape(9), np.zeros(3)]), (1, 3, 1))
    with pytest.raises(ValueError, match="no model of the problem has a frame-placement cost"):
        crocoddyl.ShootingProblem(sc["x0"], sc["running"], sc["terminal"], frame_ref_path=path)


def test_the_product_path_raises_without_a_gpu():
    import torch
    sc = _sea()
    p = crocoddyl.ShootingProblem(sc["x0"], sc["running"], sc["terminal"], frame_refs=sc["frame_refs"],
                                  frame_ref_path=RP.random_path(sc, 4, seed=2))
    if torch.cuda.is_available():   # (where there is one, the same line runs: tests/test_gpu_ref_path.py holds it to the oracle)
        assert p.engine.reference_row == 0
        return
    with pytest.raises(_abi.AslrError):
        p.engine


def test_seeded_helpers():
    sc = scenarios.two_dof_sea(B=5, T=9, seed=5)
    via = scenarios.reference_via_points(sc, seed=11)
    refs = np.asarray(sc["frame_refs"])
    assert via.shape == (5, 4, 12)
    np.testing.assert_array_equal(via, scenarios.reference_via_points(sc, seed=11))
    np.testing.assert_array_equal(via[:, :, :9], np.repeat(refs[:, None, :9], 4, axis=1))
    np.testing.assert_array_equal(via[:, :, 11], np.repeat(refs[:, None, 11], 4, axis=1))
    off = via[:, :, 9:11] - refs[:, None, 9:11] - (np.arange(4)[None, :, None] - 3) * np.array([0.01, -0.008])
    assert np.abs(off).max() <= 0.004 + 1e-15 and np.abs(off).max() > 0.002
    path = scenarios.hold_via_points(via, 9)
    assert path.shape == (5, 10, 12)
    for t, i in enumerate([0, 0, 0, 1, 1, 1, 2, 2, 2, 3]):
        np.testing.assert_array_equal(path[:, t], via[:, i])


def test_four_model_problem_is_the_sweep_over_the_held_path(oracle):
    """Pins the harness: the oracle's batched calc_diff of the four-model problem equals, bit for bit, the per-knot sweep
    (oracle.knot with the knot's row) over the path that holds the same via-points."""
    sc = scenarios.two_dof_vsa_boxddp(B=3, T=7, seed=5)
    low = scenarios.lower(sc)
    via = scenarios.reference_via_points(sc, seed=11)
    rng = np.random.default_rng(0)
    xs, us = rng.uniform(-0.5, 0.5, (8, 3, 8)), rng.uniform(0.1, 1.0, (7, 3, 4))
    path_tm = scenarios.hold_via_points(via, 7).transpose(1, 0, 2)
    got = RP.sweep(oracle, low, xs, us, path_tm, 0)
    for b in range(3):
        ref = oracle.calc_diff(RP.four_models(low, via[b], [b]), xs[:, b:b + 1], us[:, b:b + 1])
        for g, r in zip(got, ref):
            np.testing.assert_array_equal(g[:, b:b + 1], r)
    # ... and the path is seen: the create-time references give other costs
    assert np.abs(oracle.calc_diff(low, xs, us)[1] - got[1]).max() > 1e-6


@pytest.mark.parametrize("name", sorted(RP.FULL_SOLVE_CASES))
def test_oracle_is_stable_on_the_full_solve_cases(oracle, name):
    """The conditions by which the full-solve cases of tests/test_gpu_ref_path.py were chosen, on the oracle alone: at least
    90 % of the trajectories converge, and scaling x0 by (1 + 1e-14) moves no iteration count and the converged xs by less
    than the 1e-6 the GPU is held to."""
    sc, via, sp = RP.full_solve_case(name)
    ref = RP.solve(oracle, scenarios.lower(sc), via, sp)
    sc2 = dict(sc)
    sc2["x0"] = sc["x0"] * (1.0 + 1e-14)
    per = RP.solve(oracle, scenarios.lower(sc2), via, sp)
    conv = (ref["traj_i"][_abi.TI_STATUS] & _abi.ST_CONVERGED) != 0
    it = ref["traj_i"][_abi.TI_ITER]
    dx = np.abs(per["xs"] - ref["xs"]).max(axis=(0, 2))[conv].max()
    print("%s: %d of %d converge, iterations %d..%d, counts changed %d, xs move by %.1e"
          % (name, conv.sum(), conv.size, it.min(), it.max(), int((per["traj_i"][_abi.TI_ITER] != it).sum()), dx))
    assert conv.sum() >= 0.9 * conv.size
    np.testing.assert_array_equal(per["traj_i"][_abi.TI_ITER], it)
    assert dx < 1e-6
