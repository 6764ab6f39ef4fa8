"""The 7-joint arm with variable-stiffness actuation (nx = 28, nu = 14) solved with SolverBoxDDP: what can be checked
without a GPU.

* the `talos_arm_vsa` scenario lowers to the sizes and bounds the solver kernels are built for, and the CPU oracle
  converges on the whole seeded batch;
* the wave-cooperative gains / box QP of the backward kernel (aslr_to_amd/csrc/aslr_wave_gains.hpp) is compiled for the
  host (tests/host/wave_gains_emul.cpp: the same template source, the 64 lanes one after the other) and compared with
  the oracle's BoxQP (oracle/aslr_oracle.c, aslr_cpu_boxqp) on random SPD 14 x 14 problems with mixed active sets and
  warm starts: same clamped set, same iteration count, solution and Hff_inv-derived gains to 1e-12 relative.  The
  bound: both sides run the same operations in the same order in IEEE double except the pivots (1 / sqrt(d) times the
  entry here, the entry divided by sqrt(d) there: one more rounding per factor entry), so they differ by a few ulp
  (2.2e-16) amplified by the conditioning of the free block; the problems are built with cond(H) < ~1e2.
The GPU instantiation is checked by tests/test_gpu_vsa7.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from aslr_to_amd import _abi, scenarios

HERE = os.path.dirname(os.path.abspath(__file__))
NU, NX = 14, 28


def test_talos_arm_vsa_scenario_lowers_to_nu_14_and_the_oracle_converges_on_the_batch(oracle):
    sc = scenarios.SCENARIOS["talos_arm_vsa"](B=64, T=50, seed=3)
    low = scenarios.lower(sc)
    assert (low.nx, low.nu) == (28, 14)
    m = low.desc.models[0]
    assert m.dam == _abi.DAM_VSA and m.nu == 14 and m.has_u_limits
    np.testing.assert_array_equal(np.array(m.u_lb[:14]), [-100.0] * 7 + [1.0] * 7)
    np.testing.assert_array_equal(np.array(m.u_ub[:14]), [100.0] * 7 + [50.0] * 7)
    assert sc["solver"] == "SolverBoxDDP" and sc["maxiter"] == 300 and sc["th_stop"] == 1e-7
    sp = scenarios.solver_params(sc)
    ref = oracle.solve(low, sp)
    status, iters = ref["traj_i"][_abi.TI_STATUS], ref["traj_i"][_abi.TI_ITER]
    assert (status == _abi.ST_CONVERGED).all(), status
    assert iters.min() >= 2 and iters.max() < 300
    on_floor = (ref["us"][..., 7:] == 1.0).mean()
    assert 0.5 < on_floor < 1.0  # the stiffness half of the box is what the solver works against


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emul") / "libwave_gains_emul.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-shared",
                           "-fPIC", "-o", so, os.path.join(HERE, "host", "wave_gains_emul.cpp")])
    lib = C.CDLL(so)
    d, i = C.POINTER(C.c_double), C.POINTER(C.c_int)
    lib.emul_wave_gains.argtypes = [C.c_int, C.c_int, d, d, d, d, d, d, C.c_int, C.c_double, C.c_double, C.c_double,
                                    d, d, d, d, i]
    lib.emul_wave_gains.restype = C.c_int

    def run(box, boxed, H, q, lb, ub, k0, Qux, maxiter=100, th_acc=0.1, th_grad=1e-5, reg=0.0):
        H, q, lb, ub, k0, Qux = (np.ascontiguousarray(a, dtype=np.float64) for a in (H, q, lb, ub, k0, Qux))
        k, qz, K, mask = np.zeros(NU), np.zeros(NU), np.zeros((NU, NX)), np.zeros(NU)
        it = C.c_int(0)
        p = lambda a: a.ctypes.data_as(d)
        bad = lib.emul_wave_gains(box, int(boxed), p(H), p(q), p(lb), p(ub), p(k0), p(Qux), maxiter, th_acc, th_grad,
                                  reg, p(k), p(qz), p(K), p(mask), C.byref(it))
        return k, qz, K, mask, it.value, bad
    return run


def _problem(rng, scale):
    Q, _ = np.linalg.qr(rng.normal(size=(NU, NU)))
    H = (Q * rng.uniform(0.5, 20.0, NU)).dot(Q.T)
    H = 0.5 * (H + H.T)
    q = scale * rng.normal(size=NU)
    lb = -np.abs(rng.normal(size=NU)) * rng.choice([0.05, 0.5, 5.0], size=NU)
    ub = np.abs(rng.normal(size=NU)) * rng.choice([0.05, 0.5, 5.0], size=NU)
    k0 = rng.normal(size=NU) * rng.choice([0.0, 0.3, 3.0])
    return H, q, lb, ub, k0, rng.normal(size=(NU, NX))


def test_emulated_wave_reproduces_the_oracle_boxqp(oracle, emul):
    rng = np.random.default_rng(14)
    iters_seen = np.zeros(8, dtype=int)
    clamped_counts = []
    for trial in range(400):
        H, q, lb, ub, k0, Qux = _problem(rng, rng.choice([0.01, 1.0, 10.0, 300.0]))
        reg = 0.0 if trial % 5 else 1e-9
        k, qz, K, mask, it, bad = emul(1, True, H, q, lb, ub, k0, Qux, reg=reg)
        assert not bad
        r = oracle.boxqp(H, q, lb, ub, k0, maxiter=100, th_acceptstep=0.1, th_grad=1e-5, reg=reg)
        free = np.zeros(NU, dtype=bool)
        free[r["free"]] = True
        np.testing.assert_array_equal(mask == 1.0, free)
        assert it == r["iters"]
        Qinv = np.zeros((NU, NU))
        if free.any():
            Qinv[np.ix_(r["free"], r["free"])] = r["Hff_inv"]
        eK = Qinv.dot(Qux)
        np.testing.assert_allclose(k, -r["x"], rtol=0, atol=1e-12 * (1.0 + np.abs(r["x"]).max()))
        np.testing.assert_allclose(K, eK, rtol=0, atol=1e-12 * (1.0 + np.abs(eK).max()))
        eqz = q.copy()
        eqz[r["clamped"]] = 0.0
        np.testing.assert_array_equal(qz, eqz)
        iters_seen[min(it, 7)] += 1
        clamped_counts.append(NU - free.sum())
    clamped_counts = np.array(clamped_counts)
    # the cases must cover every outcome: nothing, some and everything clamped; one, two, three and more iterations
    assert (clamped_counts == 0).sum() > 5 and (clamped_counts == NU).sum() > 5
    assert ((clamped_counts > 0) & (clamped_counts < NU)).sum() > 200
    assert iters_seen[1] > 20 and iters_seen[2] > 50 and iters_seen[3:].sum() > 50


def test_emulated_wave_plain_gains_and_indefinite_quu(emul):
    rng = np.random.default_rng(15)
    for box in (0, 1):  # (box = 1 with a node that is not boxed: SolverBoxDDP while the trajectory is infeasible)
        for _ in range(40):
            H, q, lb, ub, k0, Qux = _problem(rng, 1.0)
            k, qz, K, mask, it, bad = emul(box, False, H, q, lb, ub, k0, Qux)
            assert not bad and it == -1
            np.testing.assert_allclose(k, np.linalg.solve(H, q), rtol=0, atol=1e-12 * (1.0 + np.abs(k).max()))
            eK = np.linalg.solve(H, Qux)
            np.testing.assert_allclose(K, eK, rtol=0, atol=1e-12 * (1.0 + np.abs(eK).max()))
            np.testing.assert_array_equal(qz, q)
    H, q, lb, ub, k0, Qux = _problem(rng, 1.0)
    assert emul(0, False, -H, q, lb, ub, k0, Qux)[5] == 1
    assert emul(1, True, -H, q, 10 * lb - 1, 10 * ub + 1, 0 * k0, Qux)[5] == 1


def test_emulated_wave_on_qp_instances_of_a_real_solve(oracle, emul):
    """Quu / Qu / bounds / warm starts logged by the oracle during BoxDDP iterations of the test variant of the scenario
    whose torque bounds are active as well."""
    sc = scenarios.talos_arm_vsa(B=2, T=30, seed=3, tight=True)
    low = scenarios.lower(sc)
    sp = scenarios.solver_params(sc, maxiter=25)
    L = oracle.lib()
    cap = 2_000_000
    buf = np.zeros(cap)
    L.aslr_cpu_boxqp_dump(buf.ctypes.data_as(C.POINTER(C.c_double)), C.c_long(cap))
    try:
        oracle.solve(low, sp)
        n = L.aslr_cpu_boxqp_dump_len()
    finally:
        L.aslr_cpu_boxqp_dump(None, C.c_long(0))
    rec = NU * NU + 5 * NU + 1
    inst = buf[:n].reshape(-1, rec)
    assert len(inst) > 500
    multi = 0
    for blk in inst[:: max(1, len(inst) // 600)]:
        o = NU * NU
        H, q, lb, ub, x0, xs = blk[:o], blk[o:o + NU], blk[o + NU:o + 2 * NU], blk[o + 2 * NU:o + 3 * NU], \
            blk[o + 3 * NU:o + 4 * NU], blk[o + 4 * NU:o + 5 * NU]
        k, qz, K, mask, it, bad = emul(1, True, H, q, lb, ub, x0, np.zeros((NU, NX)))
        assert not bad
        assert it == int(blk[-1])
        np.testing.assert_allclose(k, -xs, rtol=0, atol=1e-9 * (1.0 + np.abs(xs).max()))
        multi += int(blk[-1] >= 2)
    assert multi > 20
