"""The shorter input forms of the Engine's extension calls, and what they refuse: a scalar, [n] or [nj] where [B, ...] is the
full form must give the bits of the spelled-out array, and a malformed input the ValueError text written here (copied from
the source as it stood before the lowering helpers of engine.py were shared, not from the code under test).

B = 3, T = 4: no multiples of 4 or 16, so padded lanes take part.  Pinned elsewhere and not repeated: sigma0 [nx, nx] and
noise_var [nx] / [B, nx] (test_gpu_covariance.test_python_facade), the variances as [nj] (test_gpu_plant_sens.test_python_facade),
the sigmas as a scalar, [n] and [B, n] (test_gpu_policy_noise.test_python_facade)."""
import numpy as np
import pytest

import _design as D
import _ext_call as ext
import _gpu_case as gc
from aslr_to_amd import scenarios

pytestmark = pytest.mark.gpu

B, T = 3, 4


def _solved(name="two_dof_sea"):
    """a fresh engine after three iterations from the empty candidate (a plan in XS / US, gains in KGAIN) -> engine, sp, low"""
    sc = scenarios.SCENARIOS[name](B=B, T=T, seed=4)
    low = scenarios.lower(sc)
    sp = scenarios.solver_params(sc, maxiter=3)
    e = ext.fresh(low)
    e.solve(sp, poll_every=4)
    gc.sync()
    return e, sp, low


def _same_result(a, b, what):
    assert sorted(a.__dict__) == sorted(b.__dict__), what
    for k, v in a.__dict__.items():
        w = b.__dict__[k]
        if v is None or w is None:
            assert v is None and w is None, "%s: %s is None on one side only" % (what, k)
        else:
            gc.same_bits(v, w, "%s: %s" % (what, k))


def _refused(text, call, *args, **kw):
    with pytest.raises(ValueError) as err:
        call(*args, **kw)
    assert str(err.value) == text


def test_bounds_as_a_scalar_and_as_nj():
    """design_descent and plant_identify: (scalar, scalar) and ([nj], [nj]) bounds against the same bounds as [B, nj]; every
    run on an engine of its own, since both calls leave the parameter table on their result"""
    nj = 2
    # [2 nj, B], the models' constants: the same for every trajectory
    th = D.theta0_of(scenarios.lower(scenarios.SCENARIOS["two_dof_sea"](B=B, T=T, seed=4)))
    assert (th == th[:, :1]).all() and (th[:nj] > 1e-3).all() and (th[:nj] < 1e6).all() and (th[nj:] > 1e-6).all() and (th[nj:] < 1e3).all()
    klo, khi, blo, bhi = th[:nj, 0] / 2, th[:nj, 0] * 2, th[nj:, 0] / 2, th[nj:, 0] * 2
    tile = lambda v: np.tile(v, (B, 1))
    full = lambda v: np.full((B, nj), v)
    forms = {"[nj]": (((klo, khi), (blo, bhi)), ((tile(klo), tile(khi)), (tile(blo), tile(bhi)))),
             "scalar": (((1e-3, 1e6), (1e-6, 1e3)), ((full(1e-3), full(1e6)), (full(1e-6), full(1e3))))}
    for what, (short, spelled) in forms.items():
        got = []
        for kb, bb in (short, spelled):
            e, sp, _ = _solved()
            got.append(e.design_descent(sp, 2, 3, 2, stiffness_bounds=kb, motor_inertia_bounds=bb, keep_history=True))
        _same_result(got[0], got[1], "design_descent, bounds as " + what)
        got = []
        for kb, bb in (short, spelled):
            e, sp, _ = _solved()
            got.append(e.plant_identify(2, stiffness_bounds=kb, motor_inertia_bounds=bb, keep_history=True))
        _same_result(got[0], got[1], "plant_identify, bounds as " + what)
    # one field only: the other is rows of ones for the descent, left out for the fit
    e, sp, _ = _solved()
    one = e.design_descent(sp, 2, 3, 2, motor_inertia_bounds=(1e-6, 1e3))
    assert tuple(one.stiffness.shape) == (B, nj) and not hasattr(one, "cost_history")
    e, sp, _ = _solved()
    lean = e.plant_identify(2, motor_inertia_bounds=(1e-6, 1e3))
    assert tuple(lean.theta.shape) == (B, nj) and not hasattr(lean, "sse_history")


def test_weights_as_nx():
    w = np.random.default_rng(3).uniform(0.5, 2.0, 8)
    got = []
    for weights in (w, np.tile(w, (B, 1))):
        e, sp, _ = _solved()
        got.append(e.plant_identify(2, weights=weights, stiffness_bounds=(1e-3, 1e6), motor_inertia_bounds=(1e-6, 1e3)))
    _same_result(got[0], got[1], "plant_identify, weights as [nx]")


def test_malformed_inputs_are_refused_in_the_words_they_always_were():
    e, sp, _ = _solved()
    ones = np.ones
    _refused("sigma0 must have shape [B=3, nx=8, nx] or [nx, nx], not [3, 7, 7]", e.policy_covariance, sigma0=np.eye(7))
    _refused("sigma0 must have shape [B=3, nx=8, nx] or [nx, nx], not [8]", e.policy_covariance, sigma0=ones(8))
    _refused("sigma0 must be symmetric", e.policy_covariance, sigma0=np.triu(ones((8, 8))))
    _refused("sigma0 has a negative variance on its diagonal", e.policy_covariance, sigma0=-np.eye(8))
    _refused("noise_var must have shape [B=3, T=4, nx=8], [B, nx] or [nx], not [3, 4, 7]", e.policy_covariance, noise_var=ones(7))
    _refused("noise_var must have shape [B=3, T=4, nx=8], [B, nx] or [nx], not [2, 4, 8]", e.policy_covariance, noise_var=ones((2, 8)))
    _refused("noise_var must have shape [B=3, T=4, nx=8], [B, nx] or [nx], not [3, 5, 8]", e.policy_covariance, noise_var=ones((3, 5, 8)))
    _refused("noise_var has a negative variance", e.policy_covariance, noise_var=-ones(8))
    _refused("stiffness_var must have shape [B=3, nj=2] or [nj], not [3, 3]", e.policy_plant_sensitivity, stiffness_var=ones(3))
    _refused("motor_inertia_var must have shape [B=3, nj=2] or [nj], not [2, 2]", e.policy_plant_sensitivity, motor_inertia_var=ones((2, 2)))
    _refused("motor_inertia_var has a negative variance", e.policy_plant_sensitivity, motor_inertia_var=-ones(2))
    _refused("noise_std must be a scalar or have shape [8] or [3, 8], not [3]", e.policy_rollout_noise, 2, 1, noise_std=ones(3))
    _refused("stiffness_rel_std must be a scalar or have shape [2] or [3, 2], not [2, 2]", e.policy_rollout_noise, 2, 1,
             stiffness_rel_std=ones((2, 2)))
    _refused("dx0_std must be a scalar or have shape [8] or [3, 8], not [1, 3, 8]", e.policy_rollout_noise, 2, 1, dx0_std=ones((1, 3, 8)))
    _refused("seed must lie in [0, 2^64), not -1", e.policy_rollout_noise, 2, -1, noise_std=1.0)
    for call, args in ((e.design_descent, (sp, 2, 3, 2)), (e.plant_identify, (2,))):
        _refused("stiffness_bounds must be a pair (lo, hi)", call, *args, stiffness_bounds=(1.0, 2.0, 3.0))
        _refused("motor_inertia_bounds entries must have shape [B=3, nj=2], [nj] or be scalars, not [3, 3]", call, *args,
                 motor_inertia_bounds=(ones(3), 2.0))
        _refused("stiffness_bounds entries must have shape [B=3, nj=2], [nj] or be scalars, not [2, 2]", call, *args,
                 stiffness_bounds=(1.0, ones((2, 2))))
    _refused("weights must have shape [B=3, nx=8] or [nx], not [3, 7]", e.plant_identify, 2, weights=ones(7), motor_inertia_bounds=(1e-6, 1e3))
    _refused("disturbance must have shape [B=3, n_steps=2, nx=8]", e.mpc_run, sp, 2, 3, 2, disturbance=ones((3, 4, 8)))
    _refused("disturbance must have shape [3, 4, 8], not [3, 2, 8]", e.mpc_run_plant, sp, 2, 3, 2, hold=2, disturbance=ones((3, 2, 8)))
    _refused("plant_stiffness must have shape [3, 2], not [2]", e.mpc_run_plant, sp, 2, 3, 2, plant_stiffness=ones(2))
    _refused("dx0 must have shape [3, 2, 8], not [3, 8]", e.policy_rollout, 2, dx0=ones((3, 8)))
    _refused("xs must have shape [B=3, T+1=5, nx=8]", e.set_candidate, ones((3, 4, 8)), None)
    _refused("us must have shape [B=3, T=4, nu=2]", e.set_candidate, None, ones((5, 2)))
    _refused("x0s must have shape [P, nx=8]", e.solve_pool, ones((5, 7)), None, sp)
    _refused("frame_refs must have shape [P, 12]", e.solve_pool, ones((5, 8)), ones((5, 11)), sp)
    _refused("xs_init must have shape [P, T+1, nx]", e.solve_pool, ones((5, 8)), None, sp, xs_init=ones((5, 4, 8)))
    _refused("us_init must have shape [P, T, nu]", e.solve_pool, ones((5, 8)), None, sp, us_init=ones((4, 4, 2)))


def test_the_calls_that_switch_entry_point_by_size_on_the_arm():
    """talos_arm_sea (7 joints: aslr_policy_rollout_all, aslr_mpc_run_plant_all), S = 2, n_steps = 2, hold = 2: the kept
    trajectories and the closed cost change no other field, the shapes are the documented ones, the refusals name the shapes
    of this size"""
    S, rng = 2, np.random.default_rng(5)
    e, sp, _ = _solved("talos_arm_sea")
    dx0 = 1e-3 * rng.standard_normal((B, S, 28))
    kept, lean = e.policy_rollout(S, dx0=dx0, keep_trajectories=True), e.policy_rollout(S, dx0=dx0)
    gc.sync()
    assert tuple(kept.xs.shape) == (B, S, T + 1, 28) and tuple(kept.us.shape) == (B, S, T, 7) and lean.xs is None and lean.us is None
    for k in ("cost", "failed_knot", "x_final"):
        gc.same_bits(getattr(kept, k), getattr(lean, k), k)
    assert (kept.failed_knot == -1).all()
    _refused("dx0 must have shape [3, 2, 28], not [3, 28]", e.policy_rollout, S, dx0=np.ones((3, 28)))
    _refused("disturbance must have shape [3, 4, 28], not [3, 2, 28]", e.mpc_run_plant, sp, 2, 3, 2, hold=2, disturbance=np.ones((3, 2, 28)))
    dist = 1e-4 * rng.standard_normal((B, 4, 28))
    runs = []
    for closed_cost in (True, False):
        e, sp, _ = _solved("talos_arm_sea")
        e.set_candidate(None, None)
        runs.append(e.mpc_run_plant(sp, 2, 3, 2, hold=2, disturbance=dist, closed_cost=closed_cost))
    with_cost, without = runs
    assert tuple(with_cost.xs_closed.shape) == (B, 5, 28) and tuple(with_cost.us_closed.shape) == (B, 4, 7) and with_cost.hold == 2
    assert tuple(with_cost.closed_cost.shape) == (B,) and without.closed_cost is None
    for k in ("xs_closed", "us_closed", "iters", "status", "cost", "failed_knot"):
        gc.same_bits(getattr(with_cost, k), getattr(without, k), k)
