"""aslr_policy_rollout_noise on the GPU (include/aslr_to_amd_policy_noise.h; the PolicyNoiseArgs forms of
policy_rollout_kernel and policy_rollout_team_kernel, csrc/aslr_policy_noise.hpp) against three references:

 - the draws against the numpy generator of tests/_policy_noise.py, within DRAW_BOUND;
 - the roll-out against aslr_policy_rollout / aslr_policy_rollout_all fed the drawn arrays of the same run, bit for bit;
 - the roll-out against tests/_policy.rollout (the oracle's knot loop) on the HOST-drawn arrays, at the 1e-9 relative of the
   parity suites (max |a - b| / (1 + |b|)); tests/test_policy_noise_host.py shows that no sample of these cases diverges.

Shapes: tests/_policy_noise.KEYS.  The entry point is called raw, every output in a buffer of the test's own, followed by
guard words that must survive."""
import ctypes as C

import numpy as np
import pytest

import _ext_call as ext
import _gpu_case as gc
import _policy as pol
import _policy_noise as pn
import _policy_team as pt
from aslr_to_amd import _abi, crocoddyl, scenarios

pytestmark = pytest.mark.gpu

NAME = _abi.POLICY_NOISE_SYMBOLS[0]
DRAWN = ("plant_stiffness", "plant_motor_inertia", "dx0", "disturbance")   # named as the arguments of policy_rollout
FIELDS = ext.POLICY_FIELDS + DRAWN
SIGMA_OF = dict(plant_stiffness="stiffness_rel_std", plant_motor_inertia="motor_inertia_rel_std", dx0="dx0_std", disturbance="noise_std")
_TO_BATCH_MAJOR = dict(ext._POLICY_TO_BATCH_MAJOR, plant_stiffness=(2, 1, 0), plant_motor_inertia=(2, 1, 0), dx0=(1, 0, 2),
                       disturbance=(2, 0, 1, 3))
# max |drawn - numpy| / (sigma, or the nominal for the plant's draws) over all cases, measured on an MI355X: 7.23e-16 (the
# device library's log, sincospi and exp against numpy's; profiles/policy_noise/README.md).  The bound is 16 times that, as
# the issue sets it, and never above 1e-12.
DRAW_BOUND = 16 * 7.23e-16
assert DRAW_BOUND <= 1e-12


def _old(e):
    return "aslr_policy_rollout" if e.nx == 8 else "aslr_policy_rollout_all"


def _raw(e, S, sg, clamp=False, which=FIELDS, expect=_abi.OK, seed=pn.SEED, sample0=0, trajectory0=0, room=None):
    """the call with the sigmas `sg` (dict; missing or None: NULL; broadcast to [B, n]) and the outputs `which` -> batch-major
    arrays, or the message of the refusal"""
    R, nj = max(S if room is None else room, 1), e.nx // 4
    shapes = {"cost": (R, e.B), "failed_knot": (R, e.B), "x_final": (R, e.B, e.nx), "xs": (R, e.T + 1, e.B, e.nx),
              "us": (R, e.T, e.B, e.nu), "plant_stiffness": (nj, R, e.B), "plant_motor_inertia": (nj, R, e.B),
              "dx0": (R, e.B, e.nx), "disturbance": (R, e.T, e.B, e.nx)}
    outs = ext.outputs(e.device, shapes, which, perms=_TO_BATCH_MAJOR, int32=("failed_knot",))
    sig = lambda k, n: ext.dev(e.device, None if (sg or {}).get(k) is None else np.broadcast_to(np.asarray(sg[k], dtype=np.float64), (e.B, n)))
    ins = [sig("noise_std", e.nx), sig("dx0_std", e.nx), sig("stiffness_rel_std", nj), sig("motor_inertia_rel_std", nj)]
    return ext.call(e, NAME, [e.handle, S, sample0, trajectory0, C.c_uint64(seed)] + ins + [1 if clamp else 0]
                    + [outs.get(k) for k in FIELDS] + [e._stream()], outs, expect)


def _pert(got):
    """the drawn arrays of a call as the `pert` of ext.policy_rollout"""
    return {k: got.get(k) for k in DRAWN}


def _rollout(got):
    return {k: got[k] for k in ext.POLICY_FIELDS if k in got}


@pytest.fixture(scope="module")
def cases(oracle):
    """the seeded inputs of a case, built on first use and never changed"""
    made = {}

    def get(key):
        if key not in made:
            made[key] = pt.case(oracle, key) if isinstance(key, tuple) else pn.case(oracle, key)
        return made[key]
    return get


@pytest.fixture(scope="module")
def loaded(cases):
    """key -> (engine with the candidate and its gains in place, the device's K, the sigmas, the call with every sigma the
    model admits and every output), made on first use and shared: the call under test changes nothing it reads"""
    made = {}

    def get(key):
        if key not in made:
            c = cases(key)
            with pytest.MonkeyPatch.context() as mp:   # (pendulum_3d: the general 3-D chain; read when the handle is created)
                e, K = ext.with_gains(c, mp)
            sg = pn.sigmas(c["low"])
            which = tuple(k for k in FIELDS if k not in DRAWN or sg[SIGMA_OF[k]] is not None)
            made[key] = (e, K, sg, _raw(e, c["S"], sg, c["clamp"], which=which))
        return made[key]
    return get


def _draw_error(low, sg, got, want):
    worst = 0.0
    sc = pn.scale(low, sg)
    for k in DRAWN:
        if want[k] is None:
            assert k not in got
            continue
        worst = max(worst, float((np.abs(got[k] - want[k]) / sc[k]).max()))
    return worst


@pytest.mark.parametrize("key", pn.KEYS)
def test_draws_are_the_definition(cases, loaded, key):
    c = cases(key)
    e, K, sg, got = loaded(key)
    want = pn.draws(c["low"], c["S"], pn.SEED, **sg)
    err = _draw_error(c["low"], sg, got, want)
    print("%s: max |drawn - numpy| / scale %.2e (bound %.2e)" % (key, err, DRAW_BOUND))
    assert err <= DRAW_BOUND, err
    for k in DRAWN:   # ... and they are draws: no entry is zero, the plant's are not the nominal
        if want[k] is not None:
            assert (got[k] != 0.0).all() and (k in ("dx0", "disturbance") or (got[k] != pn.scale(c["low"], sg)[k]).all()), k


@pytest.mark.parametrize("key", pn.KEYS)
def test_rollout_is_the_existing_one(cases, loaded, key):
    """aslr_policy_rollout (2 joints) / aslr_policy_rollout_all (7 joints) on the drawn_* arrays of the same run: cost,
    failed_knot, x_final, xs_closed and us_closed bit for bit"""
    c = cases(key)
    e, K, sg, got = loaded(key)
    assert (got["failed_knot"] == -1).all()
    ext.same(_rollout(got), ext.policy_rollout(e, _old(e), c["S"], _pert(got), c["clamp"]), "%s: drawn inside against read from arrays" % key)


@pytest.mark.parametrize("key", pn.KEYS)
def test_kernel_matches_the_oracle_on_host_drawn_arrays(oracle, cases, loaded, key):
    c = cases(key)
    low, S = c["low"], c["S"]
    e, K, sg, got = loaded(key)
    want = pol.rollout(oracle, low, c["xs"], c["us"], K, S, clamp=c["clamp"], **pn.draws(low, S, pn.SEED, **sg))
    assert (want["failed_knot"] == -1).all()
    np.testing.assert_array_equal(got["failed_knot"], want["failed_knot"])
    for k in pol.OUTPUTS:
        print("%s %s: %.2e" % (key, k, gc.relerr(got[k], want[k])))
    for k in pol.OUTPUTS:
        gc._assert_close("%s %s" % (key, k), got[k], want[k], 1e-9)
    if c["clamp"]:
        assert want["bound"].any(), "the box must bind on some samples"


@pytest.mark.parametrize("key", ["sea_table", "arm_sea_table", "arm_vsa_box"])
def test_a_draw_follows_its_counter_not_the_launch(cases, loaded, key):
    """S = 17 in one call is samples [0, 16) plus a call with sample0 = 16, n_samples = 1, bit for bit, every output; the same
    seed twice is bit-equal; another seed (either key word) gives other draws"""
    c = cases(key)
    S = c["S"]
    assert S == 17
    e, K, sg, got = loaded(key)
    which = tuple(got)
    head = _raw(e, 16, sg, c["clamp"], which=which)
    tail = _raw(e, 1, sg, c["clamp"], which=which, sample0=16)
    ext.same({k: v[:, :16] for k, v in got.items()}, head, "%s: samples [0, 16)" % key)
    ext.same({k: v[:, 16:] for k, v in got.items()}, tail, "%s: sample 16 alone" % key)
    ext.same(_raw(e, S, sg, c["clamp"], which=which), got, "%s: the same seed twice" % key)
    for seed in (pn.SEED ^ 1, pn.SEED ^ (1 << 32)):
        other = _raw(e, S, sg, c["clamp"], which=which, seed=seed)
        for k in DRAWN:
            assert k not in got or (other[k] != got[k]).all(), (k, hex(seed))
        assert (other["cost"] != got["cost"]).all()


@pytest.mark.parametrize("key", ["sea_one", ("talos_arm_sea", False, False, 2, 3, 4, False, False)])
def test_trajectory0_draws_the_rows_of_the_whole_batch(cases, key):
    """trajectory0 = 3 (and sample0 = 5) on a handle of B trajectories: rows 3 .. 3 + B of the generator, on the handle's own
    nominals -- what a shard of a larger batch needs"""
    c = cases(key)
    low, S = c["low"], c["S"]
    e, K = ext.with_gains(c)
    sg = pn.sigmas(low)
    got = _raw(e, S, sg, sample0=5, trajectory0=3)
    want = pn.draws(low, S, pn.SEED, sample0=5, trajectory0=3, **sg)
    err = _draw_error(low, sg, got, want)
    print("%s: max |drawn - numpy| / scale %.2e" % (key, err))
    assert err <= DRAW_BOUND
    here = pn.draws(low, S, pn.SEED, **sg)
    assert all((here[k] != want[k]).all() for k in DRAWN)
    ext.same(_rollout(got), ext.policy_rollout(e, _old(e), S, _pert(got)), "the roll-out on those draws")


@pytest.mark.parametrize("key", ["sea_table", "arm_sea_plain"])
def test_every_sigma_alone(cases, loaded, key):
    """every sigma NULL but one, in turn: the draws of that source are those of the full call (a source does not depend on
    the others), the drawn_* buffers of the absent sources stay untouched behind their guards, and the roll-out is the
    existing one on that array alone -- the absent sources are NULL there too: no `+ 0.0`, the trajectory's own plant"""
    c = cases(key)
    S = c["S"]
    e, K, sg, full = loaded(key)
    for k in DRAWN:
        one = {SIGMA_OF[k]: sg[SIGMA_OF[k]]}
        got = _raw(e, S, one, which=ext.POLICY_FIELDS + (k,))
        ext.same(got[k], full[k], "%s: %s drawn alone" % (key, k))
        ext.same(_rollout(got), ext.policy_rollout(e, _old(e), S, {k: got[k]}), "%s: %s alone against the array form" % (key, k))
        # the absent sources with buffers given: not a word of them is written
        shapes = {"cost": (S, e.B), "plant_stiffness": (e.nx // 4, S, e.B), "plant_motor_inertia": (e.nx // 4, S, e.B),
                  "dx0": (S, e.B, e.nx), "disturbance": (S, e.T, e.B, e.nx)}
        outs = ext.outputs(e.device, shapes, ("cost",) + DRAWN)
        sig = ext.dev(e.device, np.broadcast_to(np.float64(sg[SIGMA_OF[k]]), (e.B, e.nx if k in ("dx0", "disturbance") else e.nx // 4)))
        ins = [sig if SIGMA_OF[k] == n else None for n in ("noise_std", "dx0_std", "stiffness_rel_std", "motor_inertia_rel_std")]
        ext.call(e, NAME, [e.handle, S, 0, 0, C.c_uint64(pn.SEED)] + ins + [0, outs["cost"], None, None, None, None]
                 + [outs[d] for d in DRAWN] + [e._stream()], outs)
        for d in DRAWN:
            assert ext.untouched(outs[d].buf) == (d != k), (k, d)


def test_the_call_leaves_the_workspace_as_it_was(cases, loaded):
    """after the call (every sigma, every output) the handle solves, from the empty candidate, to the bits of a fresh one"""
    c = cases("vsa_box")
    e, K, sg, got = loaded("vsa_box")
    _raw(e, c["S"], sg, c["clamp"], which=tuple(got))
    ext.solve_matches_a_fresh_handle(e, c["low"], c["sp"], ext.SOLVE_REGIONS, "after aslr_policy_rollout_noise")


def test_refusals_write_nothing_and_leave_a_live_handle(cases, loaded):
    c = cases("sea_table")
    e, _, sg, ok = loaded("sea_table")
    S = c["S"]

    def refused(eng, S_, sg_, *words, **kw):
        msg = _raw(eng, S_, sg_, expect=_abi.E_INVALID, **kw)
        assert msg.startswith(NAME + ":") and all(w in msg for w in words), msg

    for bad_s in (0, -3):   # the refusals of the shared body
        refused(e, bad_s, sg, "n_samples")
    refused(e, 16 * 65535 + 1, sg, "n_samples", "above", room=1)
    refused(e, S, sg, "NULL", which=DRAWN)   # (none of the five roll-out outputs)
    # the new ones
    refused(e, S, {}, "sigma", "NULL")
    refused(e, S, dict(sg, noise_std=None, dx0_std=None, stiffness_rel_std=None, motor_inertia_rel_std=None), "sigma")
    refused(e, S, sg, "sample0", sample0=-1)
    refused(e, S, sg, "trajectory0", trajectory0=-1)
    refused(e, S, sg, "sample0", "overflow", sample0=2 ** 31 - S)
    assert np.isfinite(_raw(e, 1, sg, which=("cost",), sample0=2 ** 31 - 2)["cost"]).all()   # the last admissible sample0
    ext.same(_raw(e, S, sg, c["clamp"], which=tuple(ok)), ok, "the handle after the refusals")
    cv = cases("vsa_box")
    ev = loaded("vsa_box")[0]
    refused(ev, cv["S"], dict(pn.SIGMAS), "VSA", "stiffness_rel_std")
    # K that is not diagonal: refused with a plant sigma, rolled out with the others
    low = scenarios.lower(scenarios.two_dof_sea(B=2, T=3, seed=4))
    for i in range(low.desc.nmodels):   # (the lowered description is what aslr_problem_create reads)
        low.desc.models[i].K[1] = low.desc.models[i].K[2] = 0.03
    e2 = ext.fresh(low)
    refused(e2, 2, dict(motor_inertia_rel_std=0.05), "diagonal")
    refused(e2, 2, dict(stiffness_rel_std=0.05), "diagonal")
    assert (_raw(e2, 2, dict(noise_std=3e-4, dx0_std=3e-3), which=("failed_knot",))["failed_knot"] == -1).all()
    # models that differ in a diagonal, no table: no single nominal for that diagonal's sigma
    for field, sigma, other in (("K", "stiffness_rel_std", "motor_inertia_rel_std"), ("B", "motor_inertia_rel_std", "stiffness_rel_std")):
        low = scenarios.lower(scenarios.two_dof_sea(B=2, T=3, seed=4))
        assert low.desc.nmodels >= 2
        getattr(low.desc.models[1], field)[0] *= 1.5
        e3 = ext.fresh(low)
        refused(e3, 2, {sigma: 0.05}, "differ in " + field, sigma)
        assert (_raw(e3, 2, {other: 0.05, "noise_std": 3e-4}, which=("failed_knot",))["failed_knot"] == -1).all()


def test_python_facade():
    """solver.policy_monte_carlo on two_dof_sea: the documented shapes, sigmas as scalar / [n] / [B, n], the bits of the raw
    call on the same engine; the kept draws passed to solver.policy_rollout give the same result; problem.policy_monte_carlo
    at the stored policy given explicitly returns the same bits"""
    import torch
    B, T, S = 3, 6, 5
    sc = scenarios.two_dof_sea(B=B, T=T, seed=4)
    problem = crocoddyl.ShootingProblem(sc["x0"], sc["running"], sc["terminal"], frame_refs=sc["frame_refs"])
    solver = getattr(crocoddyl, sc["solver"])(problem)
    solver.solve([], [], 5)
    e = problem.engine
    kw = dict(noise_std=3e-4, dx0_std=np.full(8, 3e-3), stiffness_rel_std=np.full((B, 2), 0.05), motor_inertia_rel_std=0.05)
    res = solver.policy_monte_carlo(S, pn.SEED, keep_trajectories=True, keep_draws=True, sample0=2, **kw)
    gc.sync()
    assert tuple(res.cost.shape) == (B, S) and tuple(res.failed_knot.shape) == (B, S) and res.failed_knot.dtype == torch.int32
    assert tuple(res.x_final.shape) == (B, S, 8) and tuple(res.xs.shape) == (B, S, T + 1, 8) and tuple(res.us.shape) == (B, S, T, 2)
    assert {k: tuple(v.shape) for k, v in res.draws.items()} == dict(plant_stiffness=(B, S, 2), plant_motor_inertia=(B, S, 2),
                                                                     dx0=(B, S, 8), disturbance=(B, S, T, 8))
    raw = _raw(e, S, pn.SIGMAS, clamp=sc["solver"] == "SolverBoxDDP", sample0=2)
    for k in ext.POLICY_FIELDS:
        ext.same(gc.to_np(getattr(res, k)), raw[k], k)
    for k in DRAWN:
        ext.same(gc.to_np(res.draws[k]), raw[k], k)
    back = solver.policy_rollout(S, keep_trajectories=True, **res.draws)
    for k in ext.POLICY_FIELDS:
        gc.same_bits(getattr(back, k), getattr(res, k), "the kept draws through policy_rollout: " + k)
    lean = solver.policy_monte_carlo(S, pn.SEED, sample0=2, **kw)
    assert lean.xs is None and lean.us is None and not hasattr(lean, "draws")
    gc.same_bits(lean.cost, res.cost, "costs without the trajectories and the draws")
    only = solver.policy_monte_carlo(S, pn.SEED, noise_std=3e-4, keep_draws=True)
    assert only.draws["dx0"] is None and only.draws["plant_stiffness"] is None and only.draws["disturbance"] is not None
    xs, us, K = (e.region(r).clone() for r in (_abi.R_XS, _abi.R_US, _abi.R_KGAIN))
    again = problem.policy_monte_carlo(xs.permute(1, 0, 2), us.permute(1, 0, 2), K.permute(1, 0, 2, 3), S, pn.SEED, sample0=2, **kw)
    gc.same_bits(again.cost, res.cost, "the stored policy given explicitly")
    with pytest.raises(ValueError):
        solver.policy_monte_carlo(S, pn.SEED, noise_std=np.ones(3))
