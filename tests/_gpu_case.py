"""Shared by the GPU parity suites (tests/test_gpu_*.py), imported like _parity (`import _gpu_case as gc`), in three layers:

 1. basics, one definition each: a fresh engine, a synchronisation, owned numpy copies, the relative error, bit equality;
 2. inputs and launches (these need a GPU): the seeded recipes for the inputs of aslr_backward_pass and aslr_forward_pass --
    a random candidate, gaps drawn from U(-0.05, 0.05), gains from the oracle's backward pass scaled by 0.05 so that the
    rollout of every step length stays finite -- the uploads and the launch of each kernel-level entry point, and a solve
    collected in the shape _parity.compare takes;
 3. comparisons of numpy arrays with oracle results.  They take no engine and no tensor, so tests/test_gpu_case_host.py
    holds them to failing when they must, on a CPU."""
import numpy as np

from aslr_to_amd import _abi

SOLVERS = {"SolverDDP": _abi.SOLVER_DDP, "SolverFDDP": _abi.SOLVER_FDDP, "SolverBoxDDP": _abi.SOLVER_BOXDDP}
BACKWARD_FIELDS = ("K", "k", "Qu", "Vx", "Vxx", "d1", "d2", "stop")


# ---------------------------------------------------------------------------------------------
# 1. basics
# ---------------------------------------------------------------------------------------------
def engine(low):
    """Always a new handle: the library reads ASLR_BWD_HS, ASLR_BLK_MFMA, ASLR_PIPELINE, ASLR_NO_PLANAR and
    ASLR_PLANAR_REACH when one is created, and the tests set them just before."""
    from aslr_to_amd.engine import Engine
    return Engine(low)


def sync():
    import torch
    torch.cuda.synchronize()


def to_np(t):
    """An owned copy (of a tensor or an array): the next launch overwrites the buffer, not what the test holds."""
    return np.array(t if isinstance(t, np.ndarray) else t.detach().cpu().numpy())


def relerr(a, b):
    """max |a - b| / (1 + |b|), 0 for empty arrays: the one definition (tests/_policy.py and tests/_sensitivity.py pass it on
    to the host suites under their own names; tests/_covariance.traj_relerr is another measure)"""
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b) / (1.0 + np.abs(b)))) if a.size else 0.0


def bits(t):
    import torch
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


def same_bits(a, b, what):
    """two tensors, compared where they lie; tests/_ext_call.same is the same comparison of numpy arrays and dicts of them"""
    import torch
    assert a.shape == b.shape and torch.equal(bits(a), bits(b)), what


# ---------------------------------------------------------------------------------------------
# 2. inputs and launches
# ---------------------------------------------------------------------------------------------
def random_candidate(low, seed):
    rng = np.random.default_rng(seed)
    xs = rng.uniform(-0.8, 0.8, (low.T + 1, low.B, low.nx))
    us = rng.uniform(-1.0, 1.0, (low.T, low.B, low.nu))
    if low.dam == _abi.DAM_VSA:
        us[..., low.nu // 2:] = rng.uniform(0.1, 5.0, (low.T, low.B, low.nu // 2))
    return xs, us


def backward_inputs(oracle, low, seed, clip=None, candidate=None):
    """-> xs, us, deriv, gaps.  clip = (lb, ub): the controls are clipped to the box before the oracle makes the records.
    candidate = (xs, us): that candidate in place of random_candidate(low, seed); the gaps are drawn from the seed as ever."""
    xs, us = random_candidate(low, seed) if candidate is None else candidate
    if clip is not None:
        us = np.clip(us, *clip)
    _, _, deriv = oracle.calc_diff(low, xs, us)
    gaps = np.random.default_rng(seed + 7).uniform(-0.05, 0.05, (low.T + 1, low.B, low.nx))
    return xs, us, deriv, gaps


def forward_inputs(oracle, low, sp, seed, fddp, feasible=None, full=False, candidate=None):
    """-> xs, us, K, k, gaps (full: also the oracle's backward pass the gains come from, with its unscaled Vxx).  fddp: the
    backward pass runs infeasible, so that its value function carries the gap terms; feasible: one flag per trajectory
    instead; candidate = (xs, us): as in backward_inputs."""
    xs, us, deriv, gaps = backward_inputs(oracle, low, seed, candidate=candidate)
    if feasible is None:
        feasible = 0 if fddp else 1
    ref_b = oracle.backward_pass(low, sp, deriv, gaps, us, 1e-3, feasible)
    out = (xs, us, 0.05 * ref_b["K"], 0.05 * ref_b["k"], gaps)   # mild gains keep every alpha's rollout finite
    return out + (ref_b,) if full else out


def _upload(e, **regions):
    import torch
    for name, v in regions.items():
        e.region(getattr(_abi, "R_" + name)).copy_(torch.as_tensor(v))


def _set_feasible(e, feasible):
    import torch
    if np.ndim(feasible):
        e.region(_abi.R_TRAJ_I)[_abi.TI_FEASIBLE].copy_(torch.as_tensor(np.asarray(feasible, dtype=np.int32)))
    else:
        e.region(_abi.R_TRAJ_I)[_abi.TI_FEASIBLE].fill_(int(feasible))


def run_forward(low, sp, xs, us, K, k, gaps, feasible, vxxf=None):
    """A fresh engine, the inputs in place, aslr_forward_pass.  gaps: None leaves R_GAPS as created (zero); feasible: one
    value or one per trajectory; vxxf: R_VXXF, the `Vxx f` the FDDP rollout reads for its dv."""
    e = engine(low)
    _upload(e, XS=xs, US=us, KGAIN=K, KFF=k)
    if gaps is not None:
        _upload(e, GAPS=gaps)
    if vxxf is not None:
        _upload(e, VXXF=vxxf)
    _set_feasible(e, feasible)
    e.forward_pass(sp)
    sync()
    return e


def forward_outputs(e):
    """-> XS_TRY, US_TRY, the NALPHA rows of trial costs: what assert_forward_matches takes"""
    tf = to_np(e.region(_abi.R_TRAJ_F))
    return to_np(e.region(_abi.R_XS_TRY)), to_np(e.region(_abi.R_US_TRY)), tf[_abi.TF_COST_TRY0:_abi.TF_COST_TRY0 + _abi.NALPHA]


def run_calc_diff(e, xs, us):
    """xs, us (arrays, or tensors on the engine's device) in place, aslr_calc_diff -> XNEXT, COST, DERIV"""
    _upload(e, XS=xs, US=us)
    e.calc_diff()
    sync()
    return tuple(to_np(e.region(r)) for r in (_abi.R_XNEXT, _abi.R_COST, _abi.R_DERIV))


def run_calc(e):
    """aslr_calc alone on what XS / US hold, into a zeroed XNEXT and COST -> XNEXT, COST"""
    e.region(_abi.R_XNEXT).zero_()
    e.region(_abi.R_COST).zero_()
    e.calc()
    sync()
    return to_np(e.region(_abi.R_XNEXT)), to_np(e.region(_abi.R_COST))


def check_calc_and_calc_diff(oracle, low, seed=1):
    """calcDiff, calc alone, and calcDiff at a second point (seed + 4), each against the oracle.  The second sweep does not
    rewrite the record chunks that are structural zeros or depend on the model only (DERIV was zero-filled at creation, the
    first sweep put the cost-weight diagonals in place).  -> the engine"""
    e = engine(low)
    xs, us = random_candidate(low, seed)
    ref = oracle.calc_diff(low, xs, us)
    assert_records_match(*run_calc_diff(e, xs, us), ref=ref)
    assert_records_match(*run_calc(e), None, ref=ref)
    xs2, us2 = random_candidate(low, seed + 4)
    ref2 = oracle.calc_diff(low, xs2, us2)
    assert np.abs(ref2[2] - ref[2]).max() > 1e-3        # the point really changed
    assert_records_match(*run_calc_diff(e, xs2, us2), ref=ref2)
    return e


def run_backward(e, sp, us, deriv, gaps, xreg, feasible, k0=None, prefill=None):
    """The inputs in place (xreg, feasible: one value or one per trajectory; k0: the stored k, SolverBoxDDP's warm start;
    None: zero), TI_STATUS cleared, aslr_backward_pass -> dict(K, k, Qu, Vx, Vxx, d1, d2, stop, status, and Vxxf, dg, dq:
    R_VXXF, TF_DG, TF_DQ, which SolverFDDP's sweep writes -- the oracle returns dg, dq as ITS d1, d2 under that solver).
    prefill: a float64 whose bit pattern fills the TF_D1 / TF_D2 / TF_STOP / TF_DG / TF_DQ rows and KGAIN, QU, VX, VXX,
    VXXF -- and KFF where no k0 is given -- before the launch, so that wrote(out[name], prefill) tells which entries the
    launch wrote."""
    import torch
    _upload(e, US=us, DERIV=deriv, GAPS=gaps)
    if prefill is not None:
        for rid in (_abi.R_KGAIN, _abi.R_QU, _abi.R_VX, _abi.R_VXX, _abi.R_VXXF):
            e.region(rid).fill_(prefill)
        for row in (_abi.TF_D1, _abi.TF_D2, _abi.TF_STOP, _abi.TF_DG, _abi.TF_DQ):
            e.region(_abi.R_TRAJ_F)[row].fill_(prefill)
    if k0 is None:
        e.region(_abi.R_KFF).fill_(0.0 if prefill is None else prefill)
    else:
        _upload(e, KFF=k0)
    if np.ndim(xreg):
        e.region(_abi.R_TRAJ_F)[_abi.TF_XREG].copy_(torch.as_tensor(np.asarray(xreg, dtype=np.float64)))
    else:
        e.region(_abi.R_TRAJ_F)[_abi.TF_XREG].fill_(xreg)
    _set_feasible(e, feasible)
    e.region(_abi.R_TRAJ_I)[_abi.TI_STATUS].fill_(0)
    e.backward_pass(sp)
    sync()
    out = dict(K=to_np(e.region(_abi.R_KGAIN)), k=to_np(e.region(_abi.R_KFF)), Qu=to_np(e.region(_abi.R_QU)),
               Vx=to_np(e.region(_abi.R_VX)), Vxx=to_np(e.region(_abi.R_VXX)), Vxxf=to_np(e.region(_abi.R_VXXF)))
    for fld, name in ((_abi.TF_D1, "d1"), (_abi.TF_D2, "d2"), (_abi.TF_STOP, "stop"), (_abi.TF_DG, "dg"), (_abi.TF_DQ, "dq")):
        out[name] = to_np(e.traj_f(fld))
    out["status"] = to_np(e.traj_i(_abi.TI_STATUS))
    return out


def solution(e):
    """What a solve left on the handle, in the shape _parity.compare takes (log: only with an iteration log enabled)"""
    out = dict(xs=to_np(e.region(_abi.R_XS)), us=to_np(e.region(_abi.R_US)), traj_f=to_np(e.region(_abi.R_TRAJ_F)),
               traj_i=to_np(e.region(_abi.R_TRAJ_I)))
    if e.iteration_log() is not None:
        out["log"] = to_np(e.iteration_log())
    return out


def solve_gpu(low, sp, xs=None, us=None, subshards=1, log_cap=0, poll_every=4):
    """A fresh engine solves from the candidate xs [T+1, B, nx], us [T, B, nu] (time-major, the oracle's layout; None: the
    empty one) -> (engine, solution(engine))"""
    e = engine(low)
    if subshards > 1:
        e.set_subshards(subshards)
    if log_cap:
        e.enable_iteration_log(log_cap)
    e.set_candidate(None if xs is None else xs.transpose(1, 0, 2), None if us is None else us.transpose(1, 0, 2))
    e.solve(sp, poll_every=poll_every)
    sync()
    return e, solution(e)


# ---------------------------------------------------------------------------------------------
# 3. comparisons (numpy and oracle results only)
# ---------------------------------------------------------------------------------------------
def _assert_close(what, got, ref, tol):
    err = np.abs(np.asarray(got) - ref) / (1.0 + np.abs(ref))
    worst = err.max() if err.size else 0.0
    where = np.unravel_index(np.nanargmax(err), err.shape) if err.size and not np.isnan(err).all() else ()
    print("%s relerr %.2e" % (what, worst))
    assert worst < tol, "%s mismatch: relerr %g at %s (tolerance %g)" % (what, worst, where, tol)


def assert_records_match(xnext, cost, deriv, ref, tol_state=1e-11, tol_deriv=1e-9):
    """XNEXT, COST and the DERIV record against ref = (xnext, cost, deriv) of the oracle's calc_diff.  None: not compared
    (aslr_calc writes no record)."""
    for what, got, want, tol in (("xnext", xnext, ref[0], tol_state), ("cost", cost, ref[1], tol_state),
                                 ("DERIV record", deriv, ref[2], tol_deriv)):
        if got is not None:
            _assert_close(what, got, want, tol)


def assert_backward_matches(out, ref, tol, fields=BACKWARD_FIELDS):
    """out: run_backward's dict; ref: the oracle's backward pass, which must not have failed on any trajectory."""
    assert not np.asarray(ref["fail"]).any(), "the oracle's backward pass failed"
    assert (np.asarray(out["status"]) & _abi.ST_BACKWARD_ERR == 0).all(), "ST_BACKWARD_ERR is set: %s" % out["status"]
    for name in fields:
        _assert_close(name, out[name], ref[name], tol)


def per_trajectory(a, ok):
    """the entries that belong to the trajectories of mask ok (axis 1 of the per-knot arrays, axis 0 of d1 / d2 / stop)"""
    a = np.asarray(a)
    return a[ok] if a.ndim == 1 else a[:, ok]


def assert_backward_matches_where_ok(out, ref, tol, fields=BACKWARD_FIELDS):
    """out: run_backward's dict; ref: the oracle's backward pass of a MIXED batch: it must fail on some trajectories and
    not on all.  ST_BACKWARD_ERR must be set on exactly the trajectories the oracle fails on; on the others every field
    matches as in assert_backward_matches.  -> the mask of the surviving trajectories"""
    fail = np.asarray(ref["fail"]) != 0
    assert fail.any(), "no mixed case: the oracle's backward pass fails on no trajectory"
    assert not fail.all(), "no mixed case: the oracle's backward pass fails on every trajectory"
    err = (np.asarray(out["status"]) & _abi.ST_BACKWARD_ERR) != 0
    assert err[fail].all(), "ST_BACKWARD_ERR is missing on trajectories %s the oracle fails on" % np.nonzero(fail & ~err)[0]
    assert not err[~fail].any(), "ST_BACKWARD_ERR is set on trajectories %s the oracle does not fail on" % np.nonzero(err & ~fail)[0]
    for name in fields:
        _assert_close(name, per_trajectory(out[name], ~fail), per_trajectory(ref[name], ~fail), tol)
    return ~fail


def wrote(a, prefill):
    """-> bool per entry: the entry no longer holds the bit pattern of run_backward's prefill"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a.view(np.uint64) != np.array([prefill], dtype=np.float64).view(np.uint64)[0]


def assert_forward_matches(XT, UT, cost_try_rows, oracle_forward, tol=1e-9):
    """XT, UT [NALPHA, ...] and the NALPHA rows of trial costs against the oracle's forward pass of every step length.
    oracle_forward: alpha -> (xs_try, us_try, cost_try, fail), or the NALPHA results themselves.  On the trajectories the
    oracle rolls out, candidates and costs agree within tol; on the others the cost is NaN.
    -> the per-alpha masks of the succeeding trajectories and the oracle's results"""
    oks, refs = [], []
    for a in range(_abi.NALPHA):
        ref = oracle_forward(0.5 ** a) if callable(oracle_forward) else oracle_forward[a]
        xs_try, us_try, cost_try, fail = ref
        ok = np.asarray(fail) == 0
        assert ok.any(), "the oracle's rollout fails on every trajectory at alpha index %d" % a
        got = np.asarray(cost_try_rows[a])
        _assert_close("xs_try[%d]" % a, XT[a][:, ok], xs_try[:, ok], tol)
        _assert_close("us_try[%d]" % a, UT[a][:, ok], us_try[:, ok], tol)
        _assert_close("cost_try[%d]" % a, got[ok], cost_try[ok], tol)
        assert np.isnan(got[~ok]).all(), "a finite trial cost where the oracle's rollout failed, alpha index %d" % a
        oks.append(ok)
        refs.append(ref)
    return oks, refs
