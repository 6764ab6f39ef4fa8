"""Shared by the GPU suites of the extension calls (aslr_cost_sensitivity, aslr_policy_rollout[_all], aslr_policy_covariance,
aslr_policy_plant_sensitivity, aslr_mpc_run_plant[_all], aslr_design_descent, ...), imported like _gpu_case
(`import _ext_call as ext`), in four layers:

 1. guarded output buffers: flat, sentinel-filled, GUARD sentinel words behind the payload.  Plain torch on any device, so
    tests/test_ext_call_host.py holds the checks to firing when they must, on a CPU;
 2. the guarded call: outputs(), call() and its two endings, conclude() -- a function of the return code, the expected one
    and the buffers, tested on the CPU as well -- the upload of an input, ptr();
 3. what the suites do around a call: bit equality of arrays and of dicts of arrays, a fresh engine, an engine with gains,
    a solve on a used handle against a fresh one;
 4. the raw calls that two suites share: the policy roll-outs and the MPC runs on a mismatched plant, by export name.

The suite of a NEW extension call writes its argument list and nothing else:

    def _raw(e, a_in, which=FIELDS, expect=_abi.OK):
        outs = ext.outputs(e.device, _shapes(e), which, perms=_TO_BATCH_MAJOR, int32=("failed_knot",))
        args = [e.handle, ext.dev(e.device, a_in, (1, 0, 2)), outs.get("cost"), outs.get("failed_knot"), e._stream()]
        return ext.call(e, "aslr_new_call", args, outs, expect)

_shapes(e) gives every output's shape in the library's layout, _TO_BATCH_MAJOR the permutation that makes it batch-major
(none: left as it is).  In `args`, None is NULL, a tensor or an output stands for its pointer, everything else is passed as it
is; an output that sits in a struct is placed with outs[k].buf.data_ptr().  What the suite gets: with expect == OK a dict of
owned numpy arrays, one per requested output, after the return code and every guard were checked; with any other `expect`
the text of aslr_last_error(), after the return code was checked and every word of every buffer was found untouched."""
import collections
import ctypes as C

import numpy as np

import _gpu_case as gc
from aslr_to_amd import _abi

GUARD = 64                # sentinel words behind every payload
SENTINEL = -7.25          # float64 outputs.  (Not 0: a write of the sentinel's own value cannot be seen, so it is a value no
SENTINEL_I32 = -7         # kernel here produces; int32 outputs are knot indices, counts and status words, never -7)
SOLVE_REGIONS = (_abi.R_XS, _abi.R_US, _abi.R_TRAJ_F, _abi.R_TRAJ_I)   # what a solve leaves on a handle
MPC_REGIONS = SOLVE_REGIONS + (_abi.R_X0,)                              # ... and a receding-horizon run


# ---------------------------------------------------------------------------------------------
# 1. guarded buffers (any torch device)
# ---------------------------------------------------------------------------------------------
def _sentinel(buf):
    return SENTINEL if buf.dtype.is_floating_point else SENTINEL_I32


def alloc(shape, device, int32=False):
    """-> flat buffer of prod(shape) + GUARD words, float64 (or int32), every word the dtype's sentinel"""
    import torch
    n = int(np.prod(shape, dtype=np.int64))
    return torch.full((n + GUARD,), SENTINEL_I32 if int32 else SENTINEL, dtype=torch.int32 if int32 else torch.float64, device=device)


def untouched(buf):
    """every word, payload and guard, is still the sentinel"""
    return bool((buf == _sentinel(buf)).all())


def guard_intact(buf):
    guard = buf[buf.numel() - GUARD:]
    assert guard.numel() == GUARD, "not a buffer of alloc()"
    return bool((guard == _sentinel(buf)).all())


def payload(buf, shape, perm=None):
    """-> the words before the guard as an owned numpy array of `shape`, transposed by `perm` and contiguous"""
    a = gc.to_np(buf[:buf.numel() - GUARD]).reshape(shape)
    return a if perm is None else np.ascontiguousarray(np.transpose(a, perm))


# ---------------------------------------------------------------------------------------------
# 2. the guarded call
# ---------------------------------------------------------------------------------------------
Out = collections.namedtuple("Out", "buf shape perm")


def outputs(device, shapes, which, perms=None, int32=()):
    """-> {name: Out} with a fresh guarded buffer for every name in `which`; shapes, perms: per name (perms may lack some)"""
    return {k: Out(alloc(shapes[k], device, k in int32), tuple(shapes[k]), (perms or {}).get(k)) for k in which}


def dev(device, v, perm=None):
    """numpy array or None, optionally transposed -> contiguous float64 tensor on the device, or None"""
    import torch
    if v is None:
        return None
    a = np.asarray(v) if perm is None else np.transpose(v, perm)
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=device)


def ptr(t):
    """a tensor, an Out or None -> c_void_p or None (NULL)"""
    if t is None:
        return None
    return C.c_void_p((t.buf if isinstance(t, Out) else t).data_ptr())


def conclude(rc, expect, outs, message, name="the call"):
    """The two endings of a guarded call.  A return code other than `expect` fails.  expect != OK: every word of every buffer
    must be untouched -> message.  expect == OK: every guard must be intact -> {name: payload}."""
    assert rc == expect, "%s returned %d where %d was expected: %s" % (name, rc, expect, message)
    if expect != _abi.OK:
        for k, o in outs.items():
            assert untouched(o.buf), "%s was written by the refused %s" % (k, name)
        return message
    for k, o in outs.items():
        assert guard_intact(o.buf), "the guard behind %s was overwritten by %s" % (k, name)
    return {k: payload(*o) for k, o in outs.items()}


def call(e, name, args, outs, expect=_abi.OK):
    """The export `name` on the engine's device with `args` (None: NULL; a tensor or an Out: its pointer; anything else as
    it is), a synchronisation, then conclude()."""
    import torch
    args = [ptr(a) if a is None or isinstance(a, (Out, torch.Tensor)) else a for a in args]
    with torch.cuda.device(e.device):
        rc = getattr(e.lib, name)(*args)
    gc.sync()
    return conclude(rc, expect, outs, e.lib.aslr_last_error().decode() if rc != _abi.OK else "", name)


# ---------------------------------------------------------------------------------------------
# 3. around a call
# ---------------------------------------------------------------------------------------------
def same(a, b, what):
    """Bit equality of two arrays, or of two dicts of arrays with the same keys: float64 as uint64, other dtypes as they
    are; None equals None only."""
    if isinstance(a, dict) or isinstance(b, dict):
        keys = [sorted(x) if isinstance(x, dict) else "no dict" for x in (a, b)]
        assert isinstance(keys[0], list) and keys[0] == keys[1], "%s: the keys differ: %s against %s" % (what, keys[0], keys[1])
        for k in a:
            same(a[k], b[k], "%s: %s" % (what, k))
        return
    if a is None or b is None:
        assert a is None and b is None, "%s: None on one side only" % what
        return
    a, b = (x.view(np.uint64) if x.dtype == np.float64 else x for x in (np.ascontiguousarray(a), np.ascontiguousarray(b)))
    np.testing.assert_array_equal(a, b, err_msg=what)


def fresh(low, nsub=1):
    """a new engine on the empty candidate"""
    e = gc.engine(low)
    if nsub > 1:
        e.set_subshards(nsub)
    e.set_candidate(None, None)
    return e


def with_gains(c, monkeypatch=None):
    """a fresh engine with the case's candidate in XS / US and the gains of one aslr_calc_diff + aslr_backward_pass on it in
    KGAIN (the case's own solver: SolverBoxDDP where the scenario has one) -> engine, K [T, B, nu, nx].  A case that asks for
    the general 3-D chain path gets it where a monkeypatch is passed."""
    import _policy as pol
    if monkeypatch is not None and c.get("three_d"):
        monkeypatch.setenv("ASLR_NO_PLANAR", "1")   # (read when the handle is created)
    low = c["low"]
    e = gc.engine(low)
    deriv = gc.run_calc_diff(e, c["xs"], c["us"])[2]
    out = gc.run_backward(e, c["sp"], c["us"], deriv, np.zeros((low.T + 1, low.B, low.nx)), pol.XREG, 1)
    assert (out["status"] & _abi.ST_BACKWARD_ERR == 0).all(), out["status"]
    assert np.abs(out["K"]).max() > 1e-3
    return e, out["K"]


def solve_matches_a_fresh_handle(e, low, sp, regions, what):
    """the handle and a new one solve from the empty candidate: `regions` bit for bit.  what: the words after "region N" """
    new = gc.engine(low)
    for h in (e, new):
        h.set_candidate(None, None)
        h.solve(sp, poll_every=4)
    gc.sync()
    for rid in regions:
        gc.same_bits(e.region(rid), new.region(rid), "region %d %s" % (rid, what))


# ---------------------------------------------------------------------------------------------
# 4. raw calls of two suites each
# ---------------------------------------------------------------------------------------------
POLICY_FIELDS = ("cost", "failed_knot", "x_final", "xs", "us")
_POLICY_TO_BATCH_MAJOR = {"cost": (1, 0), "failed_knot": (1, 0), "x_final": (1, 0, 2), "xs": (2, 0, 1, 3), "us": (2, 0, 1, 3)}
_POLICY_TO_DEVICE = {"plant_stiffness": (2, 1, 0), "plant_motor_inertia": (2, 1, 0), "dx0": (1, 0, 2), "disturbance": (1, 2, 0, 3)}


def policy_rollout(e, name, S, pert=None, clamp=False, which=POLICY_FIELDS, expect=_abi.OK, room=None):
    """aslr_policy_rollout or aslr_policy_rollout_all (`name`) with the batch-major inputs `pert` (missing or None: NULL) and
    the outputs `which` (the others NULL).  The buffers are sized for `room` samples (default S; at least 1, so that a refused
    S <= 0 still has buffers to inspect); failed_knot is int32.  -> call(): batch-major arrays in the layout of
    tests/_policy.rollout, or the message of the refusal."""
    R = max(S if room is None else room, 1)
    shapes = {"cost": (R, e.B), "failed_knot": (R, e.B), "x_final": (R, e.B, e.nx), "xs": (R, e.T + 1, e.B, e.nx),
              "us": (R, e.T, e.B, e.nu)}
    outs = outputs(e.device, shapes, which, perms=_POLICY_TO_BATCH_MAJOR, int32=("failed_knot",))
    ins = [dev(e.device, (pert or {}).get(k), perm) for k, perm in _POLICY_TO_DEVICE.items()]
    return call(e, name, [e.handle, S] + ins + [1 if clamp else 0] + [outs.get(k) for k in POLICY_FIELDS] + [e._stream()], outs, expect)


def mpc_run_plant(e, name, sp, n, first, per, hold=1, pk=None, pb=None, dist=None, clamp=False, cost=True, failed=True,
                  expect=_abi.OK):
    """aslr_mpc_run_plant or aslr_mpc_run_plant_all (`name`).  pk, pb: batch-major [B, nj] or None (NULL); dist: time-major
    [N, B, nx] or None; cost / failed: whether closed_cost / failed_knot are given.  -> dict of time-major numpy arrays:
    x [N+1, B, nx], u [N, B, nu], stat_f [n, 4, B], stat_i [n, 2, B], cost [B], failed [B] (None where not given), or the
    message of the refusal."""
    N = max(n, 0) * max(hold, 0)
    shapes = {"x": (N + 1, e.B, e.nx), "u": (N, e.B, e.nu), "stat_f": (max(n, 1), 4, e.B), "stat_i": (max(n, 1), 2, e.B),
              "cost": (e.B,), "failed": (e.B,)}
    which = ("x", "u", "stat_f", "stat_i") + (("cost",) if cost else ()) + (("failed",) if failed else ())
    outs = outputs(e.device, shapes, which, int32=("stat_i", "failed"))
    td = dev(e.device, dist)
    mpc = _abi.Mpc()
    mpc.n_steps, mpc.first_maxiter, mpc.iters_per_step = n, first, per
    mpc.disturbance = None if td is None else td.data_ptr()
    mpc.x_closed, mpc.u_closed, mpc.stat_f, mpc.stat_i = (outs[k].buf.data_ptr() for k in ("x", "u", "stat_f", "stat_i"))
    got = call(e, name, [e.handle, C.byref(sp), C.byref(mpc), hold, dev(e.device, pk, (1, 0)), dev(e.device, pb, (1, 0)),
                         1 if clamp else 0, outs.get("cost"), outs.get("failed"), e._stream()], outs, expect)
    return got if expect != _abi.OK else dict({"cost": None, "failed": None}, **got)
