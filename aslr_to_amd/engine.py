"""GPU engine: one shooting-problem shard on one MI355X, behind the C ABI of include/aslr_to_amd.h.

PyTorch-ROCm is used for storage and streams only: ONE torch uint8 tensor is the workspace the HIP
library carves into regions; every region is exposed as a zero-copy typed torch view.  All
arithmetic happens in the hand-written HIP kernels (csrc/aslr_*.hip: one translation unit per kernel family and size).  No CPU fallback: if the
library or a GPU is missing this module raises.
"""
import ctypes as C

import numpy as np

from . import _abi
from .lowering import lower_problem, lower_reference_path, lower_traj_params


def _torch():
    import torch
    return torch


def _ptr(t):
    """A device tensor as the C ABI takes it: its address, NULL for None."""
    return None if t is None else C.c_void_p(t.data_ptr())


class _Result(object):
    """What an Engine call returns: its fields as attributes."""

    def __init__(self, **fields):
        self.__dict__.update(fields)


class MpcResult(_Result):
    """What Engine.mpc_run returns: batch-major device tensors, views of the time-major arrays the kernels wrote --
    xs_closed [B, n+1, nx], us_closed [B, n, nu_user], and per step's solve iters, status (int32), cost, stop, x_reg,
    step [B, n]; reference_row (int): the row of the reference path knot 0 reads after the run (0 without a path).
    Engine.mpc_run_plant returns the same with N = n * hold applied knots in xs_closed [B, N+1, nx] and us_closed
    [B, N, nu_user], plus closed_cost [B] (None when not asked for), failed_knot [B] (int32; -1: none) and hold."""


class SensitivityResult(_Result):
    """What Engine.cost_sensitivity returns: batch-major device tensors -- stiffness [B, nj] (dJ/dK_j; None for a VSA model,
    whose stiffness is a control), motor_inertia [B, nj] (dJ/dB_j), x0 [B, nx] (dJ/dx0) and costate [B, T+1, nx]."""


class PolicyRolloutResult(_Result):
    """What Engine.policy_rollout returns: batch-major device tensors -- cost [B, S] (NaN for a failed sample),
    failed_knot [B, S] (int32; -1: none), x_final [B, S, nx] and, when kept, xs [B, S, T+1, nx] and us [B, S, T, nu] (the
    models' own nu: padded controls are cut); xs and us are None otherwise."""


class PolicyCovarianceResult(_Result):
    """What Engine.policy_covariance returns: batch-major device tensors -- x_var [B, T+1, nx] (diagonal of Sigma_t), u_var
    [B, T, nu] (diagonal of K Sigma K^T; the models' own nu: padded controls are cut), cov_final [B, nx, nx] (Sigma_T),
    cost_increase [B] and, when kept, cov [B, T+1, nx, nx] (every Sigma_t); cov is None otherwise."""


class LqgResult(_Result):
    """What Engine.policy_lqg returns: batch-major device tensors -- x_var [B, T+1, nx] (diagonal of Sigma_t = Xh_t + P_t), u_var
    [B, T, nu] (diagonal of K Xh K^T; the models' own nu: padded controls are cut), est_var [B, T+1, nx] (diagonal of the
    posterior error covariance P_t), cov_final [B, nx, nx] (Sigma_T), est_cov_final [B, nx, nx] (P_T), cost_increase [B] and,
    when kept, kalman_gain [B, T+1, nx, ny] (L_t, columns in the order of `measured`; None otherwise); measured: the list of
    measured state entries the call used."""


class SmoothResult(_Result):
    """What Engine.estimate_states returns: batch-major device tensors -- xs [B, T+1, nx] (the smoothed states of the last
    iteration, before relax), neg_log_lik and step_norm [B, n_iters] (the filter's negative log-likelihood and max |xs - nominal|
    of every iteration) and, when the filter is kept, x_filt [B, T+1, nx] (the filter's posterior mean m_t), est_var
    [B, T+1, nx] (diagonal of P_t) and nis [B, T+1] (the normalised innovation squared), all of the last iteration (None
    otherwise); measured: the list of measured state entries the call used."""


class PlantSensitivityResult(_Result):
    """What Engine.policy_plant_sensitivity returns: batch-major device tensors -- dx_final_dstiffness,
    dx_final_dmotor_inertia [B, nx, nj] (dx_T/dK_j, dx_T/dB_j), dcost_dstiffness, dcost_dmotor_inertia [B, nj], x_var
    [B, T+1, nx] and u_var [B, T, nu] (the models' own nu; both None when no variance was given) and, when kept,
    dxs_dstiffness, dxs_dmotor_inertia [B, T+1, nx, nj] (None otherwise).  The stiffness fields are None for a VSA model."""


class DesignResult(_Result):
    """What Engine.design_descent returns: batch-major device tensors -- stiffness [B, nj] (the accepted diag K; None for a
    VSA model), motor_inertia [B, nj] (the accepted diag B), cost [B], xs [B, T+1, nx], us [B, T, nu] (the models' own nu) and,
    when the history is kept, cost_history, eta_history, predicted_history [B, n_steps], accepted_history [B, n_steps]
    (int32: 1 accepted, 0 rejected, -1 not evaluable), stiffness_history (None for VSA) and motor_inertia_history
    [B, n_steps, nj]: the candidate evaluated in every step."""


class IdentifyResult(_Result):
    """What Engine.plant_identify returns: batch-major device tensors -- stiffness [B, nj] (None for a VSA model) and
    motor_inertia [B, nj] (the fit where the field was fitted, the table's value otherwise), theta [B, np] (the fitted entries,
    stiffness first), sse [B], n_accepted [B] (int32), grad [B, np], information [B, np, np] (the Gauss-Newton matrix H in
    z = log theta, unpacked and symmetric), identifiable [B, np] (bool), mu [B] and, when the history is kept, theta_history
    [B, n_steps, np], sse_history [B, n_steps], decision_history [B, n_steps] (int32: 1 accepted, 0 rejected, -1 not
    evaluable)."""


class Engine(object):
    """ShootingProblem shard resident in HBM.  Region layouts: include/aslr_to_amd.h."""

    def __init__(self, lowered, device=None):
        torch = _torch()
        self.lib = _abi.load_library()
        if not torch.cuda.is_available():
            raise _abi.AslrError("aslr_to_amd needs a ROCm GPU (torch.cuda.is_available() is False); "
                                 "there is no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.low = lowered
        self.B, self.T, self.nx, self.nu, self.rec = lowered.B, lowered.T, lowered.nx, lowered.nu, lowered.rec
        self.nu_user = getattr(lowered, "nu_user", lowered.nu)  # < nu: controls are padded on the device (pad_u / cut_u)
        nbytes = self.lib.aslr_workspace_bytes(C.byref(lowered.desc))
        if nbytes <= 0:
            raise _abi.AslrError("invalid problem description (aslr_workspace_bytes = %d)" % nbytes)
        with torch.cuda.device(self.device):
            # zeroed, not empty: the library zeroes the regions a solve expects zeroed, but XS / US and the scratch are
            # whatever the allocator's block held, and a call on a handle whose candidate was never set would read that
            # (the fill is on the stream aslr_problem_create uploads on, so it is ordered before it)
            self.ws = torch.zeros(nbytes + 256, dtype=torch.uint8, device=self.device)
            off = (-self.ws.data_ptr()) % 256
            self.ws = self.ws[off:off + nbytes]
            self.handle = C.c_void_p()
            _abi.check(self.lib.aslr_problem_create(C.byref(lowered.desc), C.c_void_p(self.ws.data_ptr()),
                                                    nbytes, self._stream(), C.byref(self.handle)),
                       "aslr_problem_create")
        self._views = {}
        self._ref_path = None
        if getattr(lowered, "traj_params", None):
            self.upload_traj_params(lowered.traj_params)
        if getattr(lowered, "ref_path", None) is not None:
            self.upload_reference_path(*lowered.ref_path)

    def set_reference_path(self, path, row0=0):
        """Time-varying reference placements of this shard (aslr_set_reference_path): path [B, N, 12] (row-major R, p; host
        or lists of SE3) or None = back to the create-time references; knot t reads row min(row0 + t, N - 1)."""
        self.upload_reference_path(None if path is None else lower_reference_path(self.low.desc, path, row0), row0)

    def upload_reference_path(self, path_tm, row0=0):
        """path_tm: what lower_reference_path returned ([N, B, 12], time-major, validated) or a device tensor of that
        shape, or None.  The engine keeps the tensor alive while it is set (the library reads it where it lies)."""
        torch = _torch()
        if path_tm is None:
            self._call("aslr_set_reference_path", None, 0, 0, self._stream())
            self._ref_path = None
            return
        with torch.cuda.device(self.device):
            t = torch.as_tensor(path_tm, dtype=torch.float64, device=self.device).contiguous()
        if t.dim() != 3 or t.shape[1] != self.B or t.shape[2] != 12:
            raise ValueError("the time-major reference path must have shape [n_rows, B=%d, 12]" % self.B)
        self._call("aslr_set_reference_path", C.c_void_p(t.data_ptr()), int(t.shape[0]), int(row0), self._stream())
        self._ref_path = t  # (only once the library took it: a declined path leaves the earlier one set and alive)

    @property
    def reference_row(self):
        n = C.c_int32(0)
        self._call("aslr_reference_row", C.byref(n))
        return n.value

    def set_trajectory_params(self, stiffness=None, motor_inertia=None, u_lb=None, u_ub=None):
        """Per-trajectory diagonals of K and B ([B, nj]) and control boxes ([B, nu], or the models' own narrower nu:
        padded like lower_traj_params says) for the B trajectories of this shard (aslr_set_trajectory_params); every
        field optional, all None: back to the models' constants.  Callable between solves."""
        low = self.low
        self.upload_traj_params(lower_traj_params(low.desc, low.nj, low.nu, self.nu_user, low.dam, stiffness,
                                                  motor_inertia, u_lb, u_ub))

    def upload_traj_params(self, tp):
        """tp: what lower_traj_params returned (validated, device-sized), or None: no table"""
        if tp is None:
            self._call("aslr_set_trajectory_params", None, self._stream())
            return
        st = _abi.TrajParams()
        for name, a in tp.items():
            setattr(st, name, a.ctypes.data_as(C.POINTER(C.c_double)))
        self._call("aslr_set_trajectory_params", C.byref(st), self._stream())  # (synchronous upload: tp may die now)

    def _stream(self):
        torch = _torch()
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _f64(self, v):
        """v (array, tensor or None) as a float64 tensor on this engine's device; None stays None."""
        if v is None:
            return None
        torch = _torch()
        return torch.as_tensor(np.asarray(v, dtype=np.float64) if not torch.is_tensor(v) else v, dtype=torch.float64,
                               device=self.device)

    def _dev(self, v, shape, perm, name, message=None):
        """_f64(v), checked against the batch-major `shape`, permuted to the library's layout (perm None: as it is) and
        made contiguous.  message: the ValueError text, where a caller has its own."""
        if v is None:
            return None
        t = self._f64(v)
        if tuple(t.shape) != shape:
            raise ValueError(message or "%s must have shape %s, not %s" % (name, list(shape), list(t.shape)))
        return (t if perm is None else t.permute(*perm)).contiguous()

    def _bcast(self, v, shape, short, perm, message, nonneg=None, say_given=False):
        """_dev for a value that may come in a shorter form.  short: the accepted forms, each the tuple of the axes of
        `shape` it carries (() is a scalar); the other axes are broadcast.  message: the ValueError text of a wrong shape,
        {} in it the shape refused -- as far as it was broadcast, or as it was given (say_given).  nonneg: the ValueError
        text of a negative entry, where the caller refuses one."""
        if v is None:
            return None
        t = self._f64(v)
        said = list(t.shape)
        for axes in short:
            if t.dim() == len(axes):
                seen = [t.shape[axes.index(a)] if a in axes else 1 for a in range(len(shape))]
                t = t.reshape(seen).expand([-1 if a in axes else n for a, n in enumerate(shape)])
                break
        t = self._dev(t, shape, perm, None, message.format(list(t.shape) if not say_given else said))
        if nonneg and bool((t < 0).any()):
            raise ValueError(nonneg)
        return t

    def _bounds(self, fields, ones):
        """fields: (bounds, name) of the stiffness and of the motor inertia, bounds None or (lo, hi), each [B, nj], [nj] or a
        scalar -> lo, hi: the rows [nj, B] of the fields stacked.  A field whose bounds are None is rows of ones (never
        read) with `ones`, left out otherwise; (None, None) when that leaves nothing."""
        torch = _torch()
        B, nj = self.B, self.nx // 4
        los, his = [], []
        for bounds, name in fields:
            if bounds is None:
                if ones:
                    los.append(torch.ones((nj, B), dtype=torch.float64, device=self.device))
                    his.append(los[-1])
                continue
            if len(bounds) != 2:
                raise ValueError("%s must be a pair (lo, hi)" % name)
            lo, hi = (self._bcast(v, (B, nj), ((), (1,)), (1, 0), "%s entries must have shape [B=%d, nj=%d], [nj] or be scalars, "
                                  "not {}" % (name, B, nj)) for v in bounds)
            los.append(lo)
            his.append(hi)
        return (torch.cat(los), torch.cat(his)) if los else (None, None)

    def _zeros(self, *shape, dtype=None):
        """a zeroed tensor on this engine's device, float64 unless dtype says otherwise"""
        torch = _torch()
        with torch.cuda.device(self.device):
            return torch.zeros(shape, dtype=dtype or torch.float64, device=self.device)

    def _call(self, name, *args):
        """One C-ABI call with this engine's device current (the ABI launches on the thread's current device, on a
        stream that belongs to self.device): an Engine on cuda:1 works whatever the caller's current device is."""
        torch = _torch()
        with torch.cuda.device(self.device):
            _abi.check(getattr(self.lib, name)(self.handle, *args), name)

    def close(self):
        if getattr(self, "handle", None) is not None and self.handle.value:
            self.lib.aslr_problem_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- zero-copy views of the workspace regions ----
    def region(self, rid):
        torch = _torch()
        if rid in self._views:
            return self._views[rid]
        r = _abi.Region()
        _abi.check(self.lib.aslr_problem_region(self.handle, rid, C.byref(r)), "aslr_problem_region")
        raw = self.ws[r.offset:r.offset + r.bytes]
        B, T, nx, nu, rec = self.B, self.T, self.nx, self.nu, self.rec
        shapes = {
            _abi.R_XS: (T + 1, B, nx), _abi.R_US: (T, B, nu), _abi.R_XNEXT: (T + 1, B, nx),
            _abi.R_COST: (T + 1, B), _abi.R_DERIV: (T + 1, B, rec), _abi.R_GAPS: (T + 1, B, nx),
            _abi.R_KGAIN: (T, B, nu, nx), _abi.R_KFF: (T, B, nu), _abi.R_QU: (T, B, nu),
            _abi.R_VX: (T + 1, B, nx), _abi.R_VXX: (T + 1, B, nx, nx),
            _abi.R_XS_TRY: (_abi.NALPHA, T + 1, B, nx), _abi.R_US_TRY: (_abi.NALPHA, T, B, nu),
            _abi.R_TRAJ_F: (_abi.TF_COUNT, B), _abi.R_X0: (B, nx), _abi.R_FRAME_REF: (B, 12),
            _abi.R_VXXF: (T + 1, B, nx), _abi.R_COST_TRY: (_abi.NALPHA, T + 1, B),
        }
        if rid in (_abi.R_XS_TRY, _abi.R_US_TRY):
            # candidate slabs: for even widths <= 8 piece-interleaved in groups of 4 trajectories
            # ([ceil(B / 4)][w / 2][4][2], include/aslr_to_amd.h) -- returned as a de-interleaved COPY
            # [NALPHA][knots][B][w] (not cached: it would go stale)
            w, knots = (nx, T + 1) if rid == _abi.R_XS_TRY else (nu, T)
            f = raw.view(torch.float64)
            if w % 2 == 0 and w <= 8:
                G = (B + 3) // 4
                return (f.view(_abi.NALPHA, knots, G, w // 2, 4, 2).permute(0, 1, 2, 4, 3, 5)
                        .reshape(_abi.NALPHA, knots, G * 4, w)[:, :, :B].contiguous())
            return f.view(_abi.NALPHA, knots, B, w)
        if rid == _abi.R_TRAJ_I:
            v = raw.view(torch.int32).view(_abi.TI_COUNT, B)
        elif rid == _abi.R_NODE_MODEL:
            v = raw.view(torch.int32)
        elif rid in shapes:
            v = raw.view(torch.float64).view(*shapes[rid])
        else:
            v = raw
        self._views[rid] = v
        return v

    def _traj_table(self):
        """the per-trajectory parameter table in R_TRAJ_PARAMS as the kernels read it: [2 nj + 2 nu, B] doubles (a view)"""
        return self.region(_abi.R_TRAJ_PARAMS).view(_torch().float64).view(2 * (self.nx // 4) + 2 * self.nu, self.B)

    # batch-major views ([B, T, ...]) of the time-major storage
    @property
    def xs(self):
        return self.region(_abi.R_XS).permute(1, 0, 2)

    @property
    def us(self):
        return self.region(_abi.R_US).permute(1, 0, 2)

    def pad_u(self, u):
        """[..., nu_user] -> [..., nu] (zeros in the padded commands); tensors and arrays pass through otherwise."""
        if self.nu_user == self.nu or u.shape[-1] != self.nu_user:
            return u
        torch = _torch()
        if torch.is_tensor(u):
            return torch.cat([u, torch.zeros(u.shape[:-1] + (self.nu - self.nu_user,), dtype=u.dtype, device=u.device)], dim=-1)
        return np.concatenate([u, np.zeros(u.shape[:-1] + (self.nu - self.nu_user,))], axis=-1)

    def cut_u(self, v, axis=-1):
        """the models' own controls out of a device-sized array (axis = the control axis)"""
        if self.nu_user == self.nu:
            return v
        idx = [slice(None)] * v.ndim
        idx[axis] = slice(0, self.nu_user)
        return v[tuple(idx)]

    def deriv_block(self, name):
        """[T+1, B, rows, cols] view of one block of the DERIV records."""
        o = _abi.record_offsets(self.nx, self.nu)
        nx, nu = self.nx, self.nu
        shp = {"Fx": (nx, nx), "Fu": (nx, nu), "Lxx": (nx, nx), "Lxu": (nx, nu), "Luu": (nu, nu),
               "Lx": (nx,), "Lu": (nu,)}[name]
        n = int(np.prod(shp))
        d = self.region(_abi.R_DERIV)
        return d[:, :, o[name]:o[name] + n].reshape(self.T + 1, self.B, *shp)

    def set_candidate(self, xs=None, us=None):
        """xs: [B, T+1, nx] / [T+1, nx] / list of arrays; us likewise.  None -> zeros
        (crocoddyl setCandidate with empty lists: state.zero() and zero controls)."""
        X, U = self.region(_abi.R_XS), self.region(_abi.R_US)
        for v, dst, text in ((xs, X, "xs must have shape [B=%d, T+1=%d, nx=%d]"), (us, U, "us must have shape [B=%d, T=%d, nu=%d]")):
            if v is None or (hasattr(v, "__len__") and len(v) == 0):
                dst.zero_()
                continue
            t = self._f64(v)
            if t.dim() == 2:
                t = t.unsqueeze(0).expand(self.B, -1, -1)
            if dst is U:
                t = self.pad_u(t)
            knots, B, width = dst.shape
            if tuple(t.shape) != (B, knots, width):
                raise ValueError(text % (B, knots, width))
            dst.copy_(t.permute(1, 0, 2))

    # ---- the hot path ----
    def calc(self):
        self._call("aslr_calc", self._stream())

    def calc_diff(self):
        self._call("aslr_calc_diff", self._stream())

    def backward_pass(self, sp):
        self._call("aslr_backward_pass", C.byref(sp), self._stream())

    def forward_pass(self, sp):
        self._call("aslr_forward_pass", C.byref(sp), self._stream())

    def iterate(self, sp, first):
        self._call("aslr_iterate", C.byref(sp), 1 if first else 0, self._stream())

    def iterate_n(self, sp, first, n):
        """n lock-step iterations in one ABI call (sub-shards run them free of each other, see set_subshards)."""
        self._call("aslr_iterate_n", C.byref(sp), 1 if first else 0, int(n), self._stream())

    def set_subshards(self, n):
        """Iterate the shard as n (1..4) sub-shards on internal streams: same results, bit for bit; the serial sweeps
        of one sub-shard overlap the streaming kernels of the others (include/aslr_to_amd.h: aslr_set_subshards)."""
        self._call("aslr_set_subshards", int(n))

    def iterate_timed(self, sp, first=False):
        """-> (calc_ms, backward_ms, forward_ms) of one iteration, from HIP events on the launch stream."""
        ms = (C.c_float * 3)()
        self._call("aslr_iterate_timed", C.byref(sp), 1 if first else 0, self._stream(), ms)
        return tuple(float(v) for v in ms)

    def quasi_static(self, maxiter=100, tol=1e-9):
        """Fill US with the quasi-static controls of the states in XS; returns the [T, B] iteration counts."""
        torch = _torch()
        iters = torch.zeros((self.T, self.B), dtype=torch.int32, device=self.device)
        self._call("aslr_quasi_static", int(maxiter), float(tol), C.c_void_p(iters.data_ptr()), self._stream())
        return iters

    def finalize(self):
        self._call("aslr_finalize", self._stream())

    def count_active(self):
        n = C.c_int32(0)
        self._call("aslr_count_active", self._stream(), C.byref(n))
        return n.value

    def solve(self, sp, poll_every=4):
        it = C.c_int32(0)
        self._call("aslr_solve", C.byref(sp), poll_every, self._stream(), C.byref(it))
        return it.value

    def cost_sensitivity(self):
        """Gradients of every trajectory's cost at the candidate in XS / US, controls held fixed, in its own spring
        stiffness, motor inertia and initial state, by one calcDiff sweep and one adjoint sweep (aslr_cost_sensitivity,
        include/aslr_to_amd_sens.h).  -> SensitivityResult.  Exact where the candidate has no gaps; at a converged
        solution also the gradient of the optimal cost; with gaps the gradient of the linearisation about (xs, us)."""
        nj, zeros = self.nx // 4, self._zeros
        vsa = self.low.dam == _abi.DAM_VSA
        dk, db, dx0, lam = (None if vsa else zeros(nj, self.B)), zeros(nj, self.B), zeros(self.nx, self.B), zeros(self.T + 1, self.B, self.nx)
        self._call("aslr_cost_sensitivity", _ptr(dk), _ptr(db), _ptr(dx0), _ptr(lam), self._stream())
        return SensitivityResult(stiffness=None if dk is None else dk.t(), motor_inertia=db.t(), x0=dx0.t(),
                                 costate=lam.permute(1, 0, 2))

    def policy_rollout(self, n_samples, plant_stiffness=None, plant_motor_inertia=None, dx0=None, disturbance=None,
                       clamp=False, keep_trajectories=False):
        """Closed-loop roll-outs of the policy in XS / US / KGAIN, u_t = us_t - K_t (x_t - xs_t), on n_samples = S perturbed
        plants per trajectory (aslr_policy_rollout, include/aslr_to_amd_policy.h; on the 7-joint arms aslr_policy_rollout_all,
        include/aslr_to_amd_policy_all.h).  Batch-major arrays or tensors, each
        optional: plant_stiffness, plant_motor_inertia [B, S, nj] (diagonals of the plant's K and B; None: the
        trajectory's own), dx0 [B, S, nx] (added to x0), disturbance [B, S, T, nx] (added to the next state of every
        knot).  clamp: clamp the control to the knot's box.  -> PolicyRolloutResult.  Writes nothing into the workspace.
        Before any backward sweep K = 0 and the roll-out is open loop; a non-positive plant inertia is not checked (it
        lives on the device) and shows up in failed_knot."""
        S, B, T, nx, nj = int(n_samples), self.B, self.T, self.nx, self.nx // 4
        if S > 0:  # (S <= 0: the library refuses by name)
            pk = self._dev(plant_stiffness, (B, S, nj), (2, 1, 0), "plant_stiffness")
            pb = self._dev(plant_motor_inertia, (B, S, nj), (2, 1, 0), "plant_motor_inertia")
            d0 = self._dev(dx0, (B, S, nx), (1, 0, 2), "dx0")
            w = self._dev(disturbance, (B, S, T, nx), (1, 2, 0, 3), "disturbance")
        else:
            pk = pb = d0 = w = None
        out = self._rollout_outputs(max(S, 0), keep_trajectories)
        # (2 joints: the entry point that has always served them; every other size: the one that serves all sizes)
        self._call("aslr_policy_rollout" if nj == 2 else "aslr_policy_rollout_all", S, _ptr(pk), _ptr(pb), _ptr(d0), _ptr(w),
                   1 if clamp else 0, *[_ptr(t) for t in out], self._stream())
        return self._rollout_result(*out)

    def _rollout_outputs(self, n, keep_trajectories):
        """the zeroed outputs of a roll-out of n samples as the library writes them: cost, failed_knot [n, B], x_final
        [n, B, nx] and, when kept, xs [n, T+1, B, nx] and us [n, T, B, nu] (None otherwise)"""
        B, T, nx, zeros = self.B, self.T, self.nx, self._zeros
        return (zeros(n, B), zeros(n, B, dtype=_torch().int32), zeros(n, B, nx),
                zeros(n, T + 1, B, nx) if keep_trajectories else None, zeros(n, T, B, self.nu) if keep_trajectories else None)

    def _rollout_result(self, cost, failed, xf, xs, us):
        """the batch-major PolicyRolloutResult of what _rollout_outputs made, once the library has written it"""
        return PolicyRolloutResult(cost=cost.t(), failed_knot=failed.t(), x_final=xf.permute(1, 0, 2),
                                   xs=None if xs is None else xs.permute(2, 0, 1, 3),
                                   us=None if us is None else self.cut_u(us.permute(2, 0, 1, 3)))

    def _sigma(self, v, n, name):
        """a sigma of policy_rollout_noise: None, a scalar, [n] or [B, n] -> None or a contiguous [B, n] device tensor"""
        return self._bcast(v, (self.B, n), ((), (1,)), None, "%s must be a scalar or have shape [%d] or [%d, %d], not {}"
                           % (name, n, self.B, n), say_given=True)

    def policy_rollout_noise(self, n_samples, seed, noise_std=None, dx0_std=None, stiffness_rel_std=None,
                             motor_inertia_rel_std=None, clamp=False, keep_trajectories=False, keep_draws=False, sample0=0,
                             trajectory0=0):
        """policy_rollout with the perturbations drawn on the device (aslr_policy_rollout_noise,
        include/aslr_to_amd_policy_noise.h, which defines the generator): sample s of trajectory b gets disturbance =
        noise_std z, dx0 = dx0_std z, K_j = Knom_j exp(stiffness_rel_std z), B_j = Bnom_j exp(motor_inertia_rel_std z) with
        standard normals z that depend on (seed, knot, sample0 + s, trajectory0 + b, entry) alone.  Each sigma is None (that
        source is absent), a scalar, [nx] / [nj] or [B, nx] / [B, nj]; at least one is given.  seed: an integer in
        [0, 2^64).  -> PolicyRolloutResult; with keep_draws it also has `draws`, a dict of batch-major tensors
        plant_stiffness, plant_motor_inertia [B, S, nj], dx0 [B, S, nx], disturbance [B, S, T, nx] (None for an absent
        source): the very arguments policy_rollout accepts.  Writes nothing into the workspace."""
        S, B, T, nx, nj = int(n_samples), self.B, self.T, self.nx, self.nx // 4
        seed = int(seed)
        if not 0 <= seed < 2 ** 64:
            raise ValueError("seed must lie in [0, 2^64), not %d" % seed)
        sw, s0 = self._sigma(noise_std, nx, "noise_std"), self._sigma(dx0_std, nx, "dx0_std")
        sk, sb = self._sigma(stiffness_rel_std, nj, "stiffness_rel_std"), self._sigma(motor_inertia_rel_std, nj, "motor_inertia_rel_std")
        n = max(S, 0)  # (S <= 0: the library refuses by name)
        out = self._rollout_outputs(n, keep_trajectories)
        kept = lambda sigma, *shape: self._zeros(*shape) if keep_draws and sigma is not None else None
        dk, db, d0, dw = kept(sk, nj, n, B), kept(sb, nj, n, B), kept(s0, n, B, nx), kept(sw, n, T, B, nx)
        self._call("aslr_policy_rollout_noise", S, int(sample0), int(trajectory0), C.c_uint64(seed), _ptr(sw), _ptr(s0), _ptr(sk),
                   _ptr(sb), 1 if clamp else 0, *[_ptr(t) for t in out], _ptr(dk), _ptr(db), _ptr(d0), _ptr(dw), self._stream())
        r = self._rollout_result(*out)
        if keep_draws:
            back = lambda t, *perm: None if t is None else t.permute(*perm)
            r.draws = dict(plant_stiffness=back(dk, 2, 1, 0), plant_motor_inertia=back(db, 2, 1, 0), dx0=back(d0, 1, 0, 2),
                           disturbance=back(dw, 2, 0, 1, 3))
        return r

    def _spread(self, sigma0, noise_var):
        """-> sigma0 [B, nx, nx] and noise_var [T, B, nx] on the device (None stays None), as policy_covariance and policy_lqg
        take them: broadcast, sigma0 symmetric, no negative variance.  Called under the engine's device."""
        torch = _torch()
        B, T, nx = self.B, self.T, self.nx
        s0 = self._bcast(sigma0, (B, nx, nx), ((1, 2),), None,
                         "sigma0 must have shape [B=%d, nx=%d, nx] or [nx, nx], not {}" % (B, nx))
        if s0 is not None:
            if not torch.equal(s0, s0.transpose(1, 2)):
                raise ValueError("sigma0 must be symmetric")
            if bool((torch.diagonal(s0, dim1=1, dim2=2) < 0).any()):
                raise ValueError("sigma0 has a negative variance on its diagonal")
        w = self._bcast(noise_var, (B, T, nx), ((2,), (0, 2)), (1, 0, 2),
                        "noise_var must have shape [B=%d, T=%d, nx=%d], [B, nx] or [nx], not {}" % (B, T, nx),
                        nonneg="noise_var has a negative variance")
        return s0, w

    def _measured(self, measured, meas_var):
        """-> the list of measured state entries (None: the nx / 2 positions) and meas_var [B, ny] on the device, as policy_lqg
        and estimate_states take them: distinct indices in [0, nx); a scalar, [ny] or [B, ny], positive"""
        torch = _torch()
        B, nx = self.B, self.nx
        if measured is None:
            measured = range(nx // 2)
        try:
            m = [int(i) for i in measured]
            whole = all(i == v for i, v in zip(m, measured))
        except (TypeError, ValueError):
            raise ValueError("measured must be a list of state indices")
        if not whole or not 1 <= len(m) <= nx or min(m) < 0 or max(m) >= nx or len(set(m)) != len(m):
            raise ValueError("measured must hold between 1 and nx = %d distinct state indices in [0, %d), not %s" % (nx, nx, list(measured)))
        ny = len(m)
        with torch.cuda.device(self.device):
            r = self._bcast(meas_var, (B, ny), ((), (1,)), None,
                            "meas_var must be a scalar or have shape [ny=%d] or [B=%d, ny], not {}" % (ny, B), say_given=True)
            if r is None:
                raise ValueError("meas_var is required: a scalar, [ny] or [B, ny]")
            if not bool((r > 0).all()):
                raise ValueError("meas_var must be positive")
        return m, r

    def policy_covariance(self, sigma0=None, noise_var=None, keep_cov=False):
        """First-order state and control covariance under the policy in XS / US / KGAIN, u_t = us_t - K_t (x_t - xs_t), by
        one calcDiff sweep and one forward sweep (aslr_policy_covariance, include/aslr_to_amd_cov.h): Sigma_{t+1} =
        A_t Sigma_t A_t^T + diag(noise_var_t) with A_t = Fx_t - Fu_t K_t.  Batch-major arrays or tensors, at least one of
        them: sigma0 [B, nx, nx] or [nx, nx] (symmetric), noise_var [B, T, nx], [B, nx] or [nx] (>= 0; noise t enters
        x_{t+1}); the shorter forms are broadcast.  -> PolicyCovarianceResult.  Side effects: those of calc_diff.  Before
        any backward sweep K = 0 and the result is the open-loop covariance; the control box is not applied."""
        torch = _torch()
        B, T, nx, nu = self.B, self.T, self.nx, self.nu
        with torch.cuda.device(self.device):
            s0, w = self._spread(sigma0, noise_var)
        zeros = self._zeros
        xv, uv, cf, ci = zeros(T + 1, B, nx), zeros(T, B, nu), zeros(B, nx, nx), zeros(B)
        cov = zeros(T + 1, B, nx, nx) if keep_cov else None
        self._call("aslr_policy_covariance", _ptr(s0), _ptr(w), _ptr(xv), _ptr(uv), _ptr(cf), _ptr(cov), _ptr(ci), self._stream())
        torch.cuda.synchronize(self.device)  # (the device copies of the inputs die on return)
        return PolicyCovarianceResult(x_var=xv.permute(1, 0, 2), u_var=self.cut_u(uv.permute(1, 0, 2)), cov_final=cf,
                                      cost_increase=ci, cov=None if cov is None else cov.permute(1, 0, 2, 3))

    def policy_lqg(self, meas_var, measured=None, sigma0=None, noise_var=None, keep_gains=False):
        """First-order state and control covariance under OUTPUT feedback: the policy in XS / US / KGAIN fed the estimate of
        the time-varying Kalman filter for "the state entries `measured` are read at every knot with noise variance
        meas_var", u_t = us_t - K_t eh_t, by one calcDiff sweep and one forward sweep (aslr_policy_lqg,
        include/aslr_to_amd_lqg.h, which gives the recursion).  measured: distinct state indices in any order (None: the
        nx / 2 positions q_l, q_m); meas_var: a scalar, [ny] or [B, ny], > 0, in the order of `measured`; sigma0 and noise_var
        as policy_covariance takes them, at least one of the two.  -> LqgResult.  Side effects: those of calc_diff.  Before any
        backward sweep K = 0: the filter is the same, the loop is open; the control box is not applied."""
        torch = _torch()
        B, T, nx, nu = self.B, self.T, self.nx, self.nu
        m, r = self._measured(measured, meas_var)
        ny = len(m)
        with torch.cuda.device(self.device):
            s0, w = self._spread(sigma0, noise_var)
        zeros = self._zeros
        xv, uv, ev = zeros(T + 1, B, nx), zeros(T, B, nu), zeros(T + 1, B, nx)
        cf, ef, ci = zeros(B, nx, nx), zeros(B, nx, nx), zeros(B)
        kg = zeros(T + 1, B, nx, ny) if keep_gains else None
        self._call("aslr_policy_lqg", ny, (C.c_int32 * ny)(*m), _ptr(r), _ptr(s0), _ptr(w), _ptr(xv), _ptr(uv), _ptr(ev), _ptr(cf),
                   _ptr(ef), _ptr(kg), _ptr(ci), self._stream())
        torch.cuda.synchronize(self.device)  # (the device copies of the inputs die on return)
        return LqgResult(x_var=xv.permute(1, 0, 2), u_var=self.cut_u(uv.permute(1, 0, 2)), est_var=ev.permute(1, 0, 2),
                         cov_final=cf, est_cov_final=ef, cost_increase=ci,
                         kalman_gain=None if kg is None else kg.permute(1, 0, 2, 3), measured=m)

    def estimate_states(self, ys, meas_var, measured=None, x0_mean=None, sigma0=None, noise_var=None, n_iters=5, relax=1.0,
                        keep_filter=False):
        """The states of a recorded run from its measurements: n_iters iterations of the extended Kalman smoother
        (Gauss-Newton on the MAP estimate) about the nominal trajectory in XS with the applied controls in US, all on the
        device in one call (aslr_state_smooth, include/aslr_to_amd_smooth.h, which gives the recursion).  ys [B, T+1, ny]: the
        state entries `measured` at every knot, read with noise of variance meas_var; measured, meas_var, sigma0 and noise_var
        as policy_lqg takes them; x0_mean [B, nx] or [nx]: the prior mean of x_0 (None: XS at knot 0); relax in (0, 1]: the
        part of every step taken.  -> SmoothResult.  Side effects: those of calc_diff, and XS holds the (relaxed) estimate."""
        torch = _torch()
        B, T, nx = self.B, self.T, self.nx
        m, r = self._measured(measured, meas_var)
        ny = len(m)
        n_iters = int(n_iters)
        if n_iters < 1:
            raise ValueError("n_iters must be at least 1")
        with torch.cuda.device(self.device):
            y = self._dev(ys, (B, T + 1, ny), (1, 0, 2), "ys")
            if y is None:
                raise ValueError("ys is required: [B, T+1, ny]")
            s0, w = self._spread(sigma0, noise_var)
            if x0_mean is None:
                x0 = self.region(_abi.R_XS)[0].clone()
            else:
                x0 = self._bcast(x0_mean, (B, nx), ((1,),), None, "x0_mean must have shape [B=%d, nx=%d] or [nx], not {}" % (B, nx))
        zeros = self._zeros
        work = zeros((T + 1) * B * (nx * nx + nx * ny + nx + ny))
        xs, nll, step = zeros(T + 1, B, nx), zeros(n_iters, B), zeros(n_iters, B)
        xf, ev, nis = (zeros(T + 1, B, nx), zeros(T + 1, B, nx), zeros(T + 1, B)) if keep_filter else (None, None, None)
        self._call("aslr_state_smooth", ny, (C.c_int32 * ny)(*m), _ptr(y), _ptr(r), _ptr(x0), _ptr(s0), _ptr(w), n_iters,
                   float(relax), _ptr(work), _ptr(xs), _ptr(xf), _ptr(ev), _ptr(nis), _ptr(nll), _ptr(step), self._stream())
        torch.cuda.synchronize(self.device)  # (the device copies of the inputs and the scratch die on return)
        back = lambda t: None if t is None else t.permute(1, 0, 2)
        return SmoothResult(xs=back(xs), neg_log_lik=nll.permute(1, 0), step_norm=step.permute(1, 0), x_filt=back(xf),
                            est_var=back(ev), nis=None if nis is None else nis.permute(1, 0), measured=m)

    def policy_plant_sensitivity(self, stiffness_var=None, motor_inertia_var=None, keep_trajectories=False):
        """First-order sensitivity of the closed loop under the policy in XS / US / KGAIN, u_t = us_t - K_t (x_t - xs_t), to
        the plant's spring stiffness and motor inertia, by one calcDiff sweep and one forward (tangent) sweep
        (aslr_policy_plant_sensitivity, include/aslr_to_amd_plant_sens.h): S_{t+1} = (Fx_t - Fu_t K_t) S_t + G_t from S_0 = 0,
        S_t = dx_t/dtheta.  stiffness_var, motor_inertia_var: [B, nj] or [nj] variances (>= 0) of independent parameter
        errors; with at least one of them the result carries x_var and u_var.  -> PlantSensitivityResult; the stiffness
        fields are None for a VSA model, which refuses stiffness_var.  Side effects: those of calc_diff.  Before any backward
        sweep K = 0 and dcost_* are what cost_sensitivity returns; the control box is not applied."""
        torch = _torch()
        B, T, nx, nu, nj = self.B, self.T, self.nx, self.nu, self.nx // 4
        vsa = self.low.dam == _abi.DAM_VSA
        if vsa and stiffness_var is not None:
            raise ValueError("stiffness_var on a VSA model, which takes its stiffness from u")

        def var(v, name):
            return self._bcast(v, (B, nj), ((1,),), (1, 0), "%s must have shape [B=%d, nj=%d] or [nj], not {}" % (name, B, nj),
                               nonneg="%s has a negative variance" % name)

        vk, vb = var(stiffness_var, "stiffness_var"), var(motor_inertia_var, "motor_inertia_var")
        zeros = self._zeros
        both = lambda *shape: (None if vsa else zeros(*shape), zeros(*shape))
        (fk, fb), (ck, cb) = both(B, nx, nj), both(nj, B)
        tk, tb = both(T + 1, B, nx, nj) if keep_trajectories else (None, None)
        xv, uv = (zeros(T + 1, B, nx), zeros(T, B, nu)) if (vk is not None or vb is not None) else (None, None)
        self._call("aslr_policy_plant_sensitivity", _ptr(vk), _ptr(vb), _ptr(tk), _ptr(tb), _ptr(fk), _ptr(fb), _ptr(ck), _ptr(cb),
                   _ptr(xv), _ptr(uv), self._stream())
        torch.cuda.synchronize(self.device)  # (the device copies of the inputs die on return)
        bm = lambda t, *perm: None if t is None else t.permute(*perm)
        return PlantSensitivityResult(dx_final_dstiffness=fk, dx_final_dmotor_inertia=fb, dcost_dstiffness=bm(ck, 1, 0),
                                      dcost_dmotor_inertia=bm(cb, 1, 0), x_var=bm(xv, 1, 0, 2),
                                      u_var=None if uv is None else self.cut_u(uv.permute(1, 0, 2)),
                                      dxs_dstiffness=bm(tk, 1, 0, 2, 3), dxs_dmotor_inertia=bm(tb, 1, 0, 2, 3))

    # ---- per-iteration log, frame placements, residuals ----
    def enable_iteration_log(self, capacity):
        """Device-resident log of the per-iteration solver state ([capacity, LOG_COUNT, B], NaN = not written): the
        line-search kernel fills it, nothing crosses PCIe until `iteration_log()` is read.  capacity 0 / None: off."""
        torch = _torch()
        if not capacity:
            self._log = None
            self._call("aslr_set_iteration_log", C.c_void_p(0), 0)
            return None
        with torch.cuda.device(self.device):
            self._log = torch.full((int(capacity), _abi.LOG_COUNT, self.B), float("nan"), dtype=torch.float64,
                                   device=self.device)
        self._call("aslr_set_iteration_log", C.c_void_p(self._log.data_ptr()), int(capacity))
        return self._log

    def iteration_log(self):
        """The log tensor ([capacity, LOG_COUNT, B], on the device), or None when logging is off."""
        return getattr(self, "_log", None)

    def frame_placement(self, frame_joint, frame_R, frame_p, x, x_stride=None):
        """World placements of a frame (joint index + local placement) at the link positions of `x`
        (a device tensor [..., >= nj], contiguous): -> ([..., 3, 3], [..., 3]) device tensors."""
        torch = _torch()
        x = x.contiguous()
        stride = x.shape[-1] if x_stride is None else int(x_stride)
        n = x.numel() // x.shape[-1]
        out = torch.empty((n, 12), dtype=torch.float64, device=self.device)
        R = (C.c_double * 9)(*[float(v) for v in np.asarray(frame_R, dtype=np.float64).reshape(9)])
        pv = (C.c_double * 3)(*[float(v) for v in np.asarray(frame_p, dtype=np.float64).reshape(3)])
        self._call("aslr_frame_placement", int(frame_joint), R, pv, n, C.c_void_p(x.data_ptr()), stride,
                   C.c_void_p(out.data_ptr()), self._stream())
        lead = tuple(x.shape[:-1])
        return out[:, :9].reshape(lead + (3, 3)), out[:, 9:].reshape(lead + (3,))

    def dam_residuals(self, model_index, x, u):
        """Stacked cost residuals (data.r) of n points, in the order of the model's cost list: numpy [n, nr]."""
        torch = _torch()
        x = np.atleast_2d(np.asarray(x, dtype=np.float64))
        u = self.pad_u(np.atleast_2d(np.asarray(u, dtype=np.float64)))
        nr = self.lib.aslr_residual_len(C.byref(self.low.desc.models[model_index]), self.nx // 4)
        if nr < 0:
            raise _abi.AslrError("aslr_residual_len failed")
        dx = torch.as_tensor(x, device=self.device).contiguous()
        du = torch.as_tensor(u, device=self.device).contiguous()
        r = torch.zeros((x.shape[0], max(nr, 1)), dtype=torch.float64, device=self.device)
        if nr > 0:
            self._call("aslr_dam_residuals", model_index, x.shape[0], C.c_void_p(dx.data_ptr()),
                       C.c_void_p(du.data_ptr()), C.c_void_p(r.data_ptr()), self._stream())
        return r[:, :nr].cpu().numpy()

    def solve_pool(self, x0s, frame_refs, sp, refill_every=4, poll_every=16, xs_init=None, us_init=None, stiffness=None,
                   motor_inertia=None, u_lb=None, u_ub=None):
        """A pool of P problems of this engine's structure solved through its B slots, each to its own convergence
        (aslr_solve_pool: stopped slots are flushed and refilled on the device; every problem is cold-started).
        x0s [P, nx], frame_refs [P, 12] or None, xs_init [P, T+1, nx] / us_init [P, T, nu] or None = zeros (host or
        device).  -> dict of device tensors: xs [P, T+1, nx],
        us [P, T, nu], cost / stop / x_reg / step [P], iters / status [P] (int32), and batch_iters (int).
        stiffness / motor_inertia [P, nj], u_lb / u_ub [P, nu] (or the models' own narrower nu, padded as lower_traj_params
        says), host arrays, each optional: problem j is solved with row j of every given field, a field left out keeps the
        models' constant (aslr_solve_pool_params: a design sweep through the pool).  With all four None the call is
        aslr_solve_pool as before; otherwise the result also holds params, the lowered table [2 nj + 2 nu, P] on the device."""
        torch = _torch()
        with torch.cuda.device(self.device):
            x0 = self._f64(x0s)
            P = x0.shape[0]
            x0 = self._dev(x0, (P, self.nx), None, "x0s", "x0s must have shape [P, nx=%d]" % self.nx)
            fr = self._dev(frame_refs, (P, 12), None, "frame_refs", "frame_refs must have shape [P, 12]")
            xi = self._dev(xs_init, (P, self.T + 1, self.nx), None, "xs_init", "xs_init must have shape [P, T+1, nx]")
            ui = self._dev(None if us_init is None else self.pad_u(self._f64(us_init)), (P, self.T, self.nu), None, "us_init",
                           "us_init must have shape [P, T, nu]")
            xs = torch.empty((P, self.T + 1, self.nx), dtype=torch.float64, device=self.device)
            us = torch.empty((P, self.T, self.nu), dtype=torch.float64, device=self.device)
            sf = torch.zeros((P, 4), dtype=torch.float64, device=self.device)
            si = torch.zeros((P, 2), dtype=torch.int32, device=self.device)
            slot = torch.empty((self.B,), dtype=torch.int32, device=self.device)
            cnt = torch.zeros((2,), dtype=torch.int32, device=self.device)
        pool = _abi.Pool()
        pool.P = P
        pool.x0, pool.frame_ref = x0.data_ptr(), (fr.data_ptr() if fr is not None else None)
        pool.xs_out, pool.us_out, pool.stat_f, pool.stat_i = xs.data_ptr(), us.data_ptr(), sf.data_ptr(), si.data_ptr()
        pool.slot_problem, pool.counters = slot.data_ptr(), cnt.data_ptr()
        pool.xs_init = xi.data_ptr() if xi is not None else None
        pool.us_init = ui.data_ptr() if ui is not None else None
        it = C.c_int32(0)
        low = self.low
        tp = lower_traj_params(low.desc, low.nj, low.nu, self.nu_user, low.dam, stiffness, motor_inertia, u_lb, u_ub, rows=P)
        more = {}
        if tp is not None:
            with torch.cuda.device(self.device):
                params = torch.empty((2 * low.nj + 2 * low.nu, P), dtype=torch.float64, device=self.device)
            pp = _abi.PoolParams()
            for name, a in tp.items():
                setattr(pp, name, a.ctypes.data_as(C.POINTER(C.c_double)))
            pp.params_dev = params.data_ptr()
            self._call("aslr_solve_pool_params", C.byref(sp), C.byref(pool), C.byref(pp), int(refill_every), int(poll_every),
                       self._stream(), C.byref(it))
            more = dict(params=params)
        else:
            self._call("aslr_solve_pool", C.byref(sp), C.byref(pool), int(refill_every), int(poll_every), self._stream(),
                       C.byref(it))
        torch.cuda.synchronize(self.device)
        return dict(xs=xs, us=self.cut_u(us), cost=sf[:, 0], stop=sf[:, 1], x_reg=sf[:, 2], step=sf[:, 3], iters=si[:, 0],
                    status=si[:, 1], batch_iters=it.value, **more)

    def mpc_run(self, sp, n_steps, first_maxiter, iters_per_step, disturbance=None):
        """A receding-horizon run on the device (aslr_mpc_run): step 0 solves first_maxiter iterations from the candidate
        as it was set, every later step iters_per_step from the shifted plan; between two solves the first control is
        applied to the plant (node 0's model, the trajectory's parameters), `disturbance` [B, n_steps, nx] (host or
        device, optional) is added to its next state and the plan moves one knot down.  One ABI call, no host round
        trip per step.  With a reference path set the window slides along it, one row per step, and the handle's
        reference_row has grown by n_steps afterwards.  -> MpcResult; XS / US are left with the last shifted plan, X0 with
        the last plant state."""
        torch = _torch()
        n = int(n_steps)
        with torch.cuda.device(self.device):
            dist = self._dev(disturbance, (self.B, n, self.nx), (1, 0, 2), "disturbance",
                             "disturbance must have shape [B=%d, n_steps=%d, nx=%d]" % (self.B, n, self.nx))
        mpc, bufs = self._mpc_block(n, max(n, 0), first_maxiter, iters_per_step, dist)
        self._call("aslr_mpc_run", C.byref(sp), C.byref(mpc), self._stream())
        torch.cuda.synchronize(self.device)  # (the time-major disturbance copy dies on return)
        return self._mpc_result(bufs)

    def _mpc_block(self, n, N, first_maxiter, iters_per_step, dist):
        """The aslr_mpc_t of a run of n control steps that apply N knots in all, and the four zeroed time-major buffers it
        points to (x_closed, u_closed, stat_f, stat_i); dist: the time-major disturbance, or None."""
        m, zeros = max(n, 0), self._zeros
        xc, uc = zeros(N + 1, self.B, self.nx), zeros(N, self.B, self.nu)
        sf, si = zeros(m, 4, self.B), zeros(m, 2, self.B, dtype=_torch().int32)
        mpc = _abi.Mpc()
        mpc.n_steps, mpc.first_maxiter, mpc.iters_per_step = n, int(first_maxiter), int(iters_per_step)
        mpc.disturbance = dist.data_ptr() if dist is not None else None
        mpc.x_closed, mpc.u_closed, mpc.stat_f, mpc.stat_i = xc.data_ptr(), uc.data_ptr(), sf.data_ptr(), si.data_ptr()
        return mpc, (xc, uc, sf, si)

    def _mpc_result(self, bufs, **more):
        """The MpcResult of the buffers _mpc_block made, once the run is complete; more: the fields of mpc_run_plant."""
        xc, uc, sf, si = bufs
        return MpcResult(xs_closed=xc.permute(1, 0, 2), us_closed=self.cut_u(uc.permute(1, 0, 2)), iters=si[:, 0].t(),
                         status=si[:, 1].t(), cost=sf[:, 0].t(), stop=sf[:, 1].t(), x_reg=sf[:, 2].t(), step=sf[:, 3].t(),
                         reference_row=self.reference_row, **more)

    def mpc_run_plant(self, sp, n_steps, first_maxiter, iters_per_step, hold=1, plant_stiffness=None, plant_motor_inertia=None,
                      disturbance=None, clamp=False, closed_cost=True):
        """mpc_run on a plant of its own (aslr_mpc_run_plant, include/aslr_to_amd_mpc_plant.h; on the 7-joint arms
        aslr_mpc_run_plant_all, include/aslr_to_amd_mpc_plant_all.h): every control step solves
        as mpc_run does, then applies `hold` knots of the plan to the plant -- the first control as it is, the later ones
        with the Riccati feedback u = us_j - K_j (x - xs_j) -- and shifts the plan by hold.  Batch-major arrays or tensors,
        each optional: plant_stiffness, plant_motor_inertia [B, nj] (diagonals of the plant's K and B; None: the
        trajectory's own), disturbance [B, N, nx] with N = n_steps * hold (added to the next state of every applied knot).
        clamp: clamp the applied control to the box.  -> MpcResult with xs_closed [B, N+1, nx], us_closed [B, N, nu_user], the
        per-step fields of mpc_run, closed_cost [B] (the running costs of the applied knots, NaN for a failed trajectory;
        None with closed_cost=False), failed_knot [B] and hold.  A non-positive plant inertia is not checked (it lives on
        the device) and shows up in failed_knot."""
        torch = _torch()
        n, h, nj = int(n_steps), int(hold), self.nx // 4
        N = max(n, 0) * max(h, 0)
        with torch.cuda.device(self.device):
            pk = self._dev(plant_stiffness, (self.B, nj), (1, 0), "plant_stiffness")
            pb = self._dev(plant_motor_inertia, (self.B, nj), (1, 0), "plant_motor_inertia")
            dist = self._dev(disturbance, (self.B, N, self.nx), (1, 0, 2), "disturbance")
            cc = self._zeros(self.B) if closed_cost else None
            fk = torch.full((self.B,), -1, dtype=torch.int32, device=self.device)
        mpc, bufs = self._mpc_block(n, N, first_maxiter, iters_per_step, dist)
        # (2 joints: the entry point that has always served them; every other size: the one that serves all sizes)
        self._call("aslr_mpc_run_plant" if nj == 2 else "aslr_mpc_run_plant_all", C.byref(sp), C.byref(mpc), h, _ptr(pk), _ptr(pb),
                   1 if clamp else 0, _ptr(cc), _ptr(fk), self._stream())
        torch.cuda.synchronize(self.device)  # (the time-major copies of the inputs die on return)
        return self._mpc_result(bufs, closed_cost=cc, failed_knot=fk, hold=h)

    def design_descent(self, sp, n_steps, first_maxiter, iters_per_step, stiffness_bounds=None, motor_inertia_bounds=None,
                       eta0=0.05, grow=2.0, shrink=0.5, c1=1e-4, max_rel=0.25, keep_history=False):
        """A descent in every trajectory's own spring stiffness and motor inertia on the device (aslr_design_descent,
        include/aslr_to_amd_design.h): per step a solve from the candidate in XS / US (first_maxiter iterations in step 0,
        iters_per_step later), the gradient of cost_sensitivity, an Armijo test against the accepted design and the next
        candidate, a bounded step in log theta.  One ABI call, no host round trip per step.  stiffness_bounds,
        motor_inertia_bounds: (lo, hi), each [B, nj], [nj] or a scalar; a field whose bounds are None is not optimised.
        The initial design is the parameter table if one is set, the models' constants otherwise.  -> DesignResult; XS /
        US and the parameter table are left on the accepted design."""
        torch = _torch()
        B, T, nx, nu, nj = self.B, self.T, self.nx, self.nu, self.nx // 4
        n = int(n_steps)
        m = max(n, 0)

        lo, hi = self._bounds(((stiffness_bounds, "stiffness_bounds"), (motor_inertia_bounds, "motor_inertia_bounds")), ones=True)
        zeros = self._zeros
        theta, cost, xb, ub = zeros(2 * nj, B), zeros(B), zeros(T + 1, B, nx), zeros(T, B, nu)
        gacc, eta, grad = zeros(2 * nj, B), zeros(B), zeros(2 * nj, B)
        hf = zeros(m, 3, B) if keep_history else None
        hi_ = zeros(m, B, dtype=torch.int32) if keep_history else None
        th = zeros(m, 2 * nj, B) if keep_history else None
        d = _abi.Design()
        d.n_steps, d.first_maxiter, d.iters_per_step = n, int(first_maxiter), int(iters_per_step)
        d.opt_stiffness, d.opt_motor_inertia = int(stiffness_bounds is not None), int(motor_inertia_bounds is not None)
        d.eta0, d.grow, d.shrink, d.c1, d.max_rel = float(eta0), float(grow), float(shrink), float(c1), float(max_rel)
        d.lo, d.hi = _ptr(lo), _ptr(hi)
        d.theta_best, d.cost_best, d.xs_best, d.us_best = _ptr(theta), _ptr(cost), _ptr(xb), _ptr(ub)
        d.hist_f, d.hist_i, d.theta_hist = _ptr(hf), _ptr(hi_), _ptr(th)
        d.g_acc, d.eta, d.grad = _ptr(gacc), _ptr(eta), _ptr(grad)
        self._call("aslr_design_descent", C.byref(sp), C.byref(d), self._stream())
        torch.cuda.synchronize(self.device)  # (the scratch tensors die on return)
        vsa = self.low.dam == _abi.DAM_VSA
        hist = {}
        if keep_history:
            hist = dict(cost_history=hf[:, 0].t(), eta_history=hf[:, 1].t(), predicted_history=hf[:, 2].t(),
                        accepted_history=hi_.t(), stiffness_history=None if vsa else th[:, :nj].permute(2, 0, 1),
                        motor_inertia_history=th[:, nj:].permute(2, 0, 1))
        return DesignResult(stiffness=None if vsa else theta[:nj].t(), motor_inertia=theta[nj:].t(), cost=cost,
                            xs=xb.permute(1, 0, 2), us=self.cut_u(ub.permute(1, 0, 2)), **hist)

    def plant_identify(self, n_steps, weights=None, stiffness_bounds=None, motor_inertia_bounds=None, mu0=1e-3, mu_min=1e-12,
                       mu_max=1e12, grow=10.0, shrink=0.1, max_rel=0.5, min_curv=1e-12, keep_history=False):
        """Fit every trajectory's own spring stiffness and motor inertia to the recorded run in XS / US on the device
        (aslr_plant_identify, include/aslr_to_amd_identify.h): n_steps Levenberg-Marquardt steps on the one-step prediction
        error, one ABI call, no host round trip per step.  weights: [B, nx], [nx] or None (ones).  stiffness_bounds,
        motor_inertia_bounds: (lo, hi), each [B, nj], [nj] or a scalar; a field whose bounds are None is not fitted.  The
        initial parameters are the parameter table if one is set, the models' constants otherwise.  -> IdentifyResult; the
        parameter table is left on the fit, XS / US are not written."""
        torch = _torch()
        B, nx, nj = self.B, self.nx, self.nx // 4
        n = int(n_steps)
        m = max(n, 0)
        fit_k, fit_b = stiffness_bounds is not None, motor_inertia_bounds is not None
        npar = (int(fit_k) + int(fit_b)) * nj
        nh = npar * (npar + 1) // 2

        zeros, i32 = self._zeros, torch.int32
        lo, hi = self._bounds(((stiffness_bounds, "stiffness_bounds"), (motor_inertia_bounds, "motor_inertia_bounds")), ones=False)
        if lo is None:
            lo, hi = zeros(1), zeros(1)
        w = self._bcast(weights, (B, nx), ((1,),), (1, 0), "weights must have shape [B=%d, nx=%d] or [nx], not {}" % (B, nx))
        r = max(npar, 1)
        theta, sse, grad, info, mu = zeros(r, B), zeros(B), zeros(r, B), zeros(max(nh, 1), B), zeros(B)
        ident, nacc = zeros(r, B, dtype=i32), zeros(B, dtype=i32)
        work = zeros(2 * r + 1 + max(nh, 1), B)
        ht = zeros(m, r, B) if keep_history else None
        hs = zeros(m, B) if keep_history else None
        hd = zeros(m, B, dtype=i32) if keep_history else None
        d = _abi.Identify()
        d.n_steps, d.fit_stiffness, d.fit_motor_inertia = n, int(fit_k), int(fit_b)
        d.mu0, d.mu_min, d.mu_max, d.grow, d.shrink = float(mu0), float(mu_min), float(mu_max), float(grow), float(shrink)
        d.max_rel, d.min_curv = float(max_rel), float(min_curv)
        d.weights, d.lo, d.hi = _ptr(w), _ptr(lo), _ptr(hi)
        d.theta, d.sse, d.grad, d.information, d.mu = _ptr(theta), _ptr(sse), _ptr(grad), _ptr(info), _ptr(mu)
        d.identifiable, d.n_accepted, d.work = _ptr(ident), _ptr(nacc), _ptr(work)
        d.hist_theta, d.hist_sse, d.hist_decision = _ptr(ht), _ptr(hs), _ptr(hd)
        self._call("aslr_plant_identify", C.byref(d), self._stream())
        torch.cuda.synchronize(self.device)  # (the scratch tensors die on return)
        # the fitted fields from theta, the others from the table (reciprocal motor rows)
        table = self._traj_table()
        vsa = self.low.dam == _abi.DAM_VSA
        k0 = nj if fit_k else 0
        stiffness = None if vsa else (theta[:nj] if fit_k else table[:nj]).t().clone()
        motor = (theta[k0:k0 + nj].t() if fit_b else (1.0 / table[nj:2 * nj]).t()).clone()
        full = zeros(B, npar, npar)
        pi, qi = (torch.as_tensor(v, device=self.device) for v in np.tril_indices(npar))
        full[:, pi, qi] = info[:nh].t()
        full[:, qi, pi] = info[:nh].t()
        hist = {}
        if keep_history:
            hist = dict(theta_history=ht.permute(2, 0, 1), sse_history=hs.t(), decision_history=hd.t())
        return IdentifyResult(stiffness=stiffness, motor_inertia=motor, theta=theta.t(), sse=sse, n_accepted=nacc, grad=grad.t(),
                              information=full, identifiable=ident.t() != 0, mu=mu, **hist)

    def traj_f(self, row):
        return self.region(_abi.R_TRAJ_F)[row]

    def traj_i(self, row):
        return self.region(_abi.R_TRAJ_I)[row]

    def dam_eval(self, model_index, x, u):
        """DAM-level calc + calcDiff on n points (numpy in / numpy out)."""
        torch = _torch()
        x = np.atleast_2d(np.asarray(x, dtype=np.float64))
        u = self.pad_u(np.atleast_2d(np.asarray(u, dtype=np.float64)))
        n, nx, nu, nv = x.shape[0], self.nx, self.nu, self.nx // 2
        dx = torch.as_tensor(x, device=self.device).contiguous()
        du = torch.as_tensor(u, device=self.device).contiguous()
        outs = {"xout": (n, nv), "cost": (n,), "Fx": (n, nv, nx), "Fu": (n, nv, nu), "Lx": (n, nx), "Lu": (n, nu),
                "Lxx": (n, nx, nx), "Lxu": (n, nx, nu), "Luu": (n, nu, nu)}
        t = {k: torch.empty(s, dtype=torch.float64, device=self.device) for k, s in outs.items()}
        p = lambda k: C.c_void_p(t[k].data_ptr())
        self._call("aslr_dam_eval", model_index, n, C.c_void_p(dx.data_ptr()), C.c_void_p(du.data_ptr()), p("xout"),
                   p("cost"), p("Fx"), p("Fu"), p("Lx"), p("Lu"), p("Lxx"), p("Lxu"), p("Luu"), self._stream())
        out = {k: v.cpu().numpy() for k, v in t.items()}
        if self.nu_user != self.nu:
            out["Fu"], out["Lu"], out["Lxu"] = self.cut_u(out["Fu"]), self.cut_u(out["Lu"]), self.cut_u(out["Lxu"])
            out["Luu"] = self.cut_u(self.cut_u(out["Luu"]), axis=-2)
        return out


class _PointEvaluator(object):
    """B = 1, T = 1 problem around one action model: backs `model.calc(data, x, u)`."""

    def __init__(self, model):
        from .models import IntegratedActionModelEulerASR
        if isinstance(model, IntegratedActionModelEulerASR):
            self.iam = model
        else:
            self.iam = IntegratedActionModelEulerASR(model, 0.0)
        self._sig = None
        self.engine = None

    def _ensure(self):
        # re-lower when the user mutated the model (weights, bounds, dt ...) since the last call
        low = lower_problem(np.zeros(self.iam.state.nx), [self.iam], self.iam)
        sig = bytes(memoryview(low.desc.models[0])) + bytes(memoryview(low.desc.chain))
        if sig != self._sig:
            if self.engine is not None:
                self.engine.close()
            self.engine = Engine(low)
            self._sig = sig
        return self.engine

    def dam(self, data, x, u, diff):
        e = self._ensure()
        r = e.dam_eval(0, x, u)
        data.xout[:] = r["xout"][0]
        data.cost = float(r["cost"][0])
        self._side_data(data, x, u)
        if diff:
            for k in ("Fx", "Fu", "Lx", "Lu", "Lxx", "Lxu", "Luu"):
                getattr(data, k)[...] = r[k][0]

    def _side_data(self, ddata, x, u):
        """data.r (the stacked cost residuals, costs.shareMemory: free_fwddyn_asr.py:128-129) and
        data.multibody.pinocchio.oMf of the frames the model knows, from the GPU."""
        e = self.engine
        dam = self.iam.differential
        r = e.dam_residuals(0, x, u)[0]
        ddata.r = dam.costs.order_residuals(r, dam.state.ndx, dam.nu, dam.nu_dev)
        ddata.multibody.pinocchio.oMf = _FrameMap(e, dam.state.pinocchio, np.asarray(x, dtype=np.float64))

    def integrated(self, data, x, u, diff):
        torch = _torch()
        e = self._ensure()
        x = np.asarray(x, dtype=np.float64)
        if u is None:
            u = self.iam.differential._default_u()
        xs = np.stack([x, x])[None]
        e.set_candidate(xs, np.asarray(u, dtype=np.float64)[None, None])
        (e.calc_diff if diff else e.calc)()
        torch.cuda.synchronize(e.device)
        data.xnext[:] = e.region(_abi.R_XNEXT)[0, 0].cpu().numpy()
        data.cost = float(e.region(_abi.R_COST)[0, 0].item())
        data.dx[:] = data.xnext - x
        self._side_data(data.differential, x, u)
        data.differential.cost = data.cost
        if self.iam.withCostResiduals:
            data.r = data.differential.r  # integrated_action.py:17-18
        if diff:
            for k in ("Fx", "Fu", "Lx", "Lu", "Lxx", "Lxu", "Luu"):
                blk = e.deriv_block(k)[0, 0].cpu().numpy()
                if k in ("Fu", "Lu", "Lxu", "Luu"):
                    blk = e.cut_u(blk)
                if k == "Luu":
                    blk = e.cut_u(blk, axis=-2)
                getattr(data, k)[...] = blk


class _SE3View(object):
    """What the scripts read from pinocchio.SE3: .rotation, .translation (numpy)."""

    def __init__(self, R, p):
        self.rotation, self.translation = R, p

    def __repr__(self):
        return "SE3(R=%r, p=%r)" % (self.rotation, self.translation)


class _FrameMap(object):
    """data.pinocchio.oMf: frame id -> placement, evaluated on the GPU (aslr_frame_placement) on first access."""

    def __init__(self, engine, pin_model, x):
        self._e, self._m, self._x, self._cache = engine, pin_model, x, {}

    def __getitem__(self, fid):
        if fid not in self._cache:
            torch = _torch()
            fr = self._m.frames[fid]
            if fr.parent < 0:  # a frame of the universe does not move
                self._cache[fid] = _SE3View(fr.placement.rotation.copy(), fr.placement.translation.copy())
                return self._cache[fid]
            xt = torch.as_tensor(self._x, dtype=torch.float64, device=self._e.device).reshape(1, -1)
            R, p = self._e.frame_placement(fr.parent, fr.placement.rotation, fr.placement.translation, xt)
            self._cache[fid] = _SE3View(R[0].cpu().numpy(), p[0].cpu().numpy())
        return self._cache[fid]

    def __len__(self):
        return len(self._m.frames)


def point_evaluator(model):
    if getattr(model, "_evaluator", None) is None:
        model._evaluator = _PointEvaluator(model)
    return model._evaluator
