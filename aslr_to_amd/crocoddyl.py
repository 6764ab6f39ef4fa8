"""The slice of Crocoddyl's Python API that aslr_to's scripts touch, re-hosted on
the MI355X engine: ShootingProblem, SolverDDP / SolverFDDP / SolverBoxDDP, the cost / activation /
residual descriptors and the two callbacks.  Use as

    from aslr_to_amd import crocoddyl

A problem is a *batch* of B shooting problems sharing structure (same robot, same cost types) with
per-trajectory x0 and, optionally, per-trajectory frame-placement targets; `ShootingProblem(x0,
runningModels, terminalModel)` is the B = 1 case and behaves like the single-problem API
(lists of numpy arrays in `solver.xs`, `solver.us`).
"""
import math
import sys

import numpy as np

from . import _abi
from .lowering import lower_problem, lower_reference_path, lower_traj_params, shard_rows
from .models import (ActivationModelQuad, ActivationModelWeightedQuad, CostModelResidual,  # noqa: F401
                     CostModelSum, Jcomponent, ResidualModelControl, ResidualModelState)


class _NodePinocchio(object):
    """data.differential.multibody.pinocchio of a node: oMf[frame_id] from the GPU (aslr_frame_placement at the
    node's link positions XS[t]), what the scripts print after a solve (examples/two_dof_sea.py:82-86,
    examples/two_dof_vsa_boxddp.py:83-84).  B = 1: an object with .rotation / .translation; a batch: the same with a
    leading batch dimension (device tensors)."""

    def __init__(self, node):
        self._node = node

    @property
    def oMf(self):
        return _NodeFrames(self._node)


class _NodeFrames(object):
    def __init__(self, node):
        self._node = node

    def __getitem__(self, fid):
        from .engine import _SE3View
        p, t = self._node._p, self._node._t
        e = p.engine
        model = p.runningModels[0].state.pinocchio if p.runningModels else p.terminalModel.state.pinocchio
        fr = model.frames[fid]
        if fr.parent < 0:
            return _SE3View(fr.placement.rotation.copy(), fr.placement.translation.copy())
        x = e.region(_abi.R_XS)[t]  # [B, nx], contiguous
        R, pos = e.frame_placement(fr.parent, fr.placement.rotation, fr.placement.translation, x)
        if p.batch == 1:
            return _SE3View(R[0].cpu().numpy(), pos[0].cpu().numpy())
        return _SE3View(R, pos)

    def __len__(self):
        p = self._node._p
        model = p.runningModels[0].state.pinocchio if p.runningModels else p.terminalModel.state.pinocchio
        return len(model.frames)


class _NodeMultibody(object):
    def __init__(self, node):
        self.pinocchio = _NodePinocchio(node)


class _NodeData(object):
    """runningDatas[t] / terminalData: views of the engine's per-node results."""

    def __init__(self, problem, t):
        self._p, self._t = problem, t
        self.differential = self
        self.multibody = _NodeMultibody(self)
        self.pinocchio = self.multibody.pinocchio

    def _blk(self, name):
        e = self._p.engine
        blk = e.deriv_block(name)[self._t, 0].cpu().numpy()
        if name in ("Fu", "Lu", "Lxu", "Luu"):
            blk = e.cut_u(blk)
        return e.cut_u(blk, axis=-2) if name == "Luu" else blk

    @property
    def r(self):
        """data.r: the stacked cost residuals of this node (integrated_action.py:17-18), trajectory 0."""
        p, t = self._p, self._t
        e = p.engine
        model = p.runningModels[t] if t < p.T else p.terminalModel
        x = e.region(_abi.R_XS)[t, 0].cpu().numpy()
        u = e.region(_abi.R_US)[t, 0].cpu().numpy() if t < p.T else model.differential._default_u()
        mi = int(p.lowered.node_model[t])
        dam = model.differential
        return dam.costs.order_residuals(e.dam_residuals(mi, x, u)[0], dam.state.ndx, dam.nu, dam.nu_dev)

    xnext = property(lambda s: s._p.engine.region(_abi.R_XNEXT)[s._t, 0].cpu().numpy())
    cost = property(lambda s: float(s._p.engine.region(_abi.R_COST)[s._t, 0].item()))
    Fx = property(lambda s: s._blk("Fx"))
    Fu = property(lambda s: s._blk("Fu"))
    Lx = property(lambda s: s._blk("Lx"))
    Lu = property(lambda s: s._blk("Lu"))
    Lxx = property(lambda s: s._blk("Lxx"))
    Lxu = property(lambda s: s._blk("Lxu"))
    Luu = property(lambda s: s._blk("Luu"))


class _DataList(list):
    def tolist(self):
        return list(self)


class ShootingProblem(object):
    """crocoddyl.ShootingProblem(x0, runningModels, terminalModel) (examples/two_dof_sea.py:66).

    Batched form: `ShootingProblem(x0s[B, nx], runningModels, terminalModel, frame_refs=...)`.
    With `rank`/`world_size` the batch is sharded in contiguous blocks, one shard per GPU
    (SURVEY.md 8(e)); every trajectory is solved independently, so results do not depend on the
    sharding.  `stiffness` / `motor_inertia` ([B, nj]) and `u_lb` / `u_ub` ([B, nu]) give every trajectory its own
    diagonal K and B and its own control box (a design sweep in one batch); sharded like x0s and frame_refs.
    `frame_ref_path` ([B, N, 12] or B lists of N SE3) gives every trajectory a reference placement per knot: knot t tracks
    row min(reference_row + t, N - 1) with every frame-placement cost (set_reference_path; solve_mpc slides along it).
    """

    def __init__(self, x0, runningModels, terminalModel, frame_refs=None, rank=0, world_size=1, device=None,
                 stiffness=None, motor_inertia=None, u_lb=None, u_ub=None, frame_ref_path=None):
        x0 = np.atleast_2d(np.asarray(x0, dtype=np.float64))
        self._x0_all = x0
        self.batch_total = x0.shape[0]
        self.rank, self.world_size = rank, world_size
        lo, hi = shard_rows(self.batch_total, rank, world_size)
        self.rows = (lo, hi)
        self.runningModels = list(runningModels)
        self.terminalModel = terminalModel
        self.T = len(self.runningModels)
        self.nthreads = 1
        fr = None if frame_refs is None else list(frame_refs)[lo:hi]
        tp = self._shard_params(stiffness, motor_inertia, u_lb, u_ub)
        self._lowered = lower_problem(x0[lo:hi], self.runningModels, terminalModel, fr, **tp)
        self.batch = hi - lo
        self.nx, self.nu = self._lowered.nx, self._lowered.nu_user
        self._device = device
        self._engine = None
        if frame_ref_path is not None:
            self.set_reference_path(frame_ref_path)

    def set_reference_path(self, path=None, row0=0):
        """Set (whole-batch [B, N, 12] array or B lists of N SE3), reposition or clear (None) the time-varying reference
        placements between solves; knot t then tracks row min(row0 + t, N - 1)."""
        low = self._lowered
        if path is None:
            low.ref_path = None
        else:
            if len(path) != self.batch_total:
                raise ValueError("frame_ref_path must have shape [B=%d, n_rows, 12], got %d paths" % (self.batch_total, len(path)))
            lo, hi = self.rows
            low.ref_path = (lower_reference_path(low.desc, path[lo:hi], row0), int(row0))
        if self._engine is not None:
            self._engine.upload_reference_path(*(low.ref_path or (None, 0)))

    @property
    def reference_row(self):
        """the path row knot 0 tracks: row0 of set_reference_path plus the control steps of every solve_mpc since"""
        if self._engine is not None:
            return self._engine.reference_row
        return 0 if self._lowered.ref_path is None else self._lowered.ref_path[1]

    def _shard(self, v, ndim=None, pair=False):
        """This rank's rows of v where v is a whole-batch array: one of `ndim` dimensions with a row per trajectory (ndim
        None: any array).  Anything else, and None, passes through for the engine to judge.  pair: v is (lo, hi), and
        each entry is cut."""
        if pair:
            return v if v is None or len(v) != 2 else tuple(self._shard(e, ndim) for e in v)
        whole = v is not None and (ndim is None or (np.ndim(v) == ndim and len(v) == self.batch_total))
        return v[self.rows[0]:self.rows[1]] if whole else v

    def _shard_params(self, stiffness, motor_inertia, u_lb, u_ub):
        """rows of this rank out of whole-batch parameter arrays"""
        out = {}
        for name, v in (("stiffness", stiffness), ("motor_inertia", motor_inertia), ("u_lb", u_lb), ("u_ub", u_ub)):
            if v is not None:
                v = np.array(v, dtype=np.float64, ndmin=2)
                if v.shape[0] != self.batch_total:
                    raise ValueError("%s needs one row per trajectory (%d), got %d" % (name, self.batch_total, v.shape[0]))
            out[name] = self._shard(v)
        return out

    def _follow_table(self, r):
        """the problem's own record of the parameter table follows the engine's, which a design descent or an identification
        left on r.stiffness / r.motor_inertia (a later engine of this problem starts from it)"""
        low = self._lowered
        old = low.traj_params or {}
        low.traj_params = lower_traj_params(low.desc, low.nj, low.nu, low.nu_user, low.dam,
                                            None if r.stiffness is None else r.stiffness.cpu().numpy(),
                                            r.motor_inertia.cpu().numpy(), old.get("u_lb"), old.get("u_ub"))

    def set_trajectory_params(self, stiffness=None, motor_inertia=None, u_lb=None, u_ub=None):
        """Replace the per-trajectory parameter table between solves (whole-batch arrays, as in the constructor; all
        None: back to the models' constants)."""
        tp = self._shard_params(stiffness, motor_inertia, u_lb, u_ub)
        low = self._lowered
        low.traj_params = lower_traj_params(low.desc, low.nj, low.nu, low.nu_user, low.dam, **tp)
        if self._engine is not None:
            self._engine.upload_traj_params(low.traj_params)

    @property
    def x0(self):
        return self._x0_all[self.rows[0]] if self.batch == 1 else self._x0_all[self.rows[0]:self.rows[1]]

    @property
    def lowered(self):
        return self._lowered

    @property
    def engine(self):
        if self._engine is None:
            from .engine import Engine
            self._engine = Engine(self._lowered, self._device)
        return self._engine

    # -- Crocoddyl API --
    def calc(self, xs, us):
        e = self.engine
        e.set_candidate(xs, us)
        e.calc()
        return self._total_cost()

    def calcDiff(self, xs, us):
        e = self.engine
        e.set_candidate(xs, us)
        e.calc_diff()
        return self._total_cost()

    def cost_sensitivity(self, xs=None, us=None):
        """Gradients of every trajectory's cost, controls held fixed, in its own spring stiffness, motor inertia and
        initial state (engine.SensitivityResult: stiffness [B, nj] -- None for VSA --, motor_inertia [B, nj], x0 [B, nx],
        costate [B, T+1, nx]) at the candidate (xs, us); neither given: at the candidate the engine holds, e.g. the
        last solution.  One calcDiff sweep and one adjoint sweep on the device.  Exact for a candidate without gaps
        (a rollout, a feasible solution); there, at a converged solution, also the gradient of the optimal cost.  This
        shard's trajectories only (as the other getters)."""
        e = self.engine
        if xs is not None or us is not None:
            e.set_candidate(xs, us)
        return e.cost_sensitivity()

    def identify_plant(self, xs, us, n_steps=10, weights=None, stiffness_bounds=None, motor_inertia_bounds=None, mu0=1e-3,
                       grow=10.0, shrink=0.1, max_rel=0.5, min_curv=1e-12, keep_history=False):
        """Fit every trajectory's own spring stiffness and motor inertia to a recorded run (Engine.plant_identify;
        aslr_plant_identify): xs [B, T+1, nx] the recorded states, us [B, T, nu] the applied controls (put into the engine
        as cost_sensitivity(xs, us) puts them).  n_steps Levenberg-Marquardt steps on the weighted one-step prediction
        error sum_t |xs_{t+1} - f(xs_t, us_t; K, B)|^2_w, every trajectory on its own, starting from the parameters the
        problem holds.  stiffness_bounds / motor_inertia_bounds: (lo, hi), each [B, nj], [nj] or a scalar; a field whose bounds
        are None is not fitted (no stiffness_bounds for a VSA model).  -> engine.IdentifyResult; the problem's parameter
        table is left on the fit.  This shard's trajectories only."""
        e = self.engine
        e.set_candidate(xs, us)
        r = e.plant_identify(n_steps, self._shard(weights, 2), self._shard(stiffness_bounds, 2, pair=True),
                             self._shard(motor_inertia_bounds, 2, pair=True), mu0=mu0, grow=grow, shrink=shrink, max_rel=max_rel,
                             min_curv=min_curv, keep_history=keep_history)
        self._follow_table(r)
        return r

    def policy_rollout(self, xs, us, K, n_samples, plant_stiffness=None, plant_motor_inertia=None, dx0=None,
                       disturbance=None, clamp=False, keep_trajectories=False):
        """Closed-loop roll-outs of the policy u_t = us_t - K_t (x_t - xs_t) on n_samples perturbed plants per trajectory
        (Engine.policy_rollout; aslr_policy_rollout): xs [B, T+1, nx], us [B, T, nu], K [B, T, nu, nx] (or without the
        batch axis: the same for every trajectory; lists of per-knot arrays as the solvers return them do), all three
        None: the policy the engine holds.  The engine's own XS / US / KGAIN are put back afterwards, so a solve in
        progress is not disturbed.  -> engine.PolicyRolloutResult.  This shard's trajectories only."""
        e = self.engine
        if xs is None and us is None and K is None:
            return e.policy_rollout(n_samples, plant_stiffness, plant_motor_inertia, dx0, disturbance, clamp, keep_trajectories)
        if xs is None or us is None or K is None:
            raise ValueError("policy_rollout: give xs, us and K together (or none of them: the engine's own policy)")
        return self._with_policy(xs, us, K, lambda: e.policy_rollout(n_samples, plant_stiffness, plant_motor_inertia, dx0,
                                                                     disturbance, clamp, keep_trajectories))

    def policy_monte_carlo(self, xs, us, K, n_samples, seed, noise_std=None, dx0_std=None, stiffness_rel_std=None,
                           motor_inertia_rel_std=None, clamp=False, keep_trajectories=False, keep_draws=False, sample0=0,
                           trajectory0=0):
        """policy_rollout with the perturbations drawn on the device from `seed` (Engine.policy_rollout_noise;
        aslr_policy_rollout_noise): xs, us, K as policy_rollout takes them, all three None: the policy the engine holds.
        The engine's own XS / US / KGAIN are put back afterwards.  -> engine.PolicyRolloutResult (with `draws` when
        keep_draws).  This shard's trajectories only; trajectory0 is the shard's offset in the whole batch."""
        e = self.engine
        run = lambda: e.policy_rollout_noise(n_samples, seed, noise_std, dx0_std, stiffness_rel_std, motor_inertia_rel_std, clamp,
                                             keep_trajectories, keep_draws, sample0, trajectory0)
        if xs is None and us is None and K is None:
            return run()
        if xs is None or us is None or K is None:
            raise ValueError("policy_monte_carlo: give xs, us and K together (or none of them: the engine's own policy)")
        return self._with_policy(xs, us, K, run)

    def policy_covariance(self, xs, us, K, sigma0=None, noise_var=None, keep_cov=False):
        """First-order state and control covariance under the policy u_t = us_t - K_t (x_t - xs_t) (Engine.policy_covariance;
        aslr_policy_covariance): xs, us, K as policy_rollout takes them, all three None: the policy the engine holds.  The
        engine's own XS / US / KGAIN are put back afterwards.  -> engine.PolicyCovarianceResult.  This shard's
        trajectories only."""
        e = self.engine
        if xs is None and us is None and K is None:
            return e.policy_covariance(sigma0, noise_var, keep_cov)
        if xs is None or us is None or K is None:
            raise ValueError("policy_covariance: give xs, us and K together (or none of them: the engine's own policy)")
        return self._with_policy(xs, us, K, lambda: e.policy_covariance(sigma0, noise_var, keep_cov))

    def policy_lqg(self, xs, us, K, meas_var, measured=None, sigma0=None, noise_var=None, keep_gains=False):
        """First-order state and control covariance under output feedback, u_t = us_t - K_t eh_t with eh_t the estimate of the
        Kalman filter for the measured state entries (Engine.policy_lqg; aslr_policy_lqg): xs, us, K as policy_rollout
        takes them, all three None: the policy the engine holds.  The engine's own XS / US / KGAIN are put back afterwards.
        -> engine.LqgResult.  This shard's trajectories only."""
        e = self.engine
        run = lambda: e.policy_lqg(meas_var, measured, sigma0, noise_var, keep_gains)
        if xs is None and us is None and K is None:
            return run()
        if xs is None or us is None or K is None:
            raise ValueError("policy_lqg: give xs, us and K together (or none of them: the engine's own policy)")
        return self._with_policy(xs, us, K, run)

    def estimate_states(self, ys, us, meas_var, measured=None, xs_init=None, x0_mean=None, sigma0=None, noise_var=None,
                        n_iters=5, relax=1.0, keep_filter=False):
        """The full states of a recorded run from its encoder samples (Engine.estimate_states; aslr_state_smooth): ys
        [B, T+1, ny] the samples of the state entries `measured` (None: the nx / 2 positions q_l, q_m) read with noise of
        variance meas_var (a scalar, [ny] or [B, ny]), us [B, T, nu] the applied controls.  n_iters iterations of the extended
        Kalman smoother on the problem's model (with the parameters the problem holds), from the nominal xs_init
        [B, T+1, nx]; None, with the default `measured` only: the positions from ys and the velocities by forward differences
        of ys over the models' dt, the last row repeated.  x0_mean [B, nx]: the prior mean of x_0 (None: xs_init at knot 0)
        with covariance sigma0; noise_var: the process noise; both as policy_lqg takes them, at least one of the two.
        -> engine.SmoothResult: xs [B, T+1, nx], neg_log_lik and step_norm [B, n_iters] and, with keep_filter, x_filt,
        est_var [B, T+1, nx] and nis [B, T+1].  result.xs goes into identify_plant(xs, us, ...) as it is.  The engine's
        candidate is left on the estimate.  This shard's trajectories only."""
        import torch
        e = self.engine
        if xs_init is None:
            if measured is not None and [int(i) for i in measured] != list(range(e.nx // 2)):
                raise ValueError("estimate_states: xs_init is required when `measured` is not the positions")
            y = e._f64(ys)
            if y.dim() != 3 or tuple(y.shape[1:]) != (self.T + 1, e.nx // 2):
                raise ValueError("ys must have shape [B=%d, T+1=%d, ny=%d]" % (self.batch, self.T + 1, e.nx // 2))
            dt = torch.as_tensor([float(m.dt) for m in self.runningModels], dtype=torch.float64, device=y.device)
            v = (y[:, 1:] - y[:, :-1]) / dt[None, :, None]
            xs_init = torch.cat([y, torch.cat([v, v[:, -1:]], dim=1)], dim=2)
        e.set_candidate(xs_init, us)
        return e.estimate_states(ys, meas_var, measured, x0_mean, sigma0, noise_var, n_iters, relax, keep_filter)

    def policy_plant_sensitivity(self, xs, us, K, stiffness_var=None, motor_inertia_var=None, keep_trajectories=False):
        """First-order sensitivity of the closed loop under the policy u_t = us_t - K_t (x_t - xs_t) to the plant's spring
        stiffness and motor inertia (Engine.policy_plant_sensitivity; aslr_policy_plant_sensitivity): xs, us, K as
        policy_rollout takes them, all three None: the policy the engine holds.  The engine's own XS / US / KGAIN are put
        back afterwards.  -> engine.PlantSensitivityResult.  This shard's trajectories only."""
        e = self.engine
        if xs is None and us is None and K is None:
            return e.policy_plant_sensitivity(stiffness_var, motor_inertia_var, keep_trajectories)
        if xs is None or us is None or K is None:
            raise ValueError("policy_plant_sensitivity: give xs, us and K together (or none of them: the engine's own policy)")
        return self._with_policy(xs, us, K, lambda: e.policy_plant_sensitivity(stiffness_var, motor_inertia_var, keep_trajectories))

    def _with_policy(self, xs, us, K, call):
        """call() with (xs, us, K) in the engine's XS / US / KGAIN; the engine's own are put back afterwards"""
        import torch
        e = self.engine
        keep = [(r, e.region(r).clone()) for r in (_abi.R_XS, _abi.R_US, _abi.R_KGAIN)]
        try:
            e.set_candidate(xs, us)
            k = torch.as_tensor(np.asarray(K, dtype=np.float64) if not torch.is_tensor(K) else K, dtype=torch.float64, device=e.device)
            if k.dim() == 3:
                k = k.unsqueeze(0).expand(self.batch, -1, -1, -1)
            if k.dim() == 4 and k.shape[2] == e.nu_user and e.nu_user != e.nu:  # padded controls: zero gain rows
                k = torch.cat([k, torch.zeros(k.shape[:2] + (e.nu - e.nu_user, k.shape[3]), dtype=k.dtype, device=k.device)], dim=2)
            if tuple(k.shape) != (self.batch, self.T, e.nu, e.nx):
                raise ValueError("K must have shape [B=%d, T=%d, nu=%d, nx=%d]" % (self.batch, self.T, e.nu_user, e.nx))
            e.region(_abi.R_KGAIN).copy_(k.permute(1, 0, 2, 3))
            return call()
        finally:
            for r, t in keep:
                e.region(r).copy_(t)

    def _total_cost(self):
        c = self.engine.region(_abi.R_COST).sum(dim=0)
        return float(c[0].item()) if self.batch == 1 else c

    def rollout(self, us):
        """xs with xs[0] = x0 and xs[t+1] = xnext(xs[t], us[t]): T sequential calc sweeps are avoided by
        running the forward kernel with zero gains (K = 0, k = 0, alpha = 1)."""
        import torch
        e = self.engine
        # the solver's state the forward kernel reads is saved and put back: rollout() has no side effect on a
        # solve in progress (gains, candidate, feasibility flags)
        rids = (_abi.R_XS, _abi.R_US, _abi.R_KGAIN, _abi.R_KFF)
        keep = [(r, e.region(r).clone()) for r in rids]
        feas = e.region(_abi.R_TRAJ_I)[_abi.TI_FEASIBLE].clone()
        e.set_candidate(None, us)
        e.region(_abi.R_KGAIN).zero_()
        e.region(_abi.R_KFF).zero_()
        e.region(_abi.R_TRAJ_I)[_abi.TI_FEASIBLE].fill_(1)
        e.forward_pass(_abi.default_solver_params(_abi.SOLVER_DDP))
        xs = e.region(_abi.R_XS_TRY)[0].permute(1, 0, 2)
        out = [x for x in xs[0].cpu().numpy()] if self.batch == 1 else xs.clone()
        for r, t in keep:
            e.region(r).copy_(t)
        e.region(_abi.R_TRAJ_I)[_abi.TI_FEASIBLE].copy_(feas)
        torch.cuda.synchronize(e.device)
        return out

    def quasiStatic(self, xs, maxiter=100, tol=1e-9):
        """us[t] holding xs[t] still under node t's model (examples/two_dof_sea.py:78); xs has T entries."""
        import torch
        e = self.engine
        xs = np.asarray(xs, dtype=np.float64) if not torch.is_tensor(xs) else xs
        x = torch.as_tensor(xs, dtype=torch.float64, device=e.device)
        if x.dim() == 2:
            x = x.unsqueeze(0).expand(self.batch, -1, -1)
        X = e.region(_abi.R_XS)
        X[:self.T].copy_(x[:, :self.T].permute(1, 0, 2))
        e.region(_abi.R_US).zero_()
        e.quasi_static(maxiter, tol)
        torch.cuda.synchronize(e.device)
        U = e.cut_u(e.region(_abi.R_US).permute(1, 0, 2))
        return [u for u in U[0].cpu().numpy()] if self.batch == 1 else U.clone()

    @property
    def runningDatas(self):
        return _DataList(_NodeData(self, t) for t in range(self.T))

    @property
    def terminalData(self):
        return _NodeData(self, self.T)


class CallbackLogger(object):
    """crocoddyl.CallbackLogger (examples/double_pendulum.py:77-79, examples/two_dof_sea.py:75): per-iteration
    `costs, u_regs, x_regs, grads, stops, steps, iters` and the solver's latest `xs, us, fs`.
    B = 1: plain Python lists, one entry per iteration, as in Crocoddyl.  A batch: after solve() the same names hold
    numpy arrays [iterations, B] (NaN where a trajectory had already stopped) and `iters` the per-trajectory
    iteration counts; they come from the device-resident log in one transfer."""

    def __init__(self):
        self.xs, self.us, self.fs = [], [], []
        self.costs, self.u_regs, self.x_regs, self.grads, self.stops, self.steps = [], [], [], [], [], []
        self.iters = []

    def __call__(self, solver):
        self.xs, self.us, self.fs = solver.xs, solver.us, solver.fs
        self.iters.append(solver.iter)
        self.costs.append(solver.cost)
        self.u_regs.append(solver.u_reg)
        self.x_regs.append(solver.x_reg)
        self.grads.append(-solver.d[1])   # Crocoddyl: -expectedImprovement()[1]
        self.stops.append(solver.stop)
        self.steps.append(solver.stepLength)

    def from_batch_log(self, solver, log, iters):
        """log: numpy [n, LOG_COUNT, B]; iters: per-trajectory iteration counts."""
        self.xs, self.us, self.fs = solver.xs, solver.us, solver.fs
        self.costs, self.stops = log[:, _abi.LOG_COST], log[:, _abi.LOG_STOP]
        self.x_regs = self.u_regs = log[:, _abi.LOG_XREG]
        self.grads, self.steps = -log[:, _abi.LOG_D2], log[:, _abi.LOG_STEP]
        self.iters = iters


class CallbackVerbose(object):
    """crocoddyl.CallbackVerbose: one table row per iteration -- iter, cost, stop, grad (= -d[1]), xreg, ureg, step,
    feas -- with the header repeated every 10 iterations (the layout of the Crocoddyl 1.x generation the reference
    was written against; unverifiable here).  For a batch one row per lock-step iteration with the
    active-trajectory count, the summed cost and the largest stop / regularisation of the active trajectories."""

    def __init__(self, out=None):
        self.out = out or sys.stdout

    def __call__(self, solver):
        if solver.iter % 10 == 0:
            self.out.write("iter \t cost \t      stop \t    grad \t  xreg \t      ureg \t step \t feas\n")
        self.out.write("%4d  %.5e  %.5e  %.5e  %.5e  %.5e  %.4f     %d\n" % (
            solver.iter, solver.cost, solver.stop, -solver.d[1], solver.x_reg, solver.u_reg, solver.stepLength,
            1 if solver.isFeasible else 0))

    def from_batch_log(self, solver, log, iters):
        for i in range(log.shape[0]):
            on = ~np.isnan(log[i, _abi.LOG_COST])
            if not on.any():
                break
            if i % 10 == 0:
                self.out.write("iter  active   sum cost     max stop     max grad     max xreg   mean step\n")
            self.out.write("%4d  %6d  %.5e  %.5e  %.5e  %.5e  %.4f\n" % (
                i, int(on.sum()), log[i, _abi.LOG_COST][on].sum(), log[i, _abi.LOG_STOP][on].max(),
                (-log[i, _abi.LOG_D2][on]).max(), log[i, _abi.LOG_XREG][on].max(), log[i, _abi.LOG_STEP][on].mean()))


class _IterationView(object):
    """The solver as a callback of iteration i saw it (B = 1), rebuilt from row i of the device log."""

    def __init__(self, solver, row, i):
        self._s = solver
        self.iter = i
        self.cost, self.stop = float(row[_abi.LOG_COST]), float(row[_abi.LOG_STOP])
        self.x_reg = self.u_reg = float(row[_abi.LOG_XREG])
        self.stepLength = float(row[_abi.LOG_STEP])
        self.d = [float(row[_abi.LOG_D1]), float(row[_abi.LOG_D2])]
        self.dV, self.dVexp = float(row[_abi.LOG_DV]), float(row[_abi.LOG_DVEXP])
        self.isFeasible = int(row[_abi.LOG_FEASIBLE])
        self.status = int(row[_abi.LOG_STATUS])

    def __getattr__(self, name):  # xs, us, fs, problem, K ...: the solver's (final) ones
        return getattr(self._s, name)


class SolverDDP(object):
    """crocoddyl.SolverDDP on the batched GPU engine.  All of `x_reg, alpha, feasible, cost, stop,
    iter, status` are per trajectory; scalar properties report trajectory 0 for a
    B = 1 problem and tensors for a batch."""
    _solver = _abi.SOLVER_DDP

    def __init__(self, problem):
        self.problem = problem
        sp = _abi.default_solver_params(self._solver)
        self._sp = sp
        self._callbacks = []
        self.keep_log = False   # record the per-iteration log even without callbacks (iteration_log())
        self.poll_every = 4
        self.batch_iters = 0

    # -- parameters (crocoddyl member names) --
    def _param(name):  # noqa: N805
        return property(lambda s: getattr(s._sp, name), lambda s, v: setattr(s._sp, name, v))

    th_stop = _param("th_stop")
    th_grad = _param("th_grad")
    th_gaptol = _param("th_gaptol")
    th_stepdec = _param("th_stepdec")
    th_stepinc = _param("th_stepinc")
    th_acceptstep = _param("th_acceptstep")
    th_acceptnegstep = _param("th_acceptnegstep")
    reg_min = _param("reg_min")
    reg_max = _param("reg_max")
    reg_incfactor = _param("reg_incfactor")
    reg_decfactor = _param("reg_decfactor")
    del _param

    @property
    def alphas(self):
        return [1.0 / 2 ** j for j in range(_abi.NALPHA)]

    def setCallbacks(self, callbacks):
        """Callbacks are NOT called during the solve: the line-search kernel records what they read (cost, stop, regularisation,
        step length, d, dV, feasibility, status) into a device-resident log and they are replayed from it when solve()
        returns (B = 1: once per iteration with an _IterationView; a batch: `from_batch_log`).  Consequences, different
        from Crocoddyl: (1) inside a callback `xs / us / fs / K / k` are the solver's FINAL values, not those of that
        iteration (a display callback such as examples/double_pendulum.py:60 CallbackDisplay would show the final
        trajectory every time); (2) CallbackVerbose prints after the solve, not while it runs; (3) a callback cannot
        stop the solve.  For per-iteration trajectories drive the solver one iteration at a time: `solve(xs, us, 1,
        isFeasible=...)` in a loop keeps every semantic of the reference at the price of a host round trip per iteration."""
        self._callbacks = list(callbacks)

    def getCallbacks(self):
        return self._callbacks

    # -- solve --
    def solve(self, init_xs=None, init_us=None, maxiter=100, isFeasible=False, regInit=None):
        """solver.solve(init_xs=[], init_us=[], maxiter=100, isFeasible=False, regInit=nan) -> bool
        (all trajectories converged)."""
        import torch
        e = self.problem.engine
        sp = self._sp
        sp.maxiter = int(maxiter)
        sp.is_feasible = 1 if isFeasible else 0
        sp.reg_init = float("nan") if regInit is None else float(regInit)
        e.set_candidate(init_xs, init_us)
        # callbacks: the line-search kernel records what they read into a device-resident log; the solve runs
        # without a host round trip per iteration and the callbacks are replayed from the log afterwards
        e.enable_iteration_log(sp.maxiter if (self._callbacks or self.keep_log) and sp.maxiter > 0 else 0)
        self.batch_iters = e.solve(sp, self.poll_every)
        torch.cuda.synchronize(e.device)
        st = e.traj_i(_abi.TI_STATUS)
        if self._callbacks:
            self._replay_callbacks()
        return bool(((st & _abi.ST_CONVERGED) != 0).all().item())

    def solve_mpc(self, n_steps, iters_per_step, init_xs=None, init_us=None, maxiter=100, isFeasible=False,
                  disturbance=None, regInit=None, hold=1, plant_stiffness=None, plant_motor_inertia=None, clamp=None,
                  closed_cost=False):
        """A receding-horizon run of n_steps control steps on the device (aslr_mpc_run): `solve(init_xs, init_us,
        maxiter, isFeasible)` first, then per step -- apply us[0] to the plant (the first running model), add
        disturbance[:, s] ([B, n_steps, nx], optional) to its next state, shift the plan one knot,
        `solve(xs, us, iters_per_step, isFeasible)` -- the loop a script writes around solver.solve, without a host
        round trip per step.  Callbacks are not replayed (the per-iteration log would be overwritten every step).
        With a reference path (ShootingProblem(frame_ref_path=) / set_reference_path) step s plans against the rows
        reference_row + s + t; afterwards problem.reference_row has grown by n_steps (MpcResult.reference_row).
        -> engine.MpcResult; solver.xs / us are the last shifted plan.

        On a plant that differs from the model (aslr_mpc_run_plant; aslr_mpc_run_plant_all on the 7-joint arms, so every
        model size is served; any of the following away from its default): hold = h
        re-plans only every h knots and tracks with the Riccati gains of the last solve in between, u = us_j - K_j (x -
        xs_j); plant_stiffness / plant_motor_inertia [B, nj] are the diagonals of the plant's K and B (no plant_stiffness
        for a VSA model); clamp: clamp the applied controls to the box, None = iff this solver is SolverBoxDDP;
        closed_cost: also sum the running costs of the applied knots.  disturbance is then [B, n_steps * h, nx], the
        result holds n_steps * h applied knots, closed_cost [B], failed_knot [B] and hold, and the reference row grows
        by n_steps * h (Engine.mpc_run_plant)."""
        e = self.problem.engine
        sp = self._sp
        sp.maxiter = int(maxiter)
        sp.is_feasible = 1 if isFeasible else 0
        sp.reg_init = float("nan") if regInit is None else float(regInit)
        e.set_candidate(init_xs, init_us)
        e.enable_iteration_log(0)
        if hold == 1 and plant_stiffness is None and plant_motor_inertia is None and clamp is None and not closed_cost:
            return e.mpc_run(sp, n_steps, sp.maxiter, iters_per_step, disturbance)
        if clamp is None:
            clamp = self._solver == _abi.SOLVER_BOXDDP
        return e.mpc_run_plant(sp, n_steps, sp.maxiter, iters_per_step, hold, plant_stiffness, plant_motor_inertia,
                               disturbance, bool(clamp), bool(closed_cost))

    def solve_pool(self, x0s, frame_refs=None, maxiter=100, isFeasible=False, regInit=None, refill_every=4,
                   poll_every=16, init_xs=None, init_us=None, stiffness=None, motor_inertia=None, u_lb=None, u_ub=None):
        """Solve MANY problems of this solver's structure (per-problem x0 and, optionally, frame-placement targets as
        pinocchio.SE3 or [P, 12] arrays), each from a cold start to its own stop, streaming them through the problem's
        trajectory slots (the loop `for x0 in x0s: solver.solve([], [], maxiter)` of a script, run on the device:
        aslr_solve_pool).  -> dict of torch tensors: xs [P, T+1, nx], us [P, T, nu], cost, stop, x_reg, step, iters,
        status [P], and batch_iters.
        stiffness / motor_inertia [P, nj], u_lb / u_ub [P, nu], each optional: problem j is solved with row j of every given
        field, i.e. with action models whose K, B and control box are that row's (a design sweep streamed through the slots:
        aslr_solve_pool_params); a field left out keeps the models' constant."""
        sp = self._sp
        sp.maxiter = int(maxiter)
        sp.is_feasible = 1 if isFeasible else 0
        sp.reg_init = float("nan") if regInit is None else float(regInit)
        x0s = np.atleast_2d(np.asarray(x0s, dtype=np.float64))
        fr = None
        if frame_refs is not None:
            fr = np.array([f.as12() if hasattr(f, "as12") else np.asarray(f, dtype=np.float64).reshape(12) for f in frame_refs])
        return self.problem.engine.solve_pool(x0s, fr, sp, refill_every, poll_every, init_xs, init_us, stiffness,
                                              motor_inertia, u_lb, u_ub)

    def optimize_design(self, n_steps, iters_per_step, init_xs=None, init_us=None, maxiter=100, stiffness_bounds=None,
                        motor_inertia_bounds=None, eta0=0.05, grow=2.0, shrink=0.5, c1=1e-4, max_rel=0.25, keep_history=False):
        """Improve every trajectory's own spring stiffness and motor inertia by n_steps steps of a bounded descent on the
        device (aslr_design_descent, include/aslr_to_amd_design.h): `solve(init_xs, init_us, maxiter)` at the design the
        problem holds (its parameter table, else the models' constants), then per step -- the gradient of cost_sensitivity,
        an Armijo test (c1) against the accepted design, the next design a step of eta in log theta (at most max_rel per
        entry, inside the bounds; eta grows after an accepted step and shrinks after a rejected one), `solve(xs, us,
        iters_per_step)` from the accepted plan -- the loop a script writes around solver.solve and cost_sensitivity, without
        a host round trip per step.  stiffness_bounds / motor_inertia_bounds: (lo, hi), each [B, nj], [nj] or a scalar; a
        field whose bounds are None is not optimised (no stiffness_bounds for a VSA model).  -> engine.DesignResult
        (stiffness, motor_inertia, cost, xs, us and, with keep_history, the per-step histories); solver.xs / us and the
        problem's parameter table are left on the accepted design.  Callbacks are not replayed."""
        p = self.problem
        e = p.engine
        sp = self._sp
        sp.maxiter = int(maxiter)
        sp.is_feasible = 0
        sp.reg_init = float("nan")
        e.set_candidate(init_xs, init_us)
        e.enable_iteration_log(0)
        r = e.design_descent(sp, n_steps, sp.maxiter, iters_per_step, p._shard(stiffness_bounds, 2, pair=True),
                             p._shard(motor_inertia_bounds, 2, pair=True), eta0, grow, shrink, c1, max_rel, keep_history)
        p._follow_table(r)
        return r

    def cost_sensitivity(self):
        """problem.cost_sensitivity() at this solver's solution (the committed xs / us of the last solve): per
        trajectory dJ/dK, dJ/dB, dJ/dx0 and the costates."""
        return self.problem.cost_sensitivity()

    def policy_rollout(self, n_samples, plant_stiffness=None, plant_motor_inertia=None, dx0=None, disturbance=None,
                       clamp=None, keep_trajectories=False):
        """How the policy of the last solve (its xs, us and Riccati gains K) holds up on a plant that differs from the
        model: n_samples = S closed loops per trajectory, u_t = us_t - K_t (x_t - xs_t), each on its own plant.  Batch-
        major arrays or tensors, each optional: plant_stiffness / plant_motor_inertia [B, S, nj] (diagonals of K and B;
        no plant_stiffness for a VSA model), dx0 [B, S, nx], disturbance [B, S, T, nx].  clamp: clamp the controls to the
        box; None = iff this solver is SolverBoxDDP.  -> engine.PolicyRolloutResult: cost [B, S], failed_knot [B, S],
        x_final [B, S, nx], and xs [B, S, T+1, nx] / us [B, S, T, nu] with keep_trajectories.  One launch on the device
        that writes nothing into the solver's state (aslr_policy_rollout, include/aslr_to_amd_policy.h)."""
        if clamp is None:
            clamp = self._solver == _abi.SOLVER_BOXDDP
        return self.problem.engine.policy_rollout(n_samples, plant_stiffness, plant_motor_inertia, dx0, disturbance,
                                                  bool(clamp), keep_trajectories)

    def policy_monte_carlo(self, n_samples, seed, noise_std=None, dx0_std=None, stiffness_rel_std=None,
                           motor_inertia_rel_std=None, clamp=None, keep_trajectories=False, keep_draws=False, sample0=0,
                           trajectory0=0):
        """policy_rollout as a Monte-Carlo run whose perturbations are drawn on the device: sample s of trajectory b gets
        disturbance = noise_std z, dx0 = dx0_std z, K_j = Knom_j exp(stiffness_rel_std z) and B_j likewise, z standard
        normals of a counter-based generator (Philox4x32-10, Box-Muller; include/aslr_to_amd_policy_noise.h) that depend on
        (seed, knot, sample0 + s, trajectory0 + b, entry) alone.  So n_samples is bounded by time, not by memory; a run is
        reproducible from `seed`; a shard draws what the whole batch would (trajectory0); and one sample can be replayed
        alone (sample0, n_samples = 1) with keep_trajectories.  Each sigma: None (absent), a scalar, [nx] / [nj] or
        [B, nx] / [B, nj]; no stiffness_rel_std for a VSA model.  clamp as in policy_rollout.  -> engine.PolicyRolloutResult;
        with keep_draws it carries `draws`: plant_stiffness, plant_motor_inertia, dx0, disturbance, the very arguments
        policy_rollout accepts."""
        if clamp is None:
            clamp = self._solver == _abi.SOLVER_BOXDDP
        return self.problem.engine.policy_rollout_noise(n_samples, seed, noise_std, dx0_std, stiffness_rel_std,
                                                        motor_inertia_rel_std, bool(clamp), keep_trajectories, keep_draws,
                                                        sample0, trajectory0)

    def policy_covariance(self, sigma0=None, noise_var=None, keep_cov=False):
        """What the policy of the last solve (its xs, us and Riccati gains K) does to uncertainty, to first order and without
        samples: the state covariance Sigma_{t+1} = A_t Sigma_t A_t^T + diag(noise_var_t), A_t = Fx_t - Fu_t K_t, from
        Sigma_0 = sigma0 ([B, nx, nx] or [nx, nx], symmetric) and process noise of variance noise_var ([B, T, nx], [B, nx]
        or [nx]; noise t enters x_{t+1}), at least one of the two.  -> engine.PolicyCovarianceResult: x_var [B, T+1, nx],
        u_var [B, T, nu] (compare its square root with the distance of us to the control box), cov_final [B, nx, nx],
        cost_increase [B] (the expected cost of the spread in the solver's quadratic model) and cov [B, T+1, nx, nx] with
        keep_cov.  Every model size, the 7-joint arms included.  One calcDiff sweep and one forward sweep on the device
        (aslr_policy_covariance, include/aslr_to_amd_cov.h); the box is not applied."""
        return self.problem.engine.policy_covariance(sigma0, noise_var, keep_cov)

    def policy_lqg(self, meas_var, measured=None, sigma0=None, noise_var=None, keep_gains=False):
        """policy_covariance for an arm that does not see its whole state: the state entries `measured` (None: the positions
        q_l, q_m -- two encoders per joint) are read at every knot with noise of variance meas_var (a scalar, [ny] or [B, ny],
        > 0), a time-varying Kalman filter linearised about the plan estimates the rest, and the Riccati gains of the last
        solve act on the estimate.  sigma0 and noise_var as in policy_covariance.  -> engine.LqgResult: x_var [B, T+1, nx],
        u_var [B, T, nu], est_var [B, T+1, nx] (what the filter does not know after each measurement), cov_final and
        est_cov_final [B, nx, nx], cost_increase [B] and, with keep_gains, kalman_gain [B, T+1, nx, ny].  Every model size.
        One calcDiff sweep and one forward sweep on the device (aslr_policy_lqg, include/aslr_to_amd_lqg.h); the box is not
        applied."""
        return self.problem.engine.policy_lqg(meas_var, measured, sigma0, noise_var, keep_gains)

    def policy_plant_sensitivity(self, stiffness_var=None, motor_inertia_var=None, keep_trajectories=False):
        """Where the policy of the last solve (its xs, us and Riccati gains K) ends up on an arm whose springs or motors are
        not the model's, to first order and without samples: S_t = dx_t/dtheta for theta = (diag K, diag B) under
        u_t = us_t - K_t (x_t - xs_t), S_{t+1} = (Fx_t - Fu_t K_t) S_t + G_t from S_0 = 0.  -> engine.PlantSensitivityResult:
        dx_final_dstiffness, dx_final_dmotor_inertia [B, nx, nj], dcost_dstiffness, dcost_dmotor_inertia [B, nj] (the cost
        of the closed loop, the feedback's corrections included), with stiffness_var / motor_inertia_var ([B, nj] or [nj],
        variances of independent parameter errors) x_var [B, T+1, nx] and u_var [B, T, nu], and with keep_trajectories
        dxs_dstiffness, dxs_dmotor_inertia [B, T+1, nx, nj].  A relative error r in K_j moves x_T by
        r * K_j * dx_final_dstiffness[:, :, j].  Every model size, the 7-joint arms included; the stiffness fields are None
        for a VSA model.  One calcDiff sweep and one forward sweep on the device (aslr_policy_plant_sensitivity,
        include/aslr_to_amd_plant_sens.h); the box is not applied."""
        return self.problem.engine.policy_plant_sensitivity(stiffness_var, motor_inertia_var, keep_trajectories)

    def iteration_log(self):
        """numpy [iterations, LOG_COUNT, B] of the last solve (needs callbacks or `keep_log = True`), trimmed to the
        iterations some trajectory ran; NaN where a trajectory had stopped.  Fields: _abi.LOG_*."""
        lg = self.problem.engine.iteration_log()
        if lg is None:
            return None
        n = int(self.problem.engine.traj_i(_abi.TI_ITER).max().item())
        return lg[:min(n, lg.shape[0])].cpu().numpy()

    def _replay_callbacks(self):
        log = self.iteration_log()
        iters = self.problem.engine.traj_i(_abi.TI_ITER).cpu().numpy()
        if self._single():
            for i in range(log.shape[0]):
                row = log[i, :, 0]
                # Crocoddyl returns from solve() before the callbacks when the regularisation hits its maximum
                if int(row[_abi.LOG_STATUS]) & _abi.ST_REG_MAX:
                    break
                view = _IterationView(self, row, i)
                for cb in self._callbacks:
                    cb(view)
        else:
            for cb in self._callbacks:
                if hasattr(cb, "from_batch_log"):
                    cb.from_batch_log(self, log, iters)
                else:
                    raise TypeError("callback %r cannot consume a batch log (needs from_batch_log)" % (cb,))

    def export_solution(self, path, trajectory=0):
        """The arrays examples/two_dof_vsa_boxddp.py:104-127 saves to .mat files, as one .npz: t [T], q [T+1, nj]
        (link positions), u [T, nj] (motor commands), stiffness [T, nj] (VSA models; empty otherwise), xs, us.
        trajectory: index in the batch, or None for all ([B, ...])."""
        e = self.problem.engine
        X = self.xs if not self._single() else np.asarray(self.xs)[None]
        U = self.us if not self._single() else np.asarray(self.us)[None]
        X = X.cpu().numpy() if hasattr(X, "cpu") else np.asarray(X)
        U = U.cpu().numpy() if hasattr(U, "cpu") else np.asarray(U)
        nj = e.nx // 4
        dt = float(self.problem.runningModels[0].dt)
        sel = slice(None) if trajectory is None else int(trajectory)
        vsa = e.nu_user == 2 * nj
        np.savez(path, t=np.arange(self.problem.T) * dt, q=X[sel][..., :nj], u=U[sel][..., :nj],
                 stiffness=U[sel][..., nj:] if vsa else np.zeros(U[sel].shape[:-1] + (0,)), xs=X[sel], us=U[sel])
        return path

    # -- results --
    def _single(self):
        return self.problem.batch == 1

    def _current_xu(self):
        """xs/us including a not-yet-committed accepted candidate (only matters inside callbacks)."""
        import torch
        e = self.problem.engine
        acc = e.traj_i(_abi.TI_ACCEPTED)
        X, U = e.region(_abi.R_XS), e.region(_abi.R_US)
        if bool((acc >= 0).any().item()):
            X, U = X.clone(), U.clone()
            XT, UT = e.region(_abi.R_XS_TRY), e.region(_abi.R_US_TRY)
            for b in torch.nonzero(acc >= 0).flatten().tolist():
                a = int(acc[b].item())
                X[:, b] = XT[a, :, b]
                U[:, b] = UT[a, :, b]
        return X.permute(1, 0, 2), U.permute(1, 0, 2)

    @property
    def xs(self):
        X, _ = self._current_xu()
        return [x for x in X[0].cpu().numpy()] if self._single() else X

    @property
    def us(self):
        _, U = self._current_xu()
        U = self.problem.engine.cut_u(U)
        return [u for u in U[0].cpu().numpy()] if self._single() else U

    def _tf(self, row):
        v = self.problem.engine.traj_f(row)
        return float(v[0].item()) if self._single() else v

    def _ti(self, row):
        v = self.problem.engine.traj_i(row)
        return int(v[0].item()) if self._single() else v

    cost = property(lambda s: s._tf(_abi.TF_COST))
    stop = property(lambda s: s._tf(_abi.TF_STOP))
    x_reg = property(lambda s: s._tf(_abi.TF_XREG))
    u_reg = property(lambda s: s._tf(_abi.TF_XREG))
    stepLength = property(lambda s: s._tf(_abi.TF_STEP))
    dV = property(lambda s: s._tf(_abi.TF_DV))
    dVexp = property(lambda s: s._tf(_abi.TF_DVEXP))
    d = property(lambda s: [s._tf(_abi.TF_D1), s._tf(_abi.TF_D2)])
    status = property(lambda s: s._ti(_abi.TI_STATUS))
    isFeasible = property(lambda s: s._ti(_abi.TI_FEASIBLE))

    @property
    def iter(self):
        """Crocoddyl's iter_: index of the last iteration when solve() returned from inside the loop
        (converged / regularisation at its maximum), maxiter otherwise."""
        n, st = self._ti(_abi.TI_ITER), self._ti(_abi.TI_STATUS)
        inside = (st & (_abi.ST_CONVERGED | _abi.ST_REG_MAX)) != 0
        if self._single():
            return n - 1 if inside and n > 0 else n
        return n - (inside & (n > 0)).to(n.dtype)

    @property
    def iterations(self):
        """number of completed iterations per trajectory"""
        return self._ti(_abi.TI_ITER)

    def _gain(self, rid):
        import torch
        e = self.problem.engine
        torch.cuda.synchronize(e.device)
        v = e.region(rid)
        if rid in (_abi.R_KGAIN, _abi.R_KFF, _abi.R_QU):  # [T, B, nu(, nx)]: the models' own controls
            v = e.cut_u(v, axis=2)
        return [g for g in v[:, 0].cpu().numpy()] if self._single() else v.transpose(0, 1)

    def _value(self, rid):
        """Vx / Vxx are not kept by the solve loop (212 MB per 4096-trajectory shard, written for nobody): they are
        recomputed here by one stand-alone backward pass on the CURRENT iterate and regularisation (Crocoddyl
        holds those of its last iteration's backward pass, i.e. one step earlier); K, k, Qu are left untouched."""
        import torch
        e = self.problem.engine
        keep = [(r, e.region(r).clone()) for r in (_abi.R_KGAIN, _abi.R_KFF, _abi.R_QU)]
        e.calc_diff()
        e.backward_pass(self._sp)
        torch.cuda.synchronize(e.device)
        v = e.region(rid).clone()
        for r, t in keep:
            e.region(r).copy_(t)
        return [g for g in v[:, 0].cpu().numpy()] if self._single() else v.transpose(0, 1)

    Vx = property(lambda s: s._value(_abi.R_VX))
    Vxx = property(lambda s: s._value(_abi.R_VXX))
    K = property(lambda s: s._gain(_abi.R_KGAIN))
    k = property(lambda s: s._gain(_abi.R_KFF))
    Qu = property(lambda s: s._gain(_abi.R_QU))
    fs = property(lambda s: s._gain(_abi.R_GAPS))


class SolverFDDP(SolverDDP):
    """crocoddyl.SolverFDDP (examples/two_dof_sea.py:69)."""
    _solver = _abi.SOLVER_FDDP


class SolverBoxDDP(SolverDDP):
    """crocoddyl.SolverBoxDDP (examples/two_dof_vsa_boxddp.py:69)."""
    _solver = _abi.SOLVER_BOXDDP


def reduce_stats(solver, group=None):
    """Global termination / reporting scalars over all shards; see dist.py."""
    from .dist import all_reduce_stats, local_stats
    return all_reduce_stats(local_stats(solver.problem.engine), group)
