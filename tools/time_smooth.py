"""Times of one iteration of the state smoother (aslr_state_smooth) beside the calcDiff sweep and the filter-alone LQG sweep
(aslr_policy_lqg with est_var and kalman_gain only) of the same handle, in the same run, with HIP events on the launch
stream, and the noisy end-to-end experiment: tools/time_smooth.py [repeats]

Shapes (tools/_timing.STANDARD_SHAPES): two_dof_vsa_boxddp (B = 4096, T = 100), talos_arm_sea and talos_arm_vsa (B = 512,
T = 150); the positions measured (ny = nx / 2), sigma0 and noise_var given.  The plan is tools/time_lqg.py's; ys are its
positions.  Per shape, the median over `repeats` (default 20) of
  calc_diff    aslr_calc_diff alone;
  filter only  aslr_policy_lqg, est_var and kalman_gain alone, minus calc_diff: lqg_kernel without the estimate's half;
  smooth       aslr_state_smooth with n_iters = 1 and every output, minus calc_diff: smooth_filter_kernel and
               smooth_adjoint_kernel; XS is put back before every call, outside the timed stretch;
  ratio        smooth / filter only: what the mean, the stores to work and the adjoint sweep cost.
Experiment (two_dof_sea, B = 64, T = 100): the plant has stiffness and motor inertia 20 % off the model's, the encoders read
the positions of a roll-out on it with noise of 1e-4 rad; identify_plant on the smoothed states (5 iterations from the
finite-difference default) against identify_plant on the finite-difference states themselves: the median and the worst
relative error of the fitted parameters, each way.  No threshold is asserted."""
import sys

import numpy as np
import torch

from _timing import STANDARD_SHAPES, planned, ptr, seeded_spread, timed
from aslr_to_amd import _abi, crocoddyl, scenarios
from time_lqg import ITERATIONS


def times(repeats):
    for name, make in STANDARD_SHAPES.items():
        e, sp = planned(make, ITERATIONS[name])
        s0, w, r = seeded_spread(e)
        ny = e.nx // 2
        rh = r[:, :ny].contiguous()
        new = lambda *s: torch.zeros(s, dtype=torch.float64, device=e.device)
        ev, kg = new(e.T + 1, e.B, e.nx), new(e.T + 1, e.B, e.nx, ny)
        xs, xf, nis, nll, step = new(e.T + 1, e.B, e.nx), new(e.T + 1, e.B, e.nx), new(e.T + 1, e.B), new(1, e.B), new(1, e.B)
        work = new((e.T + 1) * e.B * (e.nx * e.nx + e.nx * ny + e.nx + ny))
        XS = e.region(_abi.R_XS)
        plan = XS.clone()
        ys, x0 = plan[:, :, :ny].contiguous(), plan[0].clone()
        filt = lambda: e._call("aslr_policy_lqg", ny, None, ptr(rh), ptr(s0), ptr(w), None, None, ptr(ev), None, None, ptr(kg), None,
                               e._stream())

        def smooth():
            e._call("aslr_state_smooth", ny, None, ptr(ys), ptr(rh), ptr(x0), ptr(s0), ptr(w), 1, 1.0, ptr(work), ptr(xs), ptr(xf),
                    ptr(ev), ptr(nis), ptr(nll), ptr(step), e._stream())

        def timed_smooth():
            ms = []
            for _ in range(repeats):
                XS.copy_(plan)
                ms.append(timed(smooth, 1))
            return float(np.median(ms))
        for fn in (e.calc_diff, filt, smooth):
            XS.copy_(plan)
            fn()
            torch.cuda.synchronize()
        assert all(bool(torch.isfinite(t).all()) for t in (ev, kg, xs, xf, nis, nll, step)), name
        XS.copy_(plan)
        t_calc, t_filt = timed(e.calc_diff, repeats), timed(filt, repeats)
        t_smooth = timed_smooth()
        print("%s B=%d T=%d nx=%d ny=%d: calc_diff %.3f ms, filter only %.3f ms (sweep %.3f ms), smooth %.3f ms (sweeps %.3f ms, "
              "%.2f x the filter-alone sweep); step %.2e" % (name, e.B, e.T, e.nx, ny, t_calc, t_filt, t_filt - t_calc, t_smooth,
                                                           t_smooth - t_calc, (t_smooth - t_calc) / (t_filt - t_calc), float(step.max())))
        e.close()


def experiment():
    B, T, nj = 64, 100, 2
    rng = np.random.default_rng(0)
    sc = scenarios.two_dof_sea(B=B, T=T, seed=0)
    model = crocoddyl.ShootingProblem(sc["x0"], sc["running"], sc["terminal"], frame_refs=sc["frame_refs"])
    k0 = np.array([float(model.runningModels[0].differential.K[j, j]) for j in range(nj)])
    b0 = np.array([float(model.runningModels[0].differential.B[j, j]) for j in range(nj)])
    true_k, true_b = k0 * rng.uniform(0.8, 1.2, (B, nj)), b0 * rng.uniform(0.8, 1.2, (B, nj))
    plant = crocoddyl.ShootingProblem(sc["x0"], sc["running"], sc["terminal"], frame_refs=sc["frame_refs"], stiffness=true_k,
                                      motor_inertia=true_b)
    us = rng.uniform(-1.0, 1.0, (B, T, 2))
    xs = plant.rollout(us).cpu().numpy()
    sigma = 1e-4
    ys = xs[:, :, :2 * nj] + sigma * rng.standard_normal((B, T + 1, 2 * nj))
    dt = float(model.runningModels[0].dt)
    v = (ys[:, 1:] - ys[:, :-1]) / dt
    fd = np.concatenate([ys, np.concatenate([v, v[:, -1:]], axis=1)], axis=2)
    bounds = dict(stiffness_bounds=(0.2 * k0, 5.0 * k0), motor_inertia_bounds=(0.2 * b0, 5.0 * b0))

    def fit(states):
        p = crocoddyl.ShootingProblem(sc["x0"], sc["running"], sc["terminal"], frame_refs=sc["frame_refs"])
        r = p.identify_plant(states, us, n_steps=16, **bounds)
        err = np.concatenate([r.stiffness.cpu().numpy() / true_k - 1.0, r.motor_inertia.cpu().numpy() / true_b - 1.0], axis=1)
        return np.median(np.abs(err)), np.abs(err).max()
    est = model.estimate_states(ys, us, sigma ** 2, sigma0=np.diag([sigma ** 2] * (2 * nj) + [(2 * sigma / dt) ** 2] * (2 * nj)),
                                noise_var=np.array([1e-8] * (2 * nj) + [1e-4] * (2 * nj)), n_iters=5)
    torch.cuda.synchronize()
    print("experiment two_dof_sea B=%d T=%d, parameters 20 %% off, encoder noise %.0e rad: step_norm per iteration %s"
          % (B, T, sigma, " ".join("%.1e" % s for s in est.step_norm.max(dim=0).values.cpu().numpy())))
    print("  state error, max |x - true| / max |true|: smoothed %.2e, finite differences %.2e"
          % (np.abs(est.xs.cpu().numpy() - xs).max() / np.abs(xs).max(), np.abs(fd - xs).max() / np.abs(xs).max()))
    for what, states in (("smoothed states", est.xs), ("finite-difference states", fd)):
        print("  identify_plant on %s: relative parameter error median %.2e, worst %.2e" % ((what,) + fit(states)))


if __name__ == "__main__":
    times(int(sys.argv[1]) if len(sys.argv) > 1 else 20)
    experiment()
