"""Shared by tests/test_gpu_mpc.py and tools/time_mpc.py: the receding-horizon loop driven from Python through the entry
points that existed before aslr_mpc_run -- solve, calc, torch shifts of the XS / US / X0 / KFF / GAPS / VXXF region views.
It states the semantics of aslr_mpc_run by composition; the device loop must reproduce it bit for bit."""
from aslr_to_amd import _abi


def host_driven_mpc(e, sp, n_steps, first_maxiter, iters_per_step, disturbance=None):
    """e: an Engine whose candidate is set; disturbance: device tensor [n_steps, B, nx] (time-major) or None.
    -> dict of time-major device tensors: x_closed [n+1, B, nx], u_closed [n, B, nu], stat_f [n, 4, B] (cost, stop,
    x_reg, step), stat_i [n, 2, B] (iterations, status).  No synchronisation inside."""
    import torch
    X, U, X0, XN = (e.region(r) for r in (_abi.R_XS, _abi.R_US, _abi.R_X0, _abi.R_XNEXT))
    TF, TI = e.region(_abi.R_TRAJ_F), e.region(_abi.R_TRAJ_I)
    zeroed = [e.region(r) for r in (_abi.R_KFF, _abi.R_GAPS, _abi.R_VXXF)]
    xc, uc, sf, si = [], [], [], []
    keep = sp.maxiter
    try:
        for s in range(n_steps):
            sp.maxiter = first_maxiter if s == 0 else iters_per_step
            e.solve(sp, poll_every=0)
            e.calc()
            xc.append(X[0].clone())
            uc.append(U[0].clone())
            sf.append(TF[[_abi.TF_COST, _abi.TF_STOP, _abi.TF_XREG, _abi.TF_STEP]].clone())
            si.append(TI[[_abi.TI_ITER, _abi.TI_STATUS]].clone())
            xp = XN[0].clone() if disturbance is None else XN[0] + disturbance[s]
            X[:-1] = X[1:].clone()
            U[:-1] = U[1:].clone()
            X[0] = xp
            X0.copy_(xp)
            for z in zeroed:
                z.zero_()
        xc.append(xp)
    finally:
        sp.maxiter = keep
    return dict(x_closed=torch.stack(xc), u_closed=torch.stack(uc), stat_f=torch.stack(sf), stat_i=torch.stack(si))
