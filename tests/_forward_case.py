"""Shared by the kernel-level forward-pass tests (tests/test_gpu_geometry.py, tests/test_gpu_forward_seam.py): one recipe
for the inputs of aslr_forward_pass -- a random candidate, gaps drawn from U(-0.05, 0.05), gains from the oracle's backward
pass scaled by 0.05 so that the rollout of every step length stays finite -- and the engine run on them."""
import numpy as np

from aslr_to_amd import _abi

SOLVERS = {"SolverDDP": _abi.SOLVER_DDP, "SolverFDDP": _abi.SOLVER_FDDP, "SolverBoxDDP": _abi.SOLVER_BOXDDP}


def random_candidate(low, seed):
    rng = np.random.default_rng(seed)
    xs = rng.uniform(-0.8, 0.8, (low.T + 1, low.B, low.nx))
    us = rng.uniform(-1.0, 1.0, (low.T, low.B, low.nu))
    if low.dam == _abi.DAM_VSA:
        us[..., low.nu // 2:] = rng.uniform(0.1, 5.0, (low.T, low.B, low.nu // 2))
    return xs, us


def forward_inputs(oracle, low, sp, seed, fddp, feasible=None, full=False):
    """-> xs, us, K, k, gaps (full: also the oracle's backward pass the gains come from, with its unscaled Vxx).  fddp: the
    backward pass runs infeasible, so that its value function carries the gap terms; feasible: one flag per trajectory
    instead."""
    xs, us = random_candidate(low, seed)
    _, _, deriv = oracle.calc_diff(low, xs, us)
    rng = np.random.default_rng(seed + 7)
    gaps = rng.uniform(-0.05, 0.05, (low.T + 1, low.B, low.nx))
    if feasible is None:
        feasible = 0 if fddp else 1
    ref_b = oracle.backward_pass(low, sp, deriv, gaps, us, 1e-3, feasible)
    out = (xs, us, 0.05 * ref_b["K"], 0.05 * ref_b["k"], gaps)   # mild gains keep every alpha's rollout finite
    return out + (ref_b,) if full else out


def run_forward(low, sp, xs, us, K, k, gaps, feasible, vxxf=None):
    """A fresh engine (it reads the environment switches now), the inputs in place, aslr_forward_pass.  feasible: one
    value or one per trajectory; vxxf: R_VXXF, the `Vxx f` the FDDP rollout reads for its dv."""
    import torch
    from aslr_to_amd.engine import Engine
    e = Engine(low)
    e.region(_abi.R_XS).copy_(torch.as_tensor(xs))
    e.region(_abi.R_US).copy_(torch.as_tensor(us))
    e.region(_abi.R_KGAIN).copy_(torch.as_tensor(K))
    e.region(_abi.R_KFF).copy_(torch.as_tensor(k))
    e.region(_abi.R_GAPS).copy_(torch.as_tensor(gaps))
    if vxxf is not None:
        e.region(_abi.R_VXXF).copy_(torch.as_tensor(vxxf))
    if np.ndim(feasible):
        e.region(_abi.R_TRAJ_I)[_abi.TI_FEASIBLE].copy_(torch.as_tensor(np.asarray(feasible, dtype=np.int32)))
    else:
        e.region(_abi.R_TRAJ_I)[_abi.TI_FEASIBLE].fill_(int(feasible))
    e.forward_pass(sp)
    torch.cuda.synchronize()
    return e
