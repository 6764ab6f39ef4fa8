"""What the timing tools of the extension calls share (tools/time_covariance.py, time_lqg.py, time_plant_sens.py,
time_sensitivity.py, time_policy.py, time_policy_team.py, time_policy_noise.py): the HIP-event median, the three standard
shapes, the handle on a plan, the seeded spread of the covariance calls and the pointer of a tensor.  Importing it puts the
repository root on sys.path, so a tool imports it before aslr_to_amd."""
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from aslr_to_amd import scenarios
from aslr_to_amd.engine import Engine

STANDARD_SHAPES = {"two_dof_vsa_boxddp": lambda: scenarios.two_dof_vsa_boxddp(B=4096, T=100, seed=0),
                   "talos_arm_sea": lambda: scenarios.talos_arm_sea(B=512, T=150, seed=0),
                   "talos_arm_vsa": lambda: scenarios.talos_arm_vsa(B=512, T=150, seed=0)}


def timed(fn, repeats):
    ms = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    return statistics.median(ms)


def planned(make, iterations=5):
    """-> engine, solver parameters: the scenario make() on a new handle after `iterations` solver iterations from a cold
    start (0: the empty candidate with aslr_calc_diff and one backward sweep on it), synchronised.  The lowered problem is
    e.low."""
    sc = make()
    sp = scenarios.solver_params(sc)
    e = Engine(scenarios.lower(sc))
    e.set_candidate(None, None)
    if iterations:
        e.iterate_n(sp, True, iterations)
        e.finalize()
    else:
        e.calc_diff()
        e.backward_pass(sp)
    torch.cuda.synchronize()
    return e, sp


def seeded_spread(e, gen=None):
    """-> sigma0 [B, nx, nx] = M M^T + 0.1 I with M ~ U(-1, 1), noise_var [T, B, nx] ~ U(0.1, 1) and a pool of meas_var
    [B, nx] ~ U(0.1, 1) (its first ny columns: [B][ny]) on the engine's device, drawn in this order from `gen` (default: a CPU
    generator with seed 0)"""
    gen = torch.Generator(device="cpu").manual_seed(0) if gen is None else gen
    m = torch.rand((e.B, e.nx, e.nx), generator=gen, dtype=torch.float64) * 2 - 1
    s0 = (m @ m.transpose(1, 2) + 0.1 * torch.eye(e.nx, dtype=torch.float64)).to(e.device)
    w = (0.1 + 0.9 * torch.rand((e.T, e.B, e.nx), generator=gen, dtype=torch.float64)).to(e.device)
    r = (0.1 + 0.9 * torch.rand((e.B, e.nx), generator=gen, dtype=torch.float64)).to(e.device)
    return s0, w, r


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())
