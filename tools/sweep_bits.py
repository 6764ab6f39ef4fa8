"""A SHA-1 of every output array of the five team-sweep kernels (aslr_sweep_team.hpp), to compare two builds of the library
bit for bit: tools/sweep_bits.py, once per build, each in a process of its own; ASLR_LIB_OVERRIDE names the library of a
run (default: the product library).  The two printouts must be identical.

For each of the four handle sizes a small seeded batch (B = 5 at nx = 8, B = 3 at nx = 28: no multiple of the teams of a wave;
T = 4) on the plan two solver iterations from a cold start leave, so that the arms move and K is not zero; then
  aslr_cost_sensitivity            every output;
  aslr_policy_covariance           every output;
  aslr_policy_lqg                  every output, with the positions measured and with every entry measured;
  aslr_policy_plant_sensitivity    every output the model has, and (SEA) once more with the motor-inertia columns alone;
  aslr_debug_identify_normal       the work buffer, and (SEA) once more without the stiffness columns.
One line per output array.  An array whose entries are all the same number could not tell two builds apart: it is marked
CONSTANT and the run ends with status 1."""
import ctypes as C
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aslr_to_amd import _abi  # noqa: E402
if os.environ.get("ASLR_LIB_OVERRIDE"):
    _abi.lib_path = lambda: os.path.abspath(os.environ["ASLR_LIB_OVERRIDE"])

import torch  # noqa: E402

from _timing import planned, ptr, seeded_spread  # noqa: E402
from aslr_to_amd import scenarios  # noqa: E402

CONSTANT = []
SIZES = {"two_dof_sea": 5, "two_dof_vsa_boxddp": 5, "talos_arm_sea": 3, "talos_arm_vsa": 3}
T = 4


def main():
    for name, B in SIZES.items():
        e, _ = planned(lambda: scenarios.SCENARIOS[name](B=B, T=T, seed=0), 2)
        nx, nu, nj, sea = e.nx, e.nu, e.nx // 4, e.low.dam == _abi.DAM_SEA
        gen = torch.Generator(device="cpu").manual_seed(0)
        new = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device=e.device)
        s0, w, r = seeded_spread(e, gen)
        var = lambda: (0.1 + 0.9 * torch.rand((nj, B), generator=gen, dtype=torch.float64)).to(e.device)
        vk, vb = (var() if sea else None), var()

        def line(tag, k, t):
            v = t.cpu().numpy()
            flat = bool((v == v.flat[0]).all()) or not bool(torch.isfinite(t).all())
            CONSTANT.append((name, tag, k)) if flat else None
            print("%s %s %s %s%s" % (name, tag, k, hashlib.sha1(v.tobytes()).hexdigest(), " CONSTANT" if flat else ""))

        def run(tag, fn, *args, **outs):
            e._call(fn, *[ptr(a) if a is None or torch.is_tensor(a) else a for a in args], e._stream())
            torch.cuda.synchronize()
            for k, t in outs.items():
                line(tag, k, t)

        dk, db, dx0, lam = (new(nj, B) if sea else None), new(nj, B), new(nx, B), new(T + 1, B, nx)
        run("adjoint", "aslr_cost_sensitivity", dk, db, dx0, lam, **dict(d_motor_inertia=db, d_x0=dx0, costate=lam, **({"d_stiffness": dk} if sea else {})))

        xv, uv, cf, cov, ci = new(T + 1, B, nx), new(T, B, nu), new(B, nx, nx), new(T + 1, B, nx, nx), new(B)
        run("covariance", "aslr_policy_covariance", s0, w, xv, uv, cf, cov, ci, x_var=xv, u_var=uv, cov_final=cf, cov=cov, cost_increase=ci)

        for tag, ny in (("lqg-positions", nx // 2), ("lqg-all", nx)):
            xv, uv, ev, ci = new(T + 1, B, nx), new(T, B, nu), new(T + 1, B, nx), new(B)
            cf, ef, kg = new(B, nx, nx), new(B, nx, nx), new(T + 1, B, nx, ny)
            run(tag, "aslr_policy_lqg", ny, None, r[:, :ny].contiguous(), s0, w, xv, uv, ev, cf, ef, kg, ci,
                x_var=xv, u_var=uv, est_var=ev, cov_final=cf, est_cov_final=ef, kalman_gain=kg, cost_increase=ci)

        for tag, stiff in (("plant_sens-stiff", True), ("plant_sens-motor", False)) if sea else (("plant_sens-motor", False),):
            k = lambda *s: new(*s) if stiff else None
            tk, fk, ck = k(T + 1, B, nx, nj), k(B, nx, nj), k(nj, B)
            tb, fb, cb, xv, uv = new(T + 1, B, nx, nj), new(B, nx, nj), new(nj, B), new(T + 1, B, nx), new(T, B, nu)
            outs = dict(dx_b=tb, dxT_b=fb, dcost_b=cb, x_var=xv, u_var=uv)
            if stiff:
                outs.update(dx_k=tk, dxT_k=fk, dcost_k=ck)
            run(tag, "aslr_policy_plant_sensitivity", vk if stiff else None, vb, tk, tb, fk, fb, ck, cb, xv, uv, **outs)

        e.lib.aslr_debug_identify_normal.restype = C.c_int
        e.lib.aslr_debug_identify_normal.argtypes = [C.c_void_p, C.POINTER(_abi.Identify), C.c_void_p]
        for tag, stiff in (("identify-stiff", True), ("identify-motor", False)) if sea else (("identify-motor", False),):
            npar = 2 * nj if stiff else nj
            work = new(2 * npar + 1 + npar * (npar + 1) // 2, B)
            work[:npar] = 0.0  # (the candidate's rows: the kernel writes the rows after them)
            d = _abi.Identify(n_steps=1, fit_stiffness=int(stiff), fit_motor_inertia=1)
            d.work = work.data_ptr()
            _abi.check(e.lib.aslr_debug_identify_normal(e.handle, C.byref(d), e._stream()), "aslr_debug_identify_normal")
            torch.cuda.synchronize()
            line(tag, "work", work[npar:])
        e.close()
    sys.exit(1 if CONSTANT else 0)


if __name__ == "__main__":
    main()
