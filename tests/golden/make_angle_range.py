"""Generate tests/golden/angle_range_v1.npz: world placements of every frame of three chains at the E, Q and W points of
tests/_angle_range.py, from the 40-digit reference of tests/_hp_geometry.py (Chain.kinematics: joint rotations as
exponentials, mpmath's own argument reduction), each entry rounded once to float64.

    python tests/golden/make_angle_range.py

The chains: the planar asr_twodof arm of C2 / C3, the `general` chain of tests/_geometry_chains.py, and the 7-joint arm,
over whose joints the sets go cyclically.  Per chain the file holds the frames (name, joint, local R, local p; asr_twodof's
"joint1" is the first joint's own frame, whose world rotation is a single sine and cosine) and, per point set, the link
angles q [n, nj] and the expected R [frames, n, 3, 3] and p [frames, n, 3].  The points are chosen with the CPU oracle
(the bound on the frame-placement residual rotation); the expected values do not depend on it.
tests/test_angle_range_host.py regenerates the file where mpmath imports and requires equality; the GPU test reads it and
needs no mpmath.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import _angle_range as ar  # noqa: E402
import _geometry_chains as chains  # noqa: E402
from aslr_to_amd import scenarios  # noqa: E402

FILE = os.path.join(HERE, "angle_range_v1.npz")
CHAINS = ("asr_twodof", "general", "talos_arm")
SETS = tuple("E_" + k for k in ar.EDGE_LAYOUTS) + ("Q", "W")
N_QW = 70
SEED = 21


def problem(name):
    """the scenario whose chain, cost frame and reference give the bound on the residual rotation"""
    if name == "asr_twodof":
        return scenarios.two_dof_sea(B=1, T=1)
    if name == "general":
        return chains.problem("general", "sea", B=1, T=1)
    return scenarios.talos_arm_sea(B=1, T=1)


def frames_of(model):
    """(name, joint, R, p) of every frame that sits on a joint"""
    return [(f.name, f.parent, np.array(f.placement.rotation, dtype=float), np.array(f.placement.translation, dtype=float))
            for f in model.frames if f.parent >= 0]


def points(oracle, name):
    """-> model, {set: q [n, nj]}, share of redrawn Q points"""
    sc = problem(name)
    low = scenarios.lower(sc)
    rot = lambda q: ar.point_rotation(oracle, low, q)
    pts = {"E_" + k: ar.edge_points(k, low.nj, rot) for k in ar.EDGE_LAYOUTS}
    pts["Q"], share = ar.quadrant_points(oracle, low, SEED, N_QW)
    pts["W"], _ = ar.wound_points(low.nj, SEED, N_QW)
    return sc["terminal"].state.pinocchio, low, pts, share


def expected(model, frames, q):
    """R [frames, n, 3, 3], p [frames, n, 3] at 40 digits, rounded once"""
    import mpmath as mp
    import _hp_geometry as hp
    R, p = np.zeros((len(frames), len(q), 3, 3)), np.zeros((len(frames), len(q), 3))
    with mp.workdps(hp.DPS):
        ch = hp.Chain(model)
        placed = [(hp._mpf_matrix(fR), hp._vec(fp)) for _, _, fR, fp in frames]
        for i, qi in enumerate(q):
            kin = ch.kinematics(hp._vec(qi))
            for f, (_, joint, _, _) in enumerate(frames):
                Rj, pj = kin[joint]
                R[f, i] = hp.to_np(Rj * placed[f][0])
                p[f, i] = hp.to_np(pj + Rj * placed[f][1])
    return R, p


def build(oracle):
    out = {}
    for name in CHAINS:
        model, _, pts, share = points(oracle, name)
        frames = frames_of(model)
        out[name + "/frame_names"] = np.array([f[0] for f in frames])
        out[name + "/frame_joint"] = np.array([f[1] for f in frames], dtype=np.int32)
        out[name + "/frame_R"] = np.array([f[2] for f in frames])
        out[name + "/frame_p"] = np.array([f[3] for f in frames])
        out[name + "/Q_redrawn"] = np.array(share)
        for key in SETS:
            out["%s/%s/q" % (name, key)] = pts[key]
            out["%s/%s/R" % (name, key)], out["%s/%s/p" % (name, key)] = expected(model, frames, pts[key])
    return out


def main():
    from oracle import pyoracle
    pyoracle.lib()
    out = build(pyoracle)
    np.savez_compressed(FILE, **out)
    print("wrote %d arrays, %d bytes" % (len(out), os.path.getsize(FILE)))


if __name__ == "__main__":
    main()
