"""Two-joint chains whose geometry the synthetic robot tables do not have, loaded through the URDF loader, and SEA / VSA
problems on them with the C2 / C3 cost stacks and actuator constants of scenarios.SPECS.

- general: axes (0, 1, 0) and (1, 0, 1)/sqrt(2), joint origins with rpy and xyz, inertial origins with rpy (full inertia
  tensors), an end-effector welded by a fixed joint with a rotated origin, gravity with three non-zero components;
- flipped: the planar arm of the C2 / C3 table with axes -z (physically planar; the planar detector declines it);
- tilted: +z axes with a 1e-3 rad x-tilt of joint 2's origin (the planar detector declines it).
Test helpers only: example_robot_data's tables are tied to the golden fixtures and stay as they are.
"""
import numpy as np

from aslr_to_amd import pinocchio, scenarios
from aslr_to_amd.models import (ASRActuation, DifferentialFreeASRFwdDynamicsModel, DifferentialFreeFwdDynamicsModelVSA,
                                IntegratedActionModelEulerASR, StateMultibodyASR, VSAASRActuation)

GENERAL_URDF = """
<robot name="general_2r">
  <link name="base_link"/>
  <link name="link1"><inertial><origin xyz="0.06 0.012 -0.018" rpy="0.4 0.1 -0.3"/><mass value="0.3"/>
    <inertia ixx="2.1e-4" ixy="1.2e-5" ixz="-2.3e-5" iyy="4.9e-4" iyz="3.1e-5" izz="4.4e-4"/></inertial></link>
  <link name="link2"><inertial><origin xyz="0.05 -0.011 0.016" rpy="-0.2 0.3 0.25"/><mass value="0.2"/>
    <inertia ixx="1.3e-4" ixy="-0.8e-5" ixz="1.1e-5" iyy="2.6e-4" iyz="-1.7e-5" izz="2.2e-4"/></inertial></link>
  <link name="EE"/>
  <joint name="joint1" type="revolute"><parent link="base_link"/><child link="link1"/>
    <origin xyz="0.02 -0.03 0.18" rpy="0.3 -0.2 0.5"/><axis xyz="0 1 0"/></joint>
  <joint name="joint2" type="revolute"><parent link="link1"/><child link="link2"/>
    <origin xyz="0.135 0.01 -0.02" rpy="-0.25 0.35 0.1"/><axis xyz="1 0 1"/></joint>
  <joint name="ee_fixed" type="fixed"><parent link="link2"/><child link="EE"/>
    <origin xyz="0.12 -0.0002 0.01" rpy="0.2 -0.4 0.7"/></joint>
</robot>
"""

# the C2 / C3 arm (example_robot_data._asr_twodof: rods of 0.135 / 0.12 m, 0.3 / 0.2 kg) with both axes -z
FLIPPED_URDF = """
<robot name="flipped_2r">
  <link name="base_link"/>
  <link name="link1"><inertial><origin xyz="0.0675 -0.001 0"/><mass value="0.3"/>
    <inertia ixx="1e-5" iyy="4.55625e-4" izz="4.55625e-4"/></inertial></link>
  <link name="link2"><inertial><origin xyz="0.06 -0.001 0"/><mass value="0.2"/>
    <inertia ixx="1e-5" iyy="2.4e-4" izz="2.4e-4"/></inertial></link>
  <link name="EE"/>
  <joint name="joint1" type="revolute"><parent link="base_link"/><child link="link1"/>
    <origin xyz="0 0 0.18"/><axis xyz="0 0 -1"/></joint>
  <joint name="joint2" type="revolute"><parent link="link1"/><child link="link2"/>
    <origin xyz="0.135 0 0"/><axis xyz="0 0 -1"/></joint>
  <joint name="ee_fixed" type="fixed"><parent link="link2"/><child link="EE"/><origin xyz="0.12 -2.03063311e-04 0"/></joint>
</robot>
"""

TILTED_URDF = FLIPPED_URDF.replace('name="flipped_2r"', 'name="tilted_2r"').replace('xyz="0 0 -1"', 'xyz="0 0 1"').replace(
    '<origin xyz="0.135 0 0"/>', '<origin xyz="0.135 0 0" rpy="0.001 0 0"/>')

URDFS = {"general": GENERAL_URDF, "flipped": FLIPPED_URDF, "tilted": TILTED_URDF}
GRAVITY = {"general": (1.7, -2.4, -9.3), "flipped": (9.81, 0.0, 0.0), "tilted": (9.81, 0.0, 0.0)}
CHAINS = tuple(URDFS)


def chain(name):
    m = pinocchio.buildModelFromUrdf(URDFS[name])
    m.gravity.linear = np.array(GRAVITY[name], dtype=float)
    return m


def problem(chain_name, actuator, B, T, seed=0):
    """A scenario dict (scenarios' layout) on chain `chain_name`: actuator "sea" takes two_dof_sea's spec (C2), "vsa"
    two_dof_vsa_boxddp's (C3: box-limited controls, stiffness regularised by the control cost)."""
    spec = scenarios.SPECS["two_dof_sea" if actuator == "sea" else "two_dof_vsa_boxddp"]
    model = chain(chain_name)
    state = StateMultibodyASR(model)
    nj = model.nv
    if actuator == "vsa":
        actuation = VSAASRActuation(state)
        nu = 2 * actuation.nu
    else:
        actuation = ASRActuation(state)
        nu = actuation.nu
    frame_id = model.getFrameId(spec["frame"])
    assert frame_id < len(model.frames)
    stacks = [scenarios._cost_stack(spec[k], state, nu, nj, frame_id, spec["target"]) for k in ("running", "terminal")]

    def differential(costs):
        if actuator == "vsa":
            return DifferentialFreeFwdDynamicsModelVSA(state, actuation, costs, spec["motor_inertia"] * np.eye(nj))
        return DifferentialFreeASRFwdDynamicsModel(state, actuation, costs, spec["stiffness"] * np.eye(nj),
                                                   spec["motor_inertia"] * np.eye(nj))

    running = IntegratedActionModelEulerASR(differential(stacks[0]), spec["dt"])
    terminal = IntegratedActionModelEulerASR(differential(stacks[1]), 0)
    if "u_lb" in spec:
        running.u_lb = np.array(spec["u_lb"], dtype=float)
        running.u_ub = np.array(spec["u_ub"], dtype=float)
    x0, refs = scenarios._batch_inputs(B, seed, nj, np.array(spec["target"], dtype=float))
    return dict(x0=x0, running=[running] * T, terminal=terminal, frame_refs=refs, solver=spec["solver"],
                maxiter=spec["maxiter"], th_stop=spec["th_stop"], name="%s_%s" % (chain_name, actuator))


def random_rotation(rng, angle=None):
    """A rotation about a random unit axis, by a random angle in [0, pi) or the given one (Rodrigues, float64)."""
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    t = rng.uniform(0.0, np.pi) if angle is None else float(angle)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1.0 - np.cos(t)) * K.dot(K)
