"""Scenes, poses and closed forms shared by tests/test_render_cpu.py and tests/test_render_gpu.py."""
import numpy as np

import mjx_amd
from mjx_amd import mjcf

# A fixed camera 3 m in front of (0, 0, 1), looking along +y with z up; a floor; one free body at (0, 0, 1).
_KAT = """<mujoco><visual><map znear="0.01" zfar="30"/></visual><worldbody>
  <light pos="0 -4 5" diffuse=".8 .8 .8"/>
  <camera name="cam" pos="0 -3 1" xyaxes="1 0 0 0 0 1" fovy="45"/>
  <geom name="floor" type="plane" size="0 0 .05"/>
  <body name="obj" pos="0 0 1"><freejoint/>%s</body>
</worldbody></mujoco>"""
SPHERE_R, CAPSULE_R, CAPSULE_H, KAT_D, KAT_CAM_Z, KAT_FOVY = 0.25, 0.1, 0.6, 3.0, 1.0, 45.0
SPHERE_XML = _KAT % '<geom type="sphere" size=".25" rgba=".9 .2 .2 1"/>'
CAPSULE_XML = _KAT % '<geom type="capsule" fromto="-.6 0 0 .6 0 0" size=".1" rgba=".2 .9 .2 1"/>'

# One camera of each mode: `fix` on a hinged arm, `trk` (track) and `com` (trackcom) on the free base.
MODES_XML = """<mujoco><worldbody>
  <light pos="0 -6 4" diffuse=".8 .8 .8"/>
  <geom name="floor" type="plane" size="0 0 .05" rgba=".3 .4 .5 1"/>
  <body name="base" pos="0 0 1"><freejoint/>
    <camera name="trk" pos="0 -3 .2" xyaxes="1 0 0 0 0 1" mode="track"/>
    <camera name="com" pos="0 -3 .2" xyaxes="1 0 0 0 0 1" mode="trackcom"/>
    <geom type="capsule" fromto="0 0 -.3 0 0 .3" size=".1" rgba=".8 .6 .4 1"/>
    <body name="arm" pos="0 0 .3">
      <joint name="sh" type="hinge" axis="0 1 0" pos="0 0 0"/>
      <geom type="capsule" fromto="0 0 0 .5 0 0" size=".05" rgba=".2 .6 .9 1"/>
      <geom type="sphere" pos=".5 0 0" size=".09" rgba=".9 .9 .2 1"/>
      <camera name="fix" pos="0 -2 .1" xyaxes="1 0 0 0 0 1" fovy="60"/>
    </body>
  </body>
</worldbody></mujoco>"""


def humanoid():
    return mjx_amd.load_model("humanoid_mjx")


def humanoid_poses(m):
    """qpos0; two poses with every hinge drawn inside its range (fixed seed); one lying on the floor
    (root z 0.2, root quaternion tilted ~80 degrees about y and 20 about z)."""
    rng = np.random.default_rng(20251019)
    A = m.arrays
    poses = [m.qpos0.copy()]
    for _ in range(2):
        q = m.qpos0.copy()
        for j in range(m.njnt):
            if A["jnt_type"][j] == mjcf.JNT_HINGE:
                lo, hi = A["jnt_range"][j]
                q[A["jnt_qposadr"][j]] = rng.uniform(lo, hi)
        poses.append(q)
    q = poses[1].copy()
    q[2] = 0.2
    q[3:7] = mjcf.quat_mul(mjcf.axis_angle_quat([0, 0, 1.0], np.deg2rad(20)), mjcf.axis_angle_quat([0, 1.0, 0], np.deg2rad(80)))
    poses.append(q)
    return poses


def pixel_dir(i, j, W, H, fovy=KAT_FOVY):
    """Unit direction in the KAT camera's world (x right, y forward, z up) of pixel (column i, row j)."""
    th = np.tan(0.5 * np.deg2rad(fovy))
    u = (2 * (i + 0.5) / W - 1) * th * W / H
    v = (1 - 2 * (j + 0.5) / H) * th
    d = np.array([u, 1.0, v])
    return d / np.linalg.norm(d)


def sphere_depth(d, centre, r, cam=(0.0, -KAT_D, KAT_CAM_Z)):
    """Law of cosines: with D the distance to the centre and a the angle between the ray and the line
    to it, the first crossing is D cos a - sqrt(r^2 - D^2 sin^2 a)."""
    c = np.asarray(centre, float) - np.asarray(cam)
    D = np.linalg.norm(c)
    ca = float(np.dot(c, d)) / D
    return D * ca - np.sqrt(r * r - D * D * (1 - ca * ca))


def floor_depth(d):
    return KAT_CAM_Z / -d[2]


def xcylinder_depth(d, r=CAPSULE_R):
    """A cylinder about the x axis through (0, 0, 1): the (y, z) components of the ray from (-3, 0)
    relative to the axis reach radius r at the smaller root of (dy^2 + dz^2) t^2 - 6 dy t + 9 - r^2 = 0."""
    a, b, c = d[1] ** 2 + d[2] ** 2, -2 * KAT_D * d[1], KAT_D ** 2 - r * r
    return (-b - np.sqrt(b * b - 4 * a * c)) / (2 * a)
