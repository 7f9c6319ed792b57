"""Numpy reference of mjl_jac_dot / mjl_centroidal (include/mjx355.h), in float64 or, with dtype=np.float32, in the
kernel's precision (the tolerance yardstick of tests/test_taskspace_gpu.py). Built on dyn_ref.dof_axes / jac and
one oracle forward output o = state_arrays(m, orc.forward(...)), of which xpos, xquat, xipos and qpos are read.
The rates of a dof's axis and anchor are plain sums over the dof's ancestors along dof_parentid (no tree
recursion); the centroidal matrices are plain sums of body Jacobians over the subtree (no composites), the bias
the same sums of the bodies' velocity-product accelerations. tests/test_taskspace.py checks all of it against
central differences of dyn_ref.jac along the motion."""
import numpy as np

from mjx_amd import mjcf

import dyn_ref as dr

# tests/test_dyn_gpu.py's two-tree model: a free 3-link hinge chain and a second free sphere
TWO_TREES = """
<mujoco model="two_trees">
  <option timestep="0.004"/>
  <worldbody>
    <geom name="floor" type="plane" size="0 0 1"/>
    <body name="a0" pos="0 0 1"><freejoint/>
      <geom type="capsule" fromto="0 0 0 0.2 0 0" size="0.03"/>
      <body name="a1" pos="0.2 0 0">
        <joint name="h1" type="hinge" axis="0 1 0" pos="0.01 0 0" armature="0.02"/>
        <geom type="capsule" fromto="0 0 0 0.2 0 0.05" size="0.03"/>
        <body name="a2" pos="0.2 0 0.05" quat="0.9 0.1 0.3 -0.2">
          <joint name="h2" type="hinge" axis="1 0 0.3"/>
          <geom type="capsule" fromto="0 0 0 0.15 0.05 0" size="0.025"/>
          <body name="a3" pos="0.15 0.05 0">
            <joint name="h3" type="hinge" axis="0 0 1" pos="0 0.01 0"/>
            <geom type="capsule" fromto="0 0 0 0.1 0.1 0.1" size="0.02"/>
            <site name="tip" pos="0.1 0.1 0.1" quat="0.7 0.1 -0.5 0.5" size="0.01"/>
          </body>
        </body>
      </body>
    </body>
    <body name="ball" pos="0.5 0.5 1"><freejoint/><geom type="sphere" size="0.1"/></body>
  </worldbody>
  <actuator><motor name="m1" joint="h1" gear="5"/></actuator>
</mujoco>
"""


def _f(x, dtype):
    return np.asarray(x, np.float64).astype(dtype)


def dof_rates(m, o, qvel, dtype=np.float64, axes=None):
    """Per dof (da/dt, dp/dt) of dyn_ref.dof_axes' axis and anchor along the motion with rate qvel."""
    A = m.arrays
    axes = dr.dof_axes(m, o, dtype) if axes is None else axes
    qv = _f(qvel, dtype)
    out = [None] * m.nv
    for d in range(m.nv):
        kind, a, p = axes[d]
        j = int(A["dof_jntid"][d])
        if A["jnt_type"][j] == mjcf.JNT_FREE:
            d0 = int(A["jnt_dofadr"][j])
            if d - d0 < 3:
                out[d] = (np.zeros(3, dtype), np.zeros(3, dtype))
                continue
            w = sum(axes[d0 + 3 + i][1] * qv[d0 + 3 + i] for i in range(3))  # R_b qvel_rot: all three rates
            out[d] = (np.cross(w, a).astype(dtype), qv[d0:d0 + 3].copy())
            continue
        w, v = np.zeros(3, dtype), np.zeros(3, dtype)
        e = int(A["dof_parentid"][d])
        while e >= 0:  # the dofs that precede d on its chain
            ke, ae, pe = axes[e]
            if ke == 1:
                v = v + ae * qv[e]
            else:
                w = w + ae * qv[e]
                v = v + np.cross(ae, p - pe) * qv[e]
            e = int(A["dof_parentid"][e])
        out[d] = (np.cross(w, a).astype(dtype), v.astype(dtype))
    return out


def jac_dot(m, o, body, x, qvel, dtype=np.float64, axes=None, rates=None):
    """(jacp_dot, jacr_dot [3, nv], jdotv [6]) of the world point x carried by (and fixed in) `body`."""
    axes = dr.dof_axes(m, o, dtype) if axes is None else axes
    rates = dof_rates(m, o, qvel, dtype, axes) if rates is None else rates
    x, qv = _f(x, dtype), _f(qvel, dtype)
    jp, _ = dr.jac(m, o, body, x, dtype, axes)
    xd = jp @ qv
    jpd, jrd = np.zeros((3, m.nv), dtype), np.zeros((3, m.nv), dtype)
    for d in dr.body_dofs(m, body):
        kind, a, p = axes[d]
        if kind == 1:
            continue
        ad, pd = rates[d]
        jrd[:, d] = ad
        jpd[:, d] = np.cross(ad, x - p) + np.cross(a, xd - pd)
    return jpd, jrd, np.concatenate([jpd @ qv, jrd @ qv])


def world_inertia(m, o, inertia=None, dtype=np.float64):
    """[nbody, 3, 3]: R_k T_k R_k' of the body-frame tensors."""
    ten = _f(m.arrays["body_inertia"] if inertia is None else inertia, dtype).reshape(m.nbody, 6)
    out = np.zeros((m.nbody, 3, 3), dtype)
    for b in range(1, m.nbody):
        R, t = dr._q2m(_f(o["xquat"][b], dtype)), ten[b]
        out[b] = R @ np.array([[t[0], t[3], t[4]], [t[3], t[1], t[5]], [t[4], t[5], t[2]]], dtype) @ R.T
    return out


def centroidal(m, o, qvel, body, mass=None, inertia=None, dtype=np.float64, axes=None, rates=None):
    """(jac_com, angmom_mat [3, nv], bias [6]) of the subtree rooted at `body` (0: the whole model)."""
    A = m.arrays
    axes = dr.dof_axes(m, o, dtype) if axes is None else axes
    rates = dof_rates(m, o, qvel, dtype, axes) if rates is None else rates
    ms, qv, xi = _f(m.body_mass if mass is None else mass, dtype), _f(qvel, dtype), _f(o["xipos"], dtype)
    Iw = world_inertia(m, o, inertia, dtype)
    sub = [k for k in range(int(body), int(A["body_subtree_end"][body])) if k > 0]
    jc, am, bias = np.zeros((3, m.nv), dtype), np.zeros((3, m.nv), dtype), np.zeros(6, dtype)
    mb = sum(ms[k] for k in sub)
    if not sub or mb < 1e-15:
        return jc, am, bias
    cb = sum(ms[k] * xi[k] for k in sub) / mb
    for k in sub:
        jp, jr = dr.jac(m, o, k, xi[k], dtype, axes)
        _, _, jdv = jac_dot(m, o, k, xi[k], qvel, dtype, axes, rates)
        r, w, a, dw = xi[k] - cb, jr @ qv, jdv[:3], jdv[3:]
        jc = jc + ms[k] * jp
        am = am + Iw[k] @ jr + ms[k] * np.cross(r, jp.T).T
        bias[:3] += ms[k] * a
        bias[3:] += Iw[k] @ dw + np.cross(w, Iw[k] @ w) + ms[k] * np.cross(r, a)
    bias[:3] /= mb
    return (jc / mb).astype(dtype), am.astype(dtype), bias


def integrate(m, qpos, qvel, h):
    """qpos advanced by h along qvel as the step integrates positions: hinge angles and free translations
    linearly, the free joint's quaternion by the exponential of its body-local rates."""
    A = m.arrays
    q, v = np.array(qpos, np.float64), np.asarray(qvel, np.float64)
    for j in range(m.njnt):
        a, d = int(A["jnt_qposadr"][j]), int(A["jnt_dofadr"][j])
        if A["jnt_type"][j] != mjcf.JNT_FREE:
            q[a] += h * v[d]
            continue
        q[a:a + 3] += h * v[d:d + 3]
        w = h * v[d + 3:d + 6]
        ang = np.linalg.norm(w)
        ex = np.array([1.0, 0.0, 0.0, 0.0]) if ang < 1e-300 else np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * w / ang])
        q[a + 3:a + 7] = mjcf.quat_mul(q[a + 3:a + 7], ex)
    return q
