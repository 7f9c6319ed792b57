"""Numpy reference of mjl_jac / mjl_mass_matrix (include/mjx355.h), in float64 or, with dtype=np.float32, in the
kernel's precision (the tolerance yardstick of tests/test_dyn_gpu.py). Inputs: the model and one oracle forward
output o = state_arrays(m, orc.forward(...)), of which xpos, xquat, xipos and qpos are read: the Jacobian is built
from the body frames and the model's joint records by the table of the header, not from the oracle's cdof, and M
as the kinetic energy's matrix sum_b m_b Jv'Jv + Jw' I_b Jw + diag(armature) with the Jacobians at xipos (the
construction of tests/test_risk_kats.py), not by composite rigid bodies. The model's own qpos0 is the zero of each
hinge angle."""
import numpy as np

from mjx_amd import mjcf


def _q2m(q):
    w, x, y, z = q
    one, two = q.dtype.type(1), q.dtype.type(2)
    return np.array([[one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)],
                     [two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)],
                     [two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]], q.dtype)


def _qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]],
                    a.dtype)


def dof_axes(m, o, dtype=np.float64):
    """Per dof: (kind, world axis, world anchor); kind 0 a rotation about the axis through the anchor, 1 a
    translation along it. A body's hinges are peeled off its final frame from the last one backwards."""
    A = m.arrays
    f = lambda x: np.asarray(x, np.float64).astype(dtype)
    xpos, xquat, qpos = f(o["xpos"]), f(o["xquat"]), f(o["qpos"])
    out = [None] * m.nv
    for b in range(1, m.nbody):
        j0, jn = int(A["body_jntadr"][b]), int(A["body_jntnum"][b])
        pos, quat = xpos[b].copy(), xquat[b].copy()
        for j in reversed(range(j0, j0 + jn)):
            d = int(A["jnt_dofadr"][j])
            R = _q2m(quat)
            if A["jnt_type"][j] == mjcf.JNT_FREE:
                for i in range(3):
                    e = np.zeros(3, dtype)
                    e[i] = 1
                    out[d + i] = (1, e, pos.copy())
                    out[d + 3 + i] = (0, R[:, i].copy(), pos.copy())
                continue
            assert A["jnt_type"][j] == mjcf.JNT_HINGE
            axis, jpos = f(A["jnt_axis"][j]), f(A["jnt_pos"][j])
            anchor = pos + R @ jpos
            out[d] = (0, R @ axis, anchor)
            half = dtype(0.5) * (qpos[int(A["jnt_qposadr"][j])] - f(m.qpos0)[int(A["jnt_qposadr"][j])])
            quat = _qmul(quat, np.concatenate([[np.cos(half)], -np.sin(half) * axis]).astype(dtype))
            pos = anchor - _q2m(quat) @ jpos
    return out


def body_dofs(m, body):
    """The dofs that move `body`: its own and its ancestors'."""
    A, dofs = m.arrays, []
    b = int(body)
    while b > 0:
        dofs += range(int(A["body_dofadr"][b]), int(A["body_dofadr"][b]) + int(A["body_dofnum"][b]))
        b = int(A["body_parentid"][b])
    return sorted(dofs)


def jac(m, o, body, x, dtype=np.float64, axes=None):
    """(jacp, jacr) [3, nv] of the world point x carried by `body`."""
    axes = dof_axes(m, o, dtype) if axes is None else axes
    x = np.asarray(x, np.float64).astype(dtype)
    jp, jr = np.zeros((3, m.nv), dtype), np.zeros((3, m.nv), dtype)
    for d in body_dofs(m, body):
        kind, a, p = axes[d]
        if kind == 1:
            jp[:, d] = a
        else:
            jr[:, d] = a
            jp[:, d] = np.cross(a, x - p)
    return jp, jr


def local_point(o, body, offset=None, dtype=np.float64):
    """xpos_b + R_b offset."""
    p = np.asarray(o["xpos"][body], np.float64).astype(dtype)
    if offset is None:
        return p
    return p + _q2m(np.asarray(o["xquat"][body], np.float64).astype(dtype)) @ np.asarray(offset, np.float64).astype(dtype)


def mass_matrix(m, o, mass=None, inertia=None, armature=None, dtype=np.float64):
    A = m.arrays
    f = lambda x: np.asarray(x, np.float64).astype(dtype)
    mass = f(m.body_mass if mass is None else mass)
    inertia = f(A["body_inertia"] if inertia is None else inertia).reshape(m.nbody, 6)
    armature = f(A["dof_armature"] if armature is None else armature)
    axes = dof_axes(m, o, dtype)
    M = np.diag(armature).astype(dtype)
    for b in range(1, m.nbody):
        jv, jw = jac(m, o, b, o["xipos"][b], dtype, axes)
        R = _q2m(f(o["xquat"][b]))
        t = inertia[b]
        Iw = R @ np.array([[t[0], t[3], t[4]], [t[3], t[1], t[5]], [t[4], t[5], t[2]]], dtype) @ R.T
        M = M + mass[b] * (jv.T @ jv) + jw.T @ (Iw @ jw)
    return M


def solve(M, v, dtype=np.float64):
    """M^-1 v ([nv] or [nvec, nv]) through numpy.linalg.cholesky and two substitutions, all in dtype."""
    L = np.linalg.cholesky(np.asarray(M, np.float64).astype(dtype)).astype(dtype)
    v = np.asarray(v, np.float64).astype(dtype)
    x = np.atleast_2d(v).copy()
    n = L.shape[0]
    for i in range(n):
        x[:, i] = (x[:, i] - x[:, :i] @ L[i, :i]) / L[i, i]
    for i in reversed(range(n)):
        x[:, i] = (x[:, i] - x[:, i + 1:] @ L[i + 1:, i]) / L[i, i]
    return x.reshape(v.shape)
