"""Numpy reference of mjl_ik (include/mjx355.h), in float64 or, with dtype=np.float32, in the kernel's precision
(the tolerance yardstick of tests/test_ik_gpu.py). It restates the header's iteration for one env: its own forward
kinematics of the iterate (the tree pass of mjl_jac: the free quaternion normalised for the pass, every hinge about
its world axis), dyn_ref's Jacobian columns from those frames, the weighted normal equations accumulated task by task
and row by row, a Cholesky solve, the step bound, mj_integratePos and the clamp to jnt_range."""
import numpy as np

from mjx_amd import mjcf

import dyn_ref as dr

MINVAL = 1e-15


def _qnorm(q):
    n = np.sqrt((q * q).sum(dtype=q.dtype))
    if n < MINVAL:
        return np.array([1, 0, 0, 0], q.dtype)
    return q * (q.dtype.type(1) / n)


def _conj(q):
    return np.array([q[0], -q[1], -q[2], -q[3]], q.dtype)


def kinematics(m, qpos, dtype=np.float64):
    """{"xpos", "xquat", "qpos"} of every body from qpos, in dtype: what dyn_ref.dof_axes / jac read."""
    A = m.arrays
    f = lambda x: np.asarray(x, np.float64).astype(dtype)
    q = f(qpos)
    q0 = f(m.qpos0)
    xpos, xquat = np.zeros((m.nbody, 3), dtype), np.zeros((m.nbody, 4), dtype)
    xquat[0, 0] = 1
    for b in range(1, m.nbody):
        par = int(A["body_parentid"][b])
        j0, jn = int(A["body_jntadr"][b]), int(A["body_jntnum"][b])
        if jn == 1 and A["jnt_type"][j0] == mjcf.JNT_FREE:
            a = int(A["jnt_qposadr"][j0])
            xpos[b], xquat[b] = q[a:a + 3], _qnorm(q[a + 3:a + 7])
            continue
        lp = xpos[par] + dr._q2m(xquat[par]) @ f(A["body_pos"][b])
        lq = dr._qmul(xquat[par], f(A["body_quat"][b]))
        for j in range(j0, j0 + jn):
            assert A["jnt_type"][j] == mjcf.JNT_HINGE
            jpos, axis = f(A["jnt_pos"][j]), f(A["jnt_axis"][j])
            anc = dr._q2m(lq) @ jpos + lp
            a = int(A["jnt_qposadr"][j])
            half = dtype(0.5) * (q[a] - q0[a])
            lq = dr._qmul(lq, np.concatenate([[np.cos(half)], np.sin(half) * axis]).astype(dtype))
            lp = anc - dr._q2m(lq) @ jpos
        xpos[b], xquat[b] = lp, _qnorm(lq)
    return {"xpos": xpos, "xquat": xquat, "qpos": q}


def rotvec(q):
    """The rotation vector of the unit quaternion q, its scalar part made non-negative: mju_quat2Vel at dt = 1."""
    t = q.dtype.type
    sg = t(-1) if q[0] < 0 else t(1)
    v = sg * q[1:]
    n = np.sqrt((v * v).sum(dtype=q.dtype))
    s = t(0) if n < MINVAL else t(2) * np.arctan2(n, sg * q[0]) / n
    return (v * s).astype(q.dtype)


def residuals(m, o, body, offset, target_pos, target_quat, dtype=np.float64):
    """(world points [ntask, 3], err [ntask, 6]) at the frames o; rows without a target array are zeros."""
    f = lambda x: np.asarray(x, np.float64).astype(dtype)
    n = len(body)
    xs, e = np.zeros((n, 3), dtype), np.zeros((n, 6), dtype)
    for t, b in enumerate(body):
        xs[t] = dr.local_point(o, b, None if offset is None else offset[t], dtype)
        if target_pos is not None:
            e[t, :3] = f(target_pos[t]) - xs[t]
        if target_quat is not None:
            e[t, 3:] = rotvec(dr._qmul(_qnorm(f(target_quat[t])), _conj(o["xquat"][b])))
    return xs, e


def dof_address(m, d):
    """(qpos address, index inside a free joint or -1, joint id) of dof d; a free rotation dof: the quaternion's."""
    A = m.arrays
    j = int(A["dof_jntid"][d])
    a = int(A["jnt_qposadr"][j])
    if A["jnt_type"][j] != mjcf.JNT_FREE:
        return a, -1, j
    k = d - int(A["jnt_dofadr"][j])
    return (a + k if k < 3 else a + 3), k, j


def differentiate_pos(m, qref, q, dtype=np.float64):
    """mj_differentiatePos(qref, q): the tangent [nv] from q toward qref."""
    f = lambda x: np.asarray(x, np.float64).astype(dtype)
    qref, q = f(qref), f(q)
    out = np.zeros(m.nv, dtype)
    for d in range(m.nv):
        a, k, _ = dof_address(m, d)
        if k < 3:
            out[d] = qref[a] - q[a]
        else:
            out[d] = rotvec(dr._qmul(_conj(_qnorm(q[a:a + 4])), _qnorm(qref[a:a + 4])))[k - 3]
    return out


def integrate_pos(m, q, dq, active, limits, dtype=np.float64):
    """mj_integratePos(q, dq, 1) over the dofs `active` [nv] may move, limited hinges clamped when `limits`."""
    A = m.arrays
    q = q.copy()
    for d in range(m.nv):
        a, k, j = dof_address(m, d)
        if k < 3:
            if active[d]:
                q[a] = q[a] + dq[d]
                if limits and k < 0 and A["jnt_limited"][j]:
                    lo, hi = np.asarray(A["jnt_range"][j], np.float64).astype(dtype)
                    q[a] = min(max(q[a], lo), hi)
        elif k == 3:
            w = np.where(active[d:d + 3], dq[d:d + 3], dtype(0)).astype(dtype)
            n = np.sqrt((w * w).sum(dtype=dtype))
            if not n > 0:
                continue
            w = w * (dtype(1) / (n + (dtype(1e-6) if n == 0 else dtype(0))))
            half = dtype(0.5) * n
            q[a:a + 4] = _qnorm(dr._qmul(q[a:a + 4], np.concatenate([[np.cos(half)], np.sin(half) * w]).astype(dtype)))
    return q


def task_rows(m, o, body, xs, dtype=np.float64):
    """[ntask, 6, nv]: (jacp ; jacr) of every task point."""
    axes = dr.dof_axes(m, o, dtype)
    return np.array([np.concatenate(dr.jac(m, o, b, xs[t], dtype, axes)) for t, b in enumerate(body)])


def solve(m, body, offset=None, target_pos=None, target_quat=None, weight=None, qpos_start=None, qpos_ref=None,
          dofmask=0xFFFFFFFF, iterations=20, damping=1e-3, posture=0.0, max_step=0.0, tol=0.0, limits=True,
          dtype=np.float64):
    """One env's solve: (qpos [nq], err [ntask, 6], niter). target_pos [ntask, 3], target_quat [ntask, 4]."""
    assert target_pos is not None or target_quat is not None
    f = lambda x: np.asarray(x, np.float64).astype(dtype)
    t_ = dtype
    n, nv = len(body), m.nv
    q = f(m.qpos0 if qpos_start is None else qpos_start)
    qref = f(m.qpos0 if qpos_ref is None else qpos_ref)
    w = np.ones((n, 2), dtype) if weight is None else f(weight)
    w = np.where(w > 0, w, 0).astype(dtype)
    if target_pos is None:
        w[:, 0] = 0
    if target_quat is None:
        w[:, 1] = 0
    active = np.array([bool((int(dofmask) >> d) & 1) for d in range(nv)])
    damping, posture, max_step, tol = t_(damping), t_(posture), t_(max_step), t_(tol)
    k = 0
    while True:
        o = kinematics(m, q, dtype)
        xs, e = residuals(m, o, body, offset, target_pos, target_quat, dtype)
        res = max(max(w[t, 0] * np.sqrt((e[t, :3] ** 2).sum(dtype=dtype)), w[t, 1] * np.sqrt((e[t, 3:] ** 2).sum(dtype=dtype)))
                  for t in range(n))
        if k >= iterations or (tol > 0 and res < tol):
            return q, e, k
        J = task_rows(m, o, body, xs, dtype)
        J[:, :, ~active] = 0
        H = np.diag(np.where(active, damping + posture, t_(1))).astype(dtype)
        g = np.zeros(nv, dtype)
        if posture > 0:
            g = np.where(active, posture * differentiate_pos(m, qref, q, dtype), t_(0)).astype(dtype)
        for t in range(n):
            for r in range(6):
                wr = w[t, 0] if r < 3 else w[t, 1]
                if not wr > 0:
                    continue
                c = (wr * J[t, r]).astype(dtype)
                H = (H + np.outer(c, c)).astype(dtype)
                g = (g + c * (wr * e[t, r])).astype(dtype)
        dq = dr.solve(H, g, dtype)
        s = np.abs(dq).max()
        if max_step > 0 and s > max_step:
            dq = (dq * (max_step / s)).astype(dtype)
        q = integrate_pos(m, q, dq, active, limits, dtype)
        k += 1


def frame_tasks(m, frames):
    """(body ids, body-frame offsets [ntask, 3], body-frame rotations [ntask, 4] as quaternions) of frames given as
    ("xbody" | "site", id): a site is its body at site_pos, turned by site_quat."""
    body, off, quat = [], [], []
    for kind, i in frames:
        if kind == "site":
            body.append(int(m.arrays["site_bodyid"][i]))
            off.append(np.asarray(m.arrays["site_pos"][i], np.float64))
            quat.append(np.asarray(m.arrays["site_quat"][i], np.float64))
        else:
            body.append(int(i))
            off.append(np.zeros(3))
            quat.append(np.array([1.0, 0, 0, 0]))
    return body, np.array(off), np.array(quat)


def frame_pose(m, qpos, body, offset, dtype=np.float64):
    """(world points [ntask, 3], body quaternions [ntask, 4]) of the task frames at qpos."""
    o = kinematics(m, qpos, dtype)
    return (np.array([dr.local_point(o, b, offset[t], dtype) for t, b in enumerate(body)]),
            np.array([o["xquat"][b] for b in body]))
