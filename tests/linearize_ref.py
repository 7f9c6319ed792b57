"""Float64 reference for the step linearization (mjl_step_jacobian / mjx.transition): the tangent-space maps of
mj_integratePos and mj_differentiatePos, written from MuJoCo's definitions, and the (A, B) they make of the
oracle's raw step Jacobian (Oracle.step_jacobian: rows (qpos', qvel'), columns (qpos, qvel, ctrl)).

  input   dq [nv] acts on qpos as integrate_pos(qpos, dq): hinge coordinates and a free joint's position add, its
          quaternion becomes q (x) exp(d), d a rotation vector in the body frame; linearised dquat = 1/2 q (x) (0, d)
  output  differentiate_pos(q1, q0) [nv]: the dq that takes q0 to q1; for the free quaternion the rotation vector of
          conj(q0) (x) q1; linearised at q0 = q'0: d' = 2 vec(conj(q'0) (x) dquat')
"""
import numpy as np

from mjx_amd import mjcf


def quat_mul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                     a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
                     a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def quat_conj(q):
    return np.array([q[0], -q[1], -q[2], -q[3]])


def _joints(m):
    """(is_free, qpos address, dof address) per joint."""
    return [(int(m.jnt_type[j]) == mjcf.JNT_FREE, int(m.jnt_qposadr[j]), int(m.jnt_dofadr[j])) for j in range(m.njnt)]


def integrate_pos(m, qpos, dq):
    """mj_integratePos(m, qpos, dq, 1) on a copy."""
    q = np.array(qpos, np.float64)
    for free, qa, da in _joints(m):
        if not free:
            q[qa] += dq[da]
            continue
        q[qa:qa + 3] += dq[da:da + 3]
        d = np.asarray(dq[da + 3:da + 6], np.float64)
        ang = np.linalg.norm(d)
        e = np.array([1.0, 0, 0, 0]) if ang == 0 else np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * d / ang])
        r = quat_mul(q[qa + 3:qa + 7], e)
        q[qa + 3:qa + 7] = r / np.linalg.norm(r)
    return q


def differentiate_pos(m, q1, q0):
    """mj_differentiatePos(m, dq, 1, q0, q1): the tangent dq [nv] with integrate_pos(q0, dq) = q1."""
    dq = np.zeros(m.nv)
    for free, qa, da in _joints(m):
        if not free:
            dq[da] = q1[qa] - q0[qa]
            continue
        dq[da:da + 3] = q1[qa:qa + 3] - q0[qa:qa + 3]
        r = quat_mul(quat_conj(q0[qa + 3:qa + 7] / np.linalg.norm(q0[qa + 3:qa + 7])),
                     q1[qa + 3:qa + 7] / np.linalg.norm(q1[qa + 3:qa + 7]))
        s = np.linalg.norm(r[1:])
        ang = 2 * np.arctan2(s, r[0])
        if ang > np.pi:
            ang -= 2 * np.pi
        dq[da + 3:da + 6] = 0 if s == 0 else r[1:] / s * ang
    return dq


def tangent_maps(m, qpos, qpos_next):
    """(E [nq, nv], T [nv, nq]): d qpos = E dq at qpos, and dq' = T d qpos' at the post-step qpos_next."""
    E, T = np.zeros((m.nq, m.nv)), np.zeros((m.nv, m.nq))
    for free, qa, da in _joints(m):
        if not free:
            E[qa, da] = T[da, qa] = 1.0
            continue
        E[qa:qa + 3, da:da + 3] = T[da:da + 3, qa:qa + 3] = np.eye(3)
        q, qn = np.asarray(qpos[qa + 3:qa + 7], np.float64), np.asarray(qpos_next[qa + 3:qa + 7], np.float64)
        for k in range(3):
            E[qa + 3:qa + 7, da + 3 + k] = 0.5 * quat_mul(q, np.concatenate([[0.0], np.eye(3)[k]]))
        for j in range(4):
            T[da + 3:da + 6, qa + 3 + j] = 2.0 * quat_mul(quat_conj(qn), np.eye(4)[j])[1:]
    return E, T


def tangent_AB(m, J, qpos, qpos_next):
    """The oracle's raw Jacobian J [nq+nv, nq+nv+nu] -> (A [2nv, 2nv], B [2nv, nu]) in the tangent layout."""
    nq, nv = m.nq, m.nv
    E, T = tangent_maps(m, qpos, qpos_next)
    Tin = np.block([[E, np.zeros((nq, nv))], [np.zeros((nv, nv)), np.eye(nv)]])
    Tout = np.block([[T, np.zeros((nv, nv))], [np.zeros((nv, nq)), np.eye(nv)]])
    return Tout @ J[:, :nq + nv] @ Tin, Tout @ J[:, nq + nv:]


def raw_AB(m, J):
    return J[:, :m.nq + m.nv], J[:, m.nq + m.nv:]


def row_errors(got_A, got_B, ref_A, ref_B, nin):
    """tests/test_adjoint.py's rule with u = e_i for every row i of [A | B]: per input group (position block of
    width nin, qvel, ctrl) max|g - ref| / (max|ref| + 1e-3 max|J|), J the whole reference matrix [A | B]. Returns
    [rows, 3]."""
    scale = 1e-3 * max(np.abs(ref_A).max(), np.abs(ref_B).max())
    err = np.zeros((ref_A.shape[0], 3))
    for i in range(ref_A.shape[0]):
        for k, (g, r) in enumerate(((got_A[i, :nin], ref_A[i, :nin]), (got_A[i, nin:], ref_A[i, nin:]),
                                    (got_B[i], ref_B[i]))):
            err[i, k] = np.abs(g - r).max() / (np.abs(r).max() + scale)
    return err
