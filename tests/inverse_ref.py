"""Numpy reference of mjl_inverse (include/mjx355.h), in float64 or, with dtype=np.float32, in the kernel's
precision (the tolerance yardstick of tests/test_inverse_gpu.py).

Inputs: the model, one oracle forward output o = state_arrays(m, orc.forward(s)) and the raw OrcState s, of which
efc_D and efc_aref are read. M, qfrc_bias and qfrc_passive are the oracle's. The constraint Jacobian is rebuilt
here row by row, in the oracle's row order (joint limits, tendon limits, then the contacts in contact order, a
pyramidal contact's rows as n + mu t1, n - mu t1, n + mu t2, n - mu t2): limit rows from the joint and tendon
tables, contact rows from con_geom / con_pos / con_frame and the pair's mu through dyn_ref.jac. The kinds it finds
must be the oracle's efc_type sequence. Then

    a_c  = a, or with `discrete` a + timestep M^-1 (k o a) under the integrator's condition
    jar  = J a_c - aref,   efc_force = -D jar where jar < 0 else 0,   qfrc_constraint = J' efc_force
    qfrc_inverse = M a_c + qfrc_bias - qfrc_passive - qfrc_constraint"""
import numpy as np

from mjx_amd import mjcf

import dyn_ref as dr


def _f(x, dtype):
    return np.asarray(x, np.float64).astype(dtype)


def constraint_jacobian(m, o, dtype=np.float64):
    """(J [nefc, nv], kinds [nefc]) rebuilt from the model's tables and the oracle's contacts."""
    A, nv = m.arrays, m.nv
    qpos = _f(o["qpos"], dtype)
    rows, kinds = [], []
    for j in range(m.njnt):
        if not A["jnt_limited"][j] or A["jnt_type"][j] != mjcf.JNT_HINGE:
            continue
        q = qpos[int(A["jnt_qposadr"][j])]
        lo, hi = _f(A["jnt_range"][j], dtype)
        dmin, dmax = q - lo, hi - q
        if not (min(dmin, dmax) - dtype(A["jnt_margin"][j]) < 0):
            continue
        r = np.zeros(nv, dtype)
        r[int(A["jnt_dofadr"][j])] = 1 if dmin < dmax else -1
        rows.append(r)
        kinds.append(0)
    for t in range(m.ntendon):
        if not A["tendon_limited"][t]:
            continue
        length, tj = dtype(0), np.zeros(nv, dtype)
        for w in range(int(A["tendon_num"][t])):
            j, c = int(A["tendon_jnt"][t][w]), dtype(A["tendon_coef"][t][w])
            length = length + c * qpos[int(A["jnt_qposadr"][j])]
            tj[int(A["jnt_dofadr"][j])] += c
        lo, hi = _f(A["tendon_range"][t], dtype)
        dmin, dmax = length - lo, hi - length
        if not (min(dmin, dmax) - dtype(A["tendon_margin"][t]) < 0):
            continue
        rows.append(tj if dmin < dmax else -tj)
        kinds.append(1)
    pair = {(int(a), int(b)): p for p, (a, b) in enumerate(zip(A["pair_geom1"], A["pair_geom2"]))}
    friction = np.reshape(np.asarray(A["pair_friction"], np.float64), (len(pair), -1))
    axes = dr.dof_axes(m, o, dtype)
    for ci in range(int(o["ncon"])):
        g1, g2 = (int(g) for g in o["con_geom"][ci])
        p = pair[(g1, g2)]
        x = _f(o["con_pos"][ci], dtype)
        fr = _f(o["con_frame"][ci], dtype).reshape(3, 3)
        jd = dr.jac(m, o, int(A["geom_bodyid"][g2]), x, dtype, axes)[0] - dr.jac(m, o, int(A["geom_bodyid"][g1]), x, dtype, axes)[0]
        jn = fr[0] @ jd
        if int(A["pair_condim"][p]) == 1:
            rows.append(jn)
            kinds.append(2)
            continue
        mu = dtype(friction[p, 0])
        for t in (1, 2):
            jt = fr[t] @ jd
            rows += [jn + mu * jt, jn - mu * jt]
            kinds += [3, 3]
    J = np.array(rows, dtype).reshape(len(rows), nv)
    return J, np.array(kinds, np.int32)


def integrator_diagonal(m, dtype=np.float64):
    """k of the header, or None when the integrator's condition does not hold (a_c = a)."""
    A = m.arrays
    k = _f(A["dof_damping"], dtype).copy()
    implicit = m.integrator == mjcf.INT_IMPLICITFAST
    on = (implicit or bool(m.eulerdamp)) and bool(np.any(np.asarray(A["dof_damping"]) != 0))
    if implicit and "actuator_biasprm" in A and np.any(np.asarray(A["actuator_biasprm"])[:, 2] != 0):
        dof = np.asarray(A["jnt_dofadr"])[np.asarray(A["actuator_trnid"])]
        gear, b2 = _f(A["actuator_gear"], dtype), _f(np.asarray(A["actuator_biasprm"])[:, 2], dtype)
        for u in range(len(dof)):
            k[dof[u]] -= gear[u] * gear[u] * b2[u]
        on = True
    return k if on else None


def efc_force(J, D, aref, acc):
    """(efc_force, jar) of the one-sided rows at the acceleration acc."""
    jar = J @ acc - aref if len(J) else np.zeros(0, acc.dtype)
    return np.where(jar < 0, -D * jar, 0).astype(acc.dtype), jar


def inverse(m, o, raw, qacc, discrete=False, dtype=np.float64, J=None):
    """(qfrc_inverse, qfrc_constraint, efc_force, jar) at the acceleration qacc [nv]."""
    nefc = int(o["nefc"])
    if J is None:
        J, kinds = constraint_jacobian(m, o, dtype)
        assert list(kinds) == [int(t) for t in o["efc_type"]], "rebuilt rows differ from the oracle's efc_type"
    M = _f(o["M"], dtype)
    D, aref = _f(np.array(raw.efc_D)[:nefc], dtype), _f(np.array(raw.efc_aref)[:nefc], dtype)
    a = _f(qacc, dtype)
    k = integrator_diagonal(m, dtype) if discrete else None
    if k is not None:
        a = a + dtype(m.timestep) * dr.solve(M, k * a, dtype)
    force, jar = efc_force(J, D, aref, a)
    fc = J.T @ force if nefc else np.zeros(m.nv, dtype)
    qfrc = M @ a + _f(o["qfrc_bias"], dtype) - _f(o["qfrc_passive"], dtype) - fc
    return qfrc.astype(dtype), fc.astype(dtype), force, jar
