"""Reference for the sensor readout (mjl_sensors / mjx.sensors): a numpy restatement of the sensor table of
include/mjx355.h, written from the definitions (MuJoCo's mj_sensorPos / mj_sensorVel / mj_sensorAcc) as a
classical rigid-body recursion over rotation matrices: frames root to leaf, each hinge a Rodrigues rotation
about its world axis through its world anchor; angular velocity and acceleration of each body and the linear
velocity and acceleration of its origin by the transport theorem. Not a transcription of the kernel (which
composes quaternions and carries a moving reference point).

Inputs are the oracle's forward outputs of the state (oracle.state_arrays: qpos, qvel, qacc, qfrc_actuator,
efc_force, efc_type, sensordata) plus ctrl. `dtype=np.float32` evaluates the same formulas in float32: the
yardstick of the GPU test's tolerances (tests/test_sensors_gpu.py). tests/test_sensors.py validates this
module on the CPU against finite differences and the oracle's kinematics."""
import numpy as np

from mjx_amd import mjcf

T = mjcf.SENSOR_TYPES


def _skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], v.dtype)


def _qmat(q):
    return np.asarray(mjcf.quat2mat(q), q.dtype)


def _rodrigues(axis, ang, dt):
    K = _skew(axis)
    return np.eye(3, dtype=dt) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)


def kinematics(m, qpos, qvel=None, qacc=None, dtype=np.float64):
    """Per body: origin x [nb,3], rotation R [nb,3,3], angular velocity w and acceleration dw, linear velocity v
    and classical acceleration a of the origin (world frame)."""
    dt = dtype
    A = m.arrays
    nb = m.nbody
    qpos = np.asarray(qpos, dt)
    qvel = np.zeros(m.nv, dt) if qvel is None else np.asarray(qvel, dt)
    qacc = np.zeros(m.nv, dt) if qacc is None else np.asarray(qacc, dt)
    x, R = np.zeros((nb, 3), dt), np.tile(np.eye(3, dtype=dt), (nb, 1, 1))
    w, dw, v, a = (np.zeros((nb, 3), dt) for _ in range(4))
    for b in range(1, nb):
        p = int(A["body_parentid"][b])
        j0, nj = int(A["body_jntadr"][b]), int(A["body_jntnum"][b])
        if nj == 1 and A["jnt_type"][j0] == mjcf.JNT_FREE:
            qa, da = int(A["jnt_qposadr"][j0]), int(A["jnt_dofadr"][j0])
            quat = qpos[qa + 3:qa + 7] / np.linalg.norm(qpos[qa + 3:qa + 7])
            x[b], R[b] = qpos[qa:qa + 3], _qmat(quat)
            v[b], a[b] = qvel[da:da + 3], qacc[da:da + 3]
            w[b], dw[b] = R[b] @ qvel[da + 3:da + 6], R[b] @ qacc[da + 3:da + 6]
            continue
        # the body frame before its joints act: rigidly attached to the parent
        Rb = R[p] @ _qmat(np.asarray(A["body_quat"][b], dt))
        xb = x[p] + R[p] @ np.asarray(A["body_pos"][b], dt)
        off = xb - x[p]
        wb, dwb = w[p].copy(), dw[p].copy()
        vb = v[p] + np.cross(wb, off)
        ab = a[p] + np.cross(dwb, off) + np.cross(wb, np.cross(wb, off))
        for j in range(j0, j0 + nj):
            ang = qpos[int(A["jnt_qposadr"][j])] - dt(A["qpos0"][int(A["jnt_qposadr"][j])])
            d = int(A["jnt_dofadr"][j])
            axis = Rb @ np.asarray(A["jnt_axis"][j], dt)
            c = xb + Rb @ np.asarray(A["jnt_pos"][j], dt)  # the anchor: fixed on both sides of the joint
            vc = vb + np.cross(wb, c - xb)
            ac = ab + np.cross(dwb, c - xb) + np.cross(wb, np.cross(wb, c - xb))
            dwb = dwb + axis * qacc[d] + np.cross(wb, axis) * qvel[d]
            wb = wb + axis * qvel[d]
            Rot = _rodrigues(axis, ang, dt)
            r = Rot @ (xb - c)  # the origin's offset from the anchor, after the rotation
            Rb, xb = Rot @ Rb, c + r
            vb = vc + np.cross(wb, r)
            ab = ac + np.cross(dwb, r) + np.cross(wb, np.cross(wb, r))
        x[b], R[b], w[b], dw[b], v[b], a[b] = xb, Rb, wb, dwb, vb, ab
    return {"x": x, "R": R, "w": w, "dw": dw, "v": v, "a": a}


def frame(m, k, objtype, objid, dtype=np.float64):
    """(p, R, w, v, a) of an xbody or site frame from kinematics() output k."""
    A = m.arrays
    if objtype == mjcf.OBJ_XBODY:
        b, off, Rl = objid, np.zeros(3, dtype), np.eye(3, dtype=dtype)
    else:
        b = int(A["site_bodyid"][objid])
        off = k["R"][b] @ np.asarray(A["site_pos"][objid], dtype)
        Rl = _qmat(np.asarray(A["site_quat"][objid], dtype))
    w, dw = k["w"][b], k["dw"][b]
    return (k["x"][b] + off, k["R"][b] @ Rl, w, k["v"][b] + np.cross(w, off),
            k["a"][b] + np.cross(dw, off) + np.cross(w, np.cross(w, off)))


def mat2quat(R):
    """Unit quaternion [w, x, y, z] of a rotation matrix, w >= 0 (largest-component branch)."""
    R = np.asarray(R, np.float64)
    K = np.array([[R[0, 0] + R[1, 1] + R[2, 2], R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]],
                  [0, R[0, 0] - R[1, 1] - R[2, 2], R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]],
                  [0, 0, R[1, 1] - R[0, 0] - R[2, 2], R[1, 2] + R[2, 1]],
                  [0, 0, 0, R[2, 2] - R[0, 0] - R[1, 1]]])
    K = K + np.triu(K, 1).T
    wv, V = np.linalg.eigh(K)
    q = V[:, -1]
    return q if q[0] >= 0 else -q


def active_limit_joints(m, qpos):
    """Joints whose limit row is active, in row order (joint order): dist - margin < 0."""
    A = m.arrays
    out = []
    for j in range(m.njnt):
        if A["jnt_type"][j] != mjcf.JNT_HINGE or not A["jnt_limited"][j]:
            continue
        q = qpos[int(A["jnt_qposadr"][j])]
        if min(q - A["jnt_range"][j][0], A["jnt_range"][j][1] - q) - A["jnt_margin"][j] < 0:
            out.append(j)
    return out


def actuator_force(m, u, qpos, qvel, ctrl, gear=None, dtype=np.float64):
    """(force after the force-range clamp, whether the clamp acted)."""
    A, dt = m.arrays, dtype
    j = int(A["actuator_trnid"][u])
    c = dt(ctrl[u])
    if A["actuator_ctrllimited"][u]:
        c = min(max(c, dt(A["actuator_ctrlrange"][u][0])), dt(A["actuator_ctrlrange"][u][1]))
    if "actuator_kind" not in A or A["actuator_kind"][u] == mjcf.ACT_MOTOR:
        return c, False
    g = dt(A["actuator_gear"][u] if gear is None else gear[u])
    b = np.asarray(A["actuator_biasprm"][u], dt)
    f = dt(A["actuator_gain"][u]) * c + b[0] + b[1] * g * dt(qpos[int(A["jnt_qposadr"][j])]) \
        + b[2] * g * dt(qvel[int(A["jnt_dofadr"][j])])
    if A["actuator_forcelimited"][u]:
        lo, hi = dt(A["actuator_forcerange"][u][0]), dt(A["actuator_forcerange"][u][1])
        return min(max(f, lo), hi), bool(f < lo or f > hi)
    return f, False


def sensordata(m, o, ctrl, gear=None, dtype=np.float64):
    """Data.sensordata [nrsensordata] from the oracle's forward outputs `o` of the state."""
    A, dt = m.arrays, dtype
    qpos, qvel = np.asarray(o["qpos"], dt), np.asarray(o["qvel"], dt)
    k = kinematics(m, qpos, qvel, o["qacc"], dt)
    g = np.asarray(m.gravity, dt)
    lim = active_limit_joints(m, np.asarray(o["qpos"], np.float64))
    rows = [r for r in range(len(o["efc_type"])) if o["efc_type"][r] == 0]
    assert len(rows) == len(lim), "the oracle's joint-limit rows are the active limits"
    out = np.zeros(m.nrsensordata, dt)
    for s in range(m.nrsensor):
        t, ot, oid = (int(A["rsensor_" + f][s]) for f in ("type", "objtype", "objid"))
        sl = slice(int(A["rsensor_adr"][s]), int(A["rsensor_adr"][s]) + int(A["rsensor_dim"][s]))
        if ot in (mjcf.OBJ_XBODY, mjcf.OBJ_SITE):
            p, R, w, v, a = frame(m, k, ot, oid, dt)
            val = {T["framepos"]: lambda: p, T["framequat"]: lambda: mat2quat(R), T["framexaxis"]: lambda: R[:, 0],
                   T["frameyaxis"]: lambda: R[:, 1], T["framezaxis"]: lambda: R[:, 2], T["gyro"]: lambda: R.T @ w,
                   T["velocimeter"]: lambda: R.T @ v, T["framelinvel"]: lambda: v, T["frameangvel"]: lambda: w,
                   T["accelerometer"]: lambda: R.T @ (a - g)}[t]()
        elif ot == mjcf.OBJ_JOINT:
            qa, d = int(A["jnt_qposadr"][oid]), int(A["jnt_dofadr"][oid])
            val = {T["jointpos"]: lambda: qpos[qa], T["jointvel"]: lambda: qvel[d],
                   T["jointactuatorfrc"]: lambda: dt(o["qfrc_actuator"][d]),
                   T["jointlimitfrc"]: lambda: dt(o["efc_force"][rows[lim.index(oid)]]) if oid in lim else dt(0)}[t]()
        elif ot == mjcf.OBJ_ACTUATOR:
            val = actuator_force(m, oid, qpos, qvel, ctrl, gear, dt)[0]
        else:
            val = dt(o["sensordata"][int(A["sensor_adr"][oid])])
        out[sl] = val
    return out


def scales(m, ref_rows):
    """Per sensor type: the value's scale over the test states, max |value| (at least 1)."""
    A = m.arrays
    out = {}
    for s in range(m.nrsensor):
        sl = slice(int(A["rsensor_adr"][s]), int(A["rsensor_adr"][s]) + int(A["rsensor_dim"][s]))
        t = int(A["rsensor_type"][s])
        out[t] = max(out.get(t, 1.0), float(np.max(np.abs(ref_rows[:, sl]))))
    return out
