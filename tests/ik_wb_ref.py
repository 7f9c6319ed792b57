"""Numpy reference of mjl_ik_wb (include/mjx355.h), in float64 or, with dtype=np.float32, in the kernel's precision
(the tolerance yardstick of tests/test_ik_wb_gpu.py). It is ik_ref.solve's iteration with the header's added steps,
restated on the references the readouts already have: ik_ref.kinematics / residuals / task_rows / integrate_pos /
differentiate_pos for the frame tasks and the update, taskspace_ref.centroidal's jac_com for the CoM rows and
distance_ref.geom_distance for the pairs' dist, witness points and normal (the gradient row is then
normal' (jacp(to) - jacp(from)) from dyn_ref.jac in dtype, as distance_ref builds it in float64).

With dtype=np.float32 the frames, the geoms' scene and every array handed to those references are float32, so their
arithmetic runs in float32 (numpy keeps the arrays' type).

solve() also returns, per evaluated iterate and pair, the margin |dist - clear_min|: the one-sided rows make the
result discontinuous where dist crosses clear_min, so a comparison is meaningful only while the margin is not small."""
import numpy as np

from mjx_amd import mjcf

import distance_ref as dref
import dyn_ref as dr
import ik_ref as ik
import taskspace_ref as ts


def _f(x, dtype):
    return np.asarray(x, np.float64).astype(dtype)


def frames(m, q, dtype=np.float64):
    """ik_ref.kinematics plus xipos: what taskspace_ref.centroidal reads."""
    o = ik.kinematics(m, q, dtype)
    ipos = _f(m.arrays["body_ipos"], dtype)
    o["xipos"] = np.array([o["xpos"][b] + dr._q2m(o["xquat"][b]) @ ipos[b] for b in range(m.nbody)], dtype)
    return o


def subtree_com(m, o, body, mass=None, dtype=np.float64):
    """The centre of mass of the subtree rooted at `body` (0: the whole model): the sums in body order."""
    ms = _f(m.body_mass if mass is None else mass, dtype)
    sub = [k for k in range(int(body), int(m.arrays["body_subtree_end"][body])) if k > 0]
    tot, s = dtype(0), np.zeros(3, dtype)
    for k in sub:
        tot = dtype(tot + ms[k])
        s = (s + ms[k] * o["xipos"][k]).astype(dtype)
    return (s * (dtype(1) / tot)).astype(dtype)


def com_rows(m, o, body, mass=None, dtype=np.float64):
    """[3, nv]: mjl_centroidal's jac_com of the subtree."""
    return ts.centroidal(m, o, np.zeros(m.nv), body, mass=mass, dtype=dtype)[0]


def scene(m, o, dtype=np.float64):
    """distance_ref's scene (render_ref.scene's fields) from the frames o, in dtype."""
    A = m.arrays
    pos, z = [], []
    for g in range(m.ngeom):
        b = int(A["geom_bodyid"][g])
        R = dr._q2m(o["xquat"][b])
        pos.append(o["xpos"][b] + R @ _f(A["geom_pos"][g], dtype))
        z.append(R @ _f(mjcf.quat2mat(A["geom_quat"][g]).reshape(3, 3)[:, 2], dtype))
    return {"pos": np.array(pos, dtype).reshape(-1, 3), "z": np.array(z, dtype).reshape(-1, 3),
            "r": _f(A["geom_size"][:, 0], dtype), "h": _f(A["geom_size"][:, 1], dtype), "type": A["geom_type"],
            "kin": {"xpos": o["xpos"], "xquat": o["xquat"]}, "qpos": o["qpos"]}


def pair_rows(m, o, geom1, geom2, dtype=np.float64):
    """(dist [P], jac [P, nv]) of the pairs at the frames o, uncapped: mjl_geom_distance's dist and jac."""
    P = len(geom1)
    if P == 0:
        return np.zeros(0, dtype), np.zeros((0, m.nv), dtype)
    dist, fromto, normal, _, _ = dref.geom_distance(m, scene(m, o, dtype), geom1, geom2, np.inf, with_jac=False)
    axes = dr.dof_axes(m, o, dtype)
    B = m.arrays["geom_bodyid"]
    jac = np.zeros((P, m.nv), dtype)
    for k in range(P):
        n = _f(normal[k], dtype)
        jt = dr.jac(m, o, int(B[geom2[k]]), _f(fromto[k, 3:], dtype), dtype, axes)[0]
        jf = dr.jac(m, o, int(B[geom1[k]]), _f(fromto[k, :3], dtype), dtype, axes)[0]
        jac[k] = n @ (jt - jf)
    return _f(dist, dtype), jac


def solve(m, body=(), offset=None, target_pos=None, target_quat=None, weight=None, qpos_start=None, qpos_ref=None,
          dofmask=0xFFFFFFFF, iterations=20, damping=1e-3, posture=0.0, max_step=0.0, tol=0.0, limits=True,
          com_body=-1, com_target=None, com_weight=None, geom1=(), geom2=(), clear_min=(), clear_weight=None,
          mass=None, dtype=np.float64):
    """One env's solve: (qpos [nq], err [ntask, 6], niter, com_err [3], clearance [npair], margins [niter + 1, npair]).
    margins[k, p] = |dist - clear_min| of pair p at iterate k (the last row: at the returned qpos)."""
    f = lambda x: _f(x, dtype)
    t_ = dtype
    n, nv, P = len(body), m.nv, len(geom1)
    assert n or com_body >= 0 or P
    q = f(m.qpos0 if qpos_start is None else qpos_start)
    qref = f(m.qpos0 if qpos_ref is None else qpos_ref)
    w = np.ones((n, 2), dtype) if weight is None else f(weight).reshape(n, 2)
    w = np.where(w > 0, w, 0).astype(dtype)
    if target_pos is None:
        w[:, 0] = 0
    if target_quat is None:
        w[:, 1] = 0
    cw = np.ones(3, dtype) if com_weight is None else f(com_weight)
    cw = np.where(cw > 0, cw, 0).astype(dtype)
    pw = np.ones(P, dtype) if clear_weight is None else f(clear_weight)
    cmin = f(np.broadcast_to(np.asarray(clear_min, np.float64), (P,)))
    active = np.array([bool((int(dofmask) >> d) & 1) for d in range(nv)])
    damping, posture, max_step, tol = t_(damping), t_(posture), t_(max_step), t_(tol)
    margins = []
    k = 0
    while True:
        o = frames(m, q, dtype)
        xs, e = ik.residuals(m, o, body, offset, target_pos, target_quat, dtype) if n else (np.zeros((0, 3), dtype), np.zeros((0, 6), dtype))
        res = t_(0)
        for t in range(n):
            res = max(res, w[t, 0] * np.sqrt((e[t, :3] ** 2).sum(dtype=dtype)), w[t, 1] * np.sqrt((e[t, 3:] ** 2).sum(dtype=dtype)))
        ec = np.zeros(3, dtype)
        if com_body >= 0:
            ec = np.where(cw > 0, f(com_target) - subtree_com(m, o, com_body, mass, dtype), t_(0)).astype(dtype)
            res = max(res, (cw * np.abs(ec)).max())
        dist, prow = pair_rows(m, o, geom1, geom2, dtype)
        on = dist < cmin
        pres = np.where(on, cmin - dist, t_(0)).astype(dtype)
        margins.append(np.abs(np.asarray(dist, np.float64) - np.asarray(cmin, np.float64)))
        if P:
            res = max(res, (pw * pres).max())
        if k >= iterations or (tol > 0 and res < tol):
            return q, e, k, ec, dist, np.array(margins).reshape(k + 1, P)
        H = np.diag(np.where(active, damping + posture, t_(1))).astype(dtype)
        g = np.zeros(nv, dtype)
        if posture > 0:
            g = np.where(active, posture * ik.differentiate_pos(m, qref, q, dtype), t_(0)).astype(dtype)
        rows = []  # (row, weight, residual) in the header's order
        if n:
            J = ik.task_rows(m, o, body, xs, dtype)
            for t in range(n):
                for r in range(6):
                    rows.append((J[t, r], w[t, 0] if r < 3 else w[t, 1], e[t, r]))
        if com_body >= 0:
            Jc = com_rows(m, o, com_body, mass, dtype)
            for a in range(3):
                rows.append((Jc[a], cw[a], ec[a]))
        for p in range(P):
            if on[p]:
                rows.append((prow[p], pw[p], pres[p]))
        for row, wr, er in rows:
            if not wr > 0:
                continue
            c = np.where(active, wr * row, t_(0)).astype(dtype)
            H = (H + np.outer(c, c)).astype(dtype)
            g = (g + c * (wr * er)).astype(dtype)
        dq = dr.solve(H, g, dtype)
        s = np.abs(dq).max()
        if max_step > 0 and s > max_step:
            dq = (dq * (max_step / s)).astype(dtype)
        q = ik.integrate_pos(m, q, dq, active, limits, dtype)
        k += 1
