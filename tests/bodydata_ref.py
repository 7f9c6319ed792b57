"""Reference for the body-level readout (mjl_body_data / mjx.body_data): a numpy restatement of the table in
include/mjx355.h as plain sums over bodies (no spatial-algebra recursion). Body origins' x, R, w, dw, v, a come
from sensors_ref.kinematics; qacc and the contact list (con_pos, con_frame, con_geom, efc_force, efc_type) from
the oracle's forward outputs of the same state (oracle.state_arrays); the xfrc_applied rows from the caller.
`dtype=np.float32` evaluates the same formulas in float32: the yardstick of the GPU test's tolerances.

ximat is not in `body_data`'s dict: where principal moments coincide (every capsule) the principal axes are not
unique, so the tests check it by what defines it (principal_moments, check_ximat)."""
import numpy as np

import sensors_ref as sr

FIELDS = ("xipos", "subtree_com", "cinert", "cvel", "subtree_linvel", "subtree_angmom", "cfrc_ext", "cfrc_int")


def _tensor(t, dt):
    return np.array([[t[0], t[3], t[4]], [t[3], t[1], t[5]], [t[4], t[5], t[2]]], dt)


def contact_forces(m, o):
    """Per oracle contact the contact-frame force (normal, t1, t2) from efc_force / efc_type: the contact rows
    follow the limit rows (types 0 / 1); a type-2 contact has one row, a pyramidal (type-3) one four."""
    pair = {(int(g1), int(g2)): p for p, (g1, g2) in enumerate(zip(m.pair_geom1, m.pair_geom2))}
    typ, f = o["efc_type"], o["efc_force"]
    adr, out = int((typ < 2).sum()), []
    for j in range(int(o["ncon"])):
        mu = m.pair_friction[pair[tuple(int(x) for x in o["con_geom"][j])]][0]
        if typ[adr] == 2:
            out.append(np.array([f[adr], 0.0, 0.0]))
            adr += 1
        else:
            r = f[adr:adr + 4]
            out.append(np.array([r.sum(), (r[0] - r[1]) * mu, (r[2] - r[3]) * mu]))
            adr += 4
    assert adr == len(f)
    return out


def body_data(m, o, xfrc=None, mass=None, inertia=None, dtype=np.float64):
    """{field: [nbody, k]} of the state behind the oracle's forward outputs `o`. xfrc [nbody, 6] (force, torque at
    xipos) or None; mass [nbody] / inertia [nbody, 6] replace the model's (per-env parameters)."""
    dt, A, nb = dtype, m.arrays, m.nbody
    k = sr.kinematics(m, o["qpos"], o["qvel"], o["qacc"], dt)
    g = np.asarray(m.gravity, dt)
    ms = np.asarray(A["body_mass"] if mass is None else mass, dt)
    ten = np.asarray(A["body_inertia"] if inertia is None else inertia, dt).reshape(nb, 6)
    end, root = [int(x) for x in A["body_subtree_end"]], [int(x) for x in A["body_rootid"]]
    xi, vc, ac = (np.zeros((nb, 3), dt) for _ in range(3))
    Iw = np.zeros((nb, 3, 3), dt)
    for b in range(1, nb):
        d = k["R"][b] @ np.asarray(A["body_ipos"][b], dt)
        w, dw = k["w"][b], k["dw"][b]
        xi[b] = k["x"][b] + d
        vc[b] = k["v"][b] + np.cross(w, d)
        ac[b] = k["a"][b] + np.cross(dw, d) + np.cross(w, np.cross(w, d))
        Iw[b] = k["R"][b] @ _tensor(ten[b], dt) @ k["R"][b].T
    out = {f: np.zeros((nb, n), dt) for f, n in zip(FIELDS, (3, 3, 10, 6, 3, 3, 6, 6))}
    out["xipos"] = xi
    for b in range(nb):
        sub = range(b, end[b])
        M = sum(ms[j] for j in sub)
        if M < 1e-15:
            out["subtree_com"][b] = xi[b]
            continue
        out["subtree_com"][b] = sum(ms[j] * xi[j] for j in sub) / M
        out["subtree_linvel"][b] = sum(ms[j] * vc[j] for j in sub) / M
        out["subtree_angmom"][b] = sum(Iw[j] @ k["w"][j] + ms[j] * np.cross(xi[j] - out["subtree_com"][b],
                                                                          vc[j] - out["subtree_linvel"][b]) for j in sub)
    c0 = np.array([out["subtree_com"][root[b]] for b in range(nb)])
    ext = out["cfrc_ext"]
    if xfrc is not None:
        for b in range(1, nb):
            f, t = np.asarray(xfrc[b][:3], dt), np.asarray(xfrc[b][3:], dt)
            ext[b, :3] += t + np.cross(xi[b] - c0[b], f)
            ext[b, 3:] += f
    for j, fc in enumerate(contact_forces(m, o)):
        F = np.asarray(np.asarray(o["con_frame"][j]).reshape(3, 3).T @ fc, dt)
        pos = np.asarray(o["con_pos"][j], dt)
        for geom, sign in ((o["con_geom"][j][1], 1), (o["con_geom"][j][0], -1)):
            b = int(A["geom_bodyid"][int(geom)])
            if b > 0:
                ext[b, :3] += sign * np.cross(pos - c0[b], F)
                ext[b, 3:] += sign * F
    net = np.zeros((nb, 6), dt)
    for b in range(1, nb):
        r, w = xi[b] - c0[b], k["w"][b]
        I = Iw[b] + ms[b] * (np.dot(r, r) * np.eye(3, dtype=dt) - np.outer(r, r))
        out["cinert"][b] = [I[0, 0], I[1, 1], I[2, 2], I[0, 1], I[0, 2], I[1, 2], *(ms[b] * r), ms[b]]
        out["cvel"][b] = np.concatenate([w, vc[b] + np.cross(w, c0[b] - xi[b])])
        f = ms[b] * (ac[b] - g)
        net[b] = np.concatenate([Iw[b] @ k["dw"][b] + np.cross(w, Iw[b] @ w) + np.cross(r, f), f]) - ext[b]
    for b in range(1, nb):
        out["cfrc_int"][b] = net[b:end[b]].sum(0)
    return out


def balance_scale(m, ref, mass=None):
    """The scale the free root's cfrc_int is small against: sum_b |cfrc_ext[b]| + M |g|."""
    M = float(np.sum(m.arrays["body_mass"] if mass is None else mass))
    return float(np.abs(ref["cfrc_ext"]).sum() + M * np.linalg.norm(m.gravity))


def principal_moments(m, inertia=None):
    """[nbody, 3]: the eigenvalues of each body-frame tensor, descending (MuJoCo's body_inertia)."""
    ten = np.asarray(m.arrays["body_inertia"] if inertia is None else inertia, np.float64).reshape(m.nbody, 6)
    return np.array([np.linalg.eigvalsh(_tensor(t, np.float64))[::-1] for t in ten])


def check_ximat(m, o, ximat, tol):
    """ximat [nbody, 3, 3] is xmat quat2mat(body_iquat): proper rotations that diagonalise the world inertia
    R T R' with the principal moments in descending order; where the three moments are distinct (relative gap >
    1e-3) its columns are the eigenvectors up to sign. Returns the worst error over `tol`-scaled checks."""
    k = sr.kinematics(m, o["qpos"])
    pm = principal_moments(m)
    worst = 0.0
    for b in range(1, m.nbody):
        X = np.asarray(ximat[b], np.float64)
        Iw = k["R"][b] @ _tensor(np.asarray(m.arrays["body_inertia"][b], np.float64), np.float64) @ k["R"][b].T
        scale = max(pm[b, 0], 1e-12)
        errs = [np.abs(X @ X.T - np.eye(3)).max(), abs(np.linalg.det(X) - 1.0),
                np.abs(X @ np.diag(pm[b]) @ X.T - Iw).max() / scale]
        if pm[b, 0] > 0 and min(pm[b, 0] - pm[b, 1], pm[b, 1] - pm[b, 2]) > 1e-3 * pm[b, 0]:
            V = np.linalg.eigh(Iw)[1][:, ::-1]
            errs.append(np.abs(np.abs(np.sum(V * X, 0)) - 1.0).max())
        worst = max(worst, max(errs))
        assert max(errs) <= tol, (b, errs, tol)
    return worst
