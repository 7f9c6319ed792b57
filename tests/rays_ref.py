"""fp64 reference of the ray casts (mjl_ray / mjl_ray_scan), on render_ref.scene and render_ref._ray_geom, and the
inputs the ray tests share.

    one ray   t = min over the geoms that pass the filter of _ray_geom(geom, pnt, vec / |vec|, tmin = 0,
              tmax = cutoff |vec| or inf) / |vec|; the lowest geom id wins a tie; a miss is dist = -1, geomid = -1
    filter    geoms of body `bodyexclude` are skipped (-1: none); geoms of body 0 unless flg_static
    scan      frame rotation R, origin p (xbody: xmat, xpos; site: xmat[b] quat2mat(site_quat), xpos[b] +
              xmat[b] site_pos); "pose": pnt = p + R lpnt, vec = R lvec; "yaw": R replaced by the rotation about
              world z by psi = atan2(R[1][0], R[0][0]), psi = 0 when R[0][0]^2 + R[1][0]^2 < 1e-12
    hitpos    pnt + dist vec, pnt on a miss
    marginal  a ray whose outcome changes when every radius and half length is scaled by 1 +- 1e-3 or the origin
              moves +- 1e-4 m along a world axis: a ray grazing a surface, which fp32 kinematics may decide
              differently. "Changes": hit / miss flips, geomid changes, or dist moves by more than ten times
              (the distance tolerance + the perturbation's own displacement: 1e-4 m for a shift, 1e-3 (r + h) of
              the hit geom for a scaling). The displacement term is needed because the measured tolerance (3e-6 m)
              is far below the perturbations: a shift of 1e-4 m along the ray moves dist by 1e-4 m on any
              surface, so "more than 10 x tolerance" alone would call every ray marginal. With the term, a ray
              is marginal when the surface amplifies the perturbation more than tenfold (incidence within about
              6 degrees of tangent) or the decision flips; the set is a subset of the literal one.
"""
import numpy as np

import mjx_amd
from mjx_amd import mjcf, rays

import render_ref as rr

NENV, NRAY = 3, 70
SCALE_EPS, SHIFT_EPS = 1e-3, 1e-4
MARGINAL_CAP = 0.05


def cast(m, sc, pnt, vec, flg_static=True, bodyexclude=-1, cutoff=0.0):
    """(dist [N], geomid [N]) of rays pnt [N, 3], vec [N, 3] against scene `sc` of model `m`."""
    pnt, vec = np.asarray(pnt, float).reshape(-1, 3), np.asarray(vec, float).reshape(-1, 3)
    ln = np.linalg.norm(vec, axis=1)
    ok = ln > 0
    d = vec / np.where(ok, ln, 1.0)[:, None]
    tmax = cutoff * ln if cutoff > 0 else np.full(len(ln), np.inf)
    best, hit = np.full(len(ln), np.inf), np.full(len(ln), -1)
    for g in range(m.ngeom):
        b = int(m.arrays["geom_bodyid"][g])
        if b == bodyexclude or (b == 0 and not flg_static):
            continue
        t = rr._ray_geom(sc, g, pnt, d, 0.0, tmax)
        better = ok & (t < best)
        best, hit = np.where(better, t, best), np.where(better, g, hit)
    return np.where(hit >= 0, best / np.where(ok, ln, 1.0), -1.0), hit


def frame(m, kin, objtype, objid):
    """Rotation and origin of an xbody's or a site's frame."""
    if objtype == "xbody":
        return kin["xmat"][objid], kin["xpos"][objid]
    A = m.arrays
    b = int(A["site_bodyid"][objid])
    return kin["xmat"][b] @ mjcf.quat2mat(A["site_quat"][objid]), kin["xpos"][b] + kin["xmat"][b] @ A["site_pos"][objid]


def scan_rays(m, kin, objtype, objid, align, lpnt, lvec):
    """World (pnt, vec) of the frame's pattern."""
    R, p = frame(m, kin, objtype, objid)
    if align == "yaw":
        psi = 0.0 if R[0, 0] ** 2 + R[1, 0] ** 2 < 1e-12 else np.arctan2(R[1, 0], R[0, 0])
        c, s = np.cos(psi), np.sin(psi)
        R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    return p + np.asarray(lpnt, float) @ R.T, np.asarray(lvec, float) @ R.T


def hitpos(pnt, vec, dist):
    return pnt + np.where(dist >= 0, dist, 0.0)[:, None] * vec


def marginal(m, sc, pnt, vec, tol, **kw):
    """The marginal mask [N] of the rays (module docstring) at distance tolerance `tol`."""
    d0, g0 = cast(m, sc, pnt, vec, **kw)
    marg = np.zeros(len(d0), bool)

    size = (sc["r"] + sc["h"])[np.maximum(g0, 0)]

    def differs(d1, g1, delta):
        return (g1 != g0) | (np.abs(d1 - d0) > 10 * (tol + delta))
    for s in (1 + SCALE_EPS, 1 - SCALE_EPS):
        marg |= differs(*cast(m, dict(sc, r=sc["r"] * s, h=sc["h"] * s), pnt, vec, **kw), SCALE_EPS * size)
    for ax in range(3):
        for sg in (1.0, -1.0):
            marg |= differs(*cast(m, sc, pnt + sg * SHIFT_EPS * np.eye(3)[ax], vec, **kw), SHIFT_EPS)
    return marg


# ---- the inputs of the GPU tests (tests/test_rays_gpu.py), and of the CPU test of their marginal share

def poses(m, seed=5, pitch=None):
    """NENV poses, rounded to float32: joint angles within +-0.4 rad of qpos0, a tilted root, different heights.
    pitch: every root pitched by that angle about y instead (a yaw about z on top, different per env)."""
    rng = np.random.default_rng(seed)
    Q = np.tile(m.qpos0, (NENV, 1))
    Q[:, 7:] += rng.uniform(-0.4, 0.4, (NENV, m.nq - 7))
    Q[:, 2] += np.array([0.0, 0.35, -0.2])
    for e in range(NENV):
        if pitch is None:
            ax = rng.normal(size=3)
            ang = rng.uniform(0.2, 0.6)
            q = np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * ax / np.linalg.norm(ax)])
        else:
            yaw = 0.7 * e - 0.5
            q = mjcf.quat_mul(np.array([np.cos(yaw / 2), 0, 0, np.sin(yaw / 2)]),
                              np.array([np.cos(pitch / 2), 0, np.sin(pitch / 2), 0]))
        Q[e, 3:7] = q
    return np.float32(Q).astype(np.float64)


def world_rays(m, Q, nray=NRAY, seed=9):
    """[nenv, nray, 3] origins and unit directions (float32-rounded): ray 0 straight down onto the floor from
    beside the root, ray 1 up, ray 2 from the centre of the torso capsule, the rest from a 2 m box around the
    root towards random points of random bodies' geoms."""
    rng = np.random.default_rng(seed)
    n = Q.shape[0]
    P, V = np.zeros((n, nray, 3)), np.zeros((n, nray, 3))
    torso = m.names["geom"].index("torso")
    for e in range(n):
        sc = rr.scene(m, Q[e])
        root = Q[e, :3]
        for r in range(nray):
            o = root + rng.uniform(-1.0, 1.0, 3)
            o[2] = max(o[2], 0.05)
            g = int(rng.integers(1, m.ngeom))
            tgt = sc["pos"][g] + sc["z"][g] * rng.uniform(-1, 1) * sc["h"][g] * (sc["type"][g] == mjcf.GEOM_CAPSULE) \
                + rng.normal(size=3) * 0.3 * sc["r"][g]
            v = tgt - o
            if r == 0 or (r > 2 and r % 9 == 0):
                v = np.array([0.0, 0.0, -1.0])
            elif r == 1 or (r > 2 and r % 9 == 1):
                v = np.array([0.0, 0.0, 1.0])
            if r == 0:
                o = root + np.array([1.5, 1.5, 0.3])
            if r == 2:
                o = sc["pos"][torso] + 0.3 * sc["r"][torso] * np.array([0.3, -0.2, 0.4])
            P[e, r], V[e, r] = o, v / np.linalg.norm(v)
    P, V = np.float32(P).astype(np.float64), np.float32(V).astype(np.float64)
    return P, V


def patterns():
    """The scan tests' patterns by name: (frame, align, (lpnt, lvec), bodyexclude)."""
    fan = rays.fan_pattern(24, 300.0, -35.0)
    grid = rays.grid_pattern(5, 7, 0.15, 0.1, 0.5)
    up = (np.zeros((1, 3), np.float32), np.array([[0.0, 0.0, 1.0]], np.float32))
    return {"torso_pose_fan": ("torso", "pose", fan, "self"),
            "foot_site_grid": ("site_foot_left", "pose", rays.grid_pattern(3, 4, 0.1, 0.1, 0.6), -1),
            "foot_rangefinder": ("site_foot_right", "pose", up, "self"),
            "torso_yaw_grid": ("torso", "yaw", grid, "self"),
            "torso_pose_grid": ("torso", "pose", grid, "self")}


def frame_ids(m, name):
    """("xbody" | "site", id, carrying body) of a frame name."""
    if name in m.names["body"]:
        b = m.names["body"].index(name)
        return "xbody", b, b
    s = m.names["site"].index(name)
    return "site", s, int(m.arrays["site_bodyid"][s])


def cases(m):
    """Every (label, qpos [nq], pnt [N, 3], vec [N, 3], kwargs of cast) the GPU tests compare, one entry per env."""
    out = []
    Q = poses(m)
    P, V = world_rays(m, Q)
    tb = m.names["body"].index("torso")
    for e in range(NENV):
        sc = rr.scene(m, Q[e])
        d0, _ = cast(m, sc, P[e], V[e])
        for label, kw in (("all", {}), ("nostatic", {"flg_static": False}), ("notorso", {"bodyexclude": tb}),
                          ("cutoff", {"cutoff": cutoff_of(m, Q, P, V)})):
            out.append((f"world {label} env {e}", Q[e], P[e], V[e], kw))
    P1, V1 = world_rays(m, Q[:1], 1, seed=9)
    P257, V257 = world_rays(m, Q[:1], 257, seed=10)
    out.append(("chunk 1", Q[0], P1[0], V1[0], {}))
    out.append(("chunk 257", Q[0], P257[0], V257[0], {}))
    for name, (fr, align, (lp, lv), excl) in patterns().items():
        Qs = poses(m, seed=6, pitch=0.5) if "grid" in name and fr == "torso" else Q
        kind, i, body = frame_ids(m, fr)
        for e in range(NENV):
            sc = rr.scene(m, Qs[e])
            p, v = scan_rays(m, sc["kin"], kind, i, align, lp, lv)
            out.append((f"scan {name} env {e}", Qs[e], p, v, {"bodyexclude": body if excl == "self" else excl}))
    Q2 = poses(m, seed=21)
    fr, align, (lp, lv), excl = patterns()["torso_yaw_grid"]
    kind, i, body = frame_ids(m, fr)
    for e in range(NENV):
        sc = rr.scene(m, Q2[e])
        p, v = scan_rays(m, sc["kin"], kind, i, align, lp, lv)
        out.append((f"capture replay env {e}", Q2[e], p, v, {"bodyexclude": body}))
    return out


def cutoff_of(m, Q, P, V):
    """A cutoff shorter than the median reference hit of the world rays, off every hit distance by > 1e-3 relative."""
    d = np.concatenate([cast(m, rr.scene(m, Q[e]), P[e], V[e])[0] for e in range(Q.shape[0])])
    d = np.sort(d[d >= 0])
    k = len(d) // 2 - 1
    while k > 0 and d[k + 1] - d[k] < 4e-3 * d[k]:
        k -= 1
    return float(np.float32(0.5 * (d[k] + d[k + 1])))


def load_tolerances():
    import json
    import os
    p = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "rays", "tolerances.json")
    with open(p) as f:
        return json.load(f)
