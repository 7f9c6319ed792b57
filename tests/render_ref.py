"""fp64 reference of the ray-cast renderer (numpy, vectorised over pixels): DESIGN.md "Rendering" restated.

Geom frames come from mjcf._fk_and_mass, camera and light from the model's visual description.

    ray     pixel (i, j) of W x H: u = (2 (i + .5) / W - 1) tan(fovy / 2) W / H, v = (1 - 2 (j + .5) / H) tan(fovy / 2),
            d = normalize(R (u, v, -1)) from the camera position o (R's columns: camera x, y, z in the world)
    hit     the smallest ray parameter t in [znear, zfar] over the geoms; a sphere or cylinder-side
            quadratic gives its near root, or its far root when the near one is below znear; a capsule is
            its cylinder side (|axial coordinate| <= half length) and the outer halves of its two cap spheres
    normal  plane: its z axis, on the side facing the ray; else (p - nearest point of the axis segment) / radius
    colour  k (ambient + diffuse max(0, n . l)), l towards the light; with shadows the Lambert term is
            dropped when any geom lies on the segment from p + 1e-3 n to the light; k = geom rgb, times
            the checker colour (rgb1 for even floor(x / cell_x) + floor(y / cell_y), else rgb2) on the
            checker plane; a miss takes (1 - s) sky_rgb2 + s sky_rgb1 with s = (1 + d_z) / 2
    output  uint8(clamp(c, 0, 1) 255 + .5), depth t (+inf for a miss), seg geom id (-1 for a miss)

`render_with_mask` also returns the marginal mask: pixels whose value rests on a knife-edge decision
(re-rendered with the ray moved by +-1/1024 pixel in x or y: another geom id, hit / miss, depth moved by more
than 1e-3 relative, or a colour channel by more than 1 LSB), which an fp32 renderer may decide differently.
"""
import numpy as np

from mjx_amd import mjcf

SHADOW_EPS = 1e-3


def _dot(a, b):
    return np.sum(a * b, axis=-1)


def scene(m, qpos):
    """World centre, z axis, radius, half length and type per geom, and the kinematics they came from."""
    kin = mjcf._fk_and_mass(m, np.asarray(qpos, float))
    A = m.arrays
    pos, zax = [], []
    for g in range(m.ngeom):
        b = A["geom_bodyid"][g]
        pos.append(kin["xpos"][b] + kin["xmat"][b] @ A["geom_pos"][g])
        zax.append(kin["xmat"][b] @ mjcf.quat2mat(A["geom_quat"][g])[:, 2])
    return {"pos": np.array(pos).reshape(-1, 3), "z": np.array(zax).reshape(-1, 3), "r": A["geom_size"][:, 0],
            "h": A["geom_size"][:, 1], "type": A["geom_type"], "kin": kin}


def camera_pose(m, kin, cam):
    c = m.visual["cameras"][cam]
    b = c["body"]
    if c["mode"] == "fixed":
        return kin["xpos"][b] + kin["xmat"][b] @ np.array(c["pos"]), kin["xmat"][b] @ np.array(c["mat"]).reshape(3, 3)
    base = kin["xpos"][b] if c["mode"] == "track" else kin["subtree_com"][b]
    return base + np.array(c["pos0_" + c["mode"]]), np.array(c["mat0"]).reshape(3, 3)


def _ray_sphere(oc, d, r, tmin):
    b = -_dot(oc, d)
    q = oc + b[:, None] * d
    disc = r * r - _dot(q, q)
    th = np.sqrt(np.maximum(disc, 0.0))
    t = np.where(b - th >= tmin, b - th, b + th)
    return np.where(disc < 0, np.inf, t)


def _ray_geom(sc, g, o, d, tmin, tmax):
    """Hit parameter in [tmin, tmax] of rays (o [N, 3] or [3], d [N, 3]) against geom g, +inf for a miss."""
    a, r, h = sc["z"][g], sc["r"][g], sc["h"][g]
    oc = np.broadcast_to(o - sc["pos"][g], d.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        if sc["type"][g] == mjcf.GEOM_PLANE:
            den = d @ a
            t = np.where(np.abs(den) > 1e-9, -(oc @ a) / den, np.inf)
        elif sc["type"][g] == mjcf.GEOM_SPHERE or h == 0:
            t = _ray_sphere(oc, d, r, tmin)
        else:
            da, oa = d @ a, oc @ a
            dp, op = d - da[:, None] * a, oc - oa[:, None] * a
            A2 = _dot(dp, dp)
            tm = -_dot(op, dp) / A2
            q = op + tm[:, None] * dp
            disc = r * r - _dot(q, q)
            th = np.sqrt(np.maximum(disc, 0.0) / A2)
            ts = np.where(tm - th >= tmin, tm - th, tm + th)
            ok = (A2 > 1e-12) & (disc >= 0) & (np.abs(oa + ts * da) <= h) & (ts >= tmin) & (ts <= tmax)
            t = np.where(ok, ts, np.inf)
            for sg in (1.0, -1.0):
                tc = _ray_sphere(oc - sg * h * a, d, r, tmin)
                ok = (sg * (oa + tc * da) >= h) & (tc >= tmin) & (tc <= tmax) & (tc < t)
                t = np.where(ok, tc, t)
        return np.where((t >= tmin) & (t <= tmax), t, np.inf)


def render(m, qpos, camera, W, H, shadows=True, dx=0.0, dy=0.0, sc=None):
    """-> rgb uint8 [H, W, 3], depth [H, W], seg [H, W], colour float [H, W, 3] (clamped, x 255, unrounded).
    dx, dy move every ray off its pixel centre (in pixels)."""
    v = m.visual
    cam = mjcf.camera_id(m, camera)
    sc = scene(m, qpos) if sc is None else sc
    o, R = camera_pose(m, sc["kin"], cam)
    th = np.tan(0.5 * np.deg2rad(v["cameras"][cam]["fovy"]))
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    u = (2 * (ii.ravel() + 0.5 + dx) / W - 1) * th * W / H
    w = (1 - 2 * (jj.ravel() + 0.5 + dy) / H) * th
    d = np.stack([u, w, -np.ones_like(u)], axis=1) @ R.T
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    N = d.shape[0]
    tbest, hit = np.full(N, np.inf), np.full(N, -1)
    for g in range(m.ngeom):
        t = _ray_geom(sc, g, o, d, v["znear"], v["zfar"])
        better = t < tbest
        tbest, hit = np.where(better, t, tbest), np.where(better, g, hit)
    s = 0.5 * (1 + d[:, 2])
    col = (1 - s)[:, None] * np.array(v["sky"]["rgb2"]) + s[:, None] * np.array(v["sky"]["rgb1"])
    idx = np.nonzero(hit >= 0)[0]
    if idx.size:
        hg = hit[idx]
        p = o + tbest[idx, None] * d[idx]
        vv = p - sc["pos"][hg]
        a = sc["z"][hg]
        plane = sc["type"][hg] == mjcf.GEOM_PLANE
        sgn = np.where(_dot(a, d[idx]) < 0, 1.0, -1.0)
        hl = np.where(sc["type"][hg] == mjcf.GEOM_CAPSULE, sc["h"][hg], 0.0)
        sax = np.clip(_dot(vv, a), -hl, hl)
        with np.errstate(divide="ignore", invalid="ignore"):
            nrm = np.where(plane[:, None], sgn[:, None] * a, (vv - sax[:, None] * a) / sc["r"][hg][:, None])
        L = v["light"]
        if L["directional"]:
            ld = np.broadcast_to(-np.array(L["dir"]), p.shape)
            tl = np.full(idx.size, np.inf)
        else:
            ld = np.array(L["pos"]) - p
            tl = np.linalg.norm(ld, axis=1)
            ld = ld / tl[:, None]
        lam = np.maximum(0.0, _dot(nrm, ld))
        if shadows:
            so = p + SHADOW_EPS * nrm
            occ = np.zeros(idx.size, bool)
            for g in range(m.ngeom):
                occ |= np.isfinite(_ray_geom(sc, g, so, ld, 0.0, tl))
            lam = np.where(occ, 0.0, lam)
        base = np.array(v["geom_rgba"])[hg, :3]
        ck = v["checker"]
        if ck is not None:
            Rg = sc["kin"]["xmat"][m.arrays["geom_bodyid"][ck["geom"]]]
            x, y = Rg @ np.array(ck["xaxis"]), Rg @ np.array(ck["yaxis"])
            par = (np.floor(_dot(vv, x) / ck["cell"][0]) + np.floor(_dot(vv, y) / ck["cell"][1])) % 2
            ckc = np.where((par == 0)[:, None], np.array(ck["rgb1"]), np.array(ck["rgb2"]))
            base = np.where((hg == ck["geom"])[:, None], base * ckc, base)
        col[idx] = base * (np.array(L["ambient"]) + np.array(L["diffuse"]) * lam[:, None])
    colf = np.clip(col, 0.0, 1.0) * 255.0
    rgb = (colf + 0.5).astype(np.uint8)
    return rgb.reshape(H, W, 3), tbest.reshape(H, W), hit.reshape(H, W), colf.reshape(H, W, 3)


def render_with_mask(m, qpos, camera, W, H, shadows=True, shift=1.0 / 1024):
    """render(...) plus the marginal mask [H, W] (see the module docstring)."""
    sc = scene(m, qpos)
    rgb, dep, seg, colf = render(m, qpos, camera, W, H, shadows, sc=sc)
    marg = np.zeros((H, W), bool)
    for dx, dy in ((shift, 0), (-shift, 0), (0, shift), (0, -shift)):
        _, d2, s2, c2 = render(m, qpos, camera, W, H, shadows, dx, dy, sc=sc)
        marg |= s2 != seg
        both = np.isfinite(dep) & np.isfinite(d2)
        with np.errstate(invalid="ignore"):
            marg |= both & (np.abs(d2 - dep) > 1e-3 * np.abs(dep))
        marg |= np.isfinite(dep) != np.isfinite(d2)
        marg |= (np.abs(c2 - colf) > 1.0).any(axis=2)
    return rgb, dep, seg, marg
