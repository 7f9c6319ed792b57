"""Ray casts (mjl_ray / mjl_ray_scan, mjx.ray / mjx.ray_scan, HumanoidEnv.scan) on the GPU against the float64
reference tests/rays_ref.py.

Both humanoids, 3 envs with different poses (random joint angles, a tilted root, different heights) written with
d.set("qpos") and no forward call: the launch does its own kinematics. 70 world rays per env (more than one
wavefront: aimed at random bodies from a 2 m box, down, up, one from inside the torso capsule), the scan patterns
of rays_ref.patterns(), 1 and 257 rays on one env.

Marginal rays (rays_ref.marginal: the reference outcome changes under a 1e-3 scaling of the sizes or a 1e-4 m shift
of the origin) are left out of the dist / geomid / hitpos comparison only; tests/test_rays.py asserts on the CPU
that they are at most 5 % of every case here. geomid is compared exactly. The dist and hitpos tolerances are
profiles/rays/tolerances.json: four times the largest error tools/ray_tolerances.py measured with this file's
`measure` on these cases, rounded up to one significant digit."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import mjx_amd
from mjx_amd import abi, mjx
from mjx_amd._header import HEADER
from mjx_amd._lib import MjlError, lib
from mjx_amd.config import reference_ppo_config
from mjx_amd.envs import HumanoidEnv, resolve_ids

import render_ref as rr
import rays_ref as rf

pytestmark = pytest.mark.gpu

SENTINEL = -77.25
NENV = rf.NENV


def _data(sys_, Q):
    d = mjx.make_data(sys_, Q.shape[0])
    d.set("qpos", torch.tensor(Q, dtype=torch.float32))  # and no forward
    return d


def _t(x):
    return torch.tensor(np.asarray(x), dtype=torch.float32, device="cuda")


def _np(t):
    return None if t is None else t.cpu().numpy()


def compare(m, label, q, pnt, vec, kw, dist, geomid, hp, tol, errs=None):
    """One env's rays against the reference; returns (max dist error, max hitpos error) over the non-marginal rays.
    tol = (marginal tolerance, dist bound, hitpos bound); a bound of None is not asserted (measurement)."""
    sc = rr.scene(m, q)
    dref, gref = rf.cast(m, sc, pnt, vec, **kw)
    keep = ~rf.marginal(m, sc, pnt, vec, tol[0], **kw)
    ed = np.abs(np.asarray(dist, np.float64) - dref)[keep].max() if keep.any() else 0.0
    eh = 0.0
    if hp is not None and keep.any():
        eh = np.abs(np.asarray(hp, np.float64) - rf.hitpos(pnt, vec, dref))[keep].max()
    print(f"{m.name} {label}: {int((~keep).sum())}/{len(keep)} marginal, max |dist - ref| {ed:.3e}, hitpos {eh:.3e}")
    if errs is not None:
        errs.append((ed, eh))
    if geomid is not None:
        np.testing.assert_array_equal(np.asarray(geomid)[keep], gref[keep], err_msg=label)
    else:
        np.testing.assert_array_equal((np.asarray(dist) < 0)[keep], (gref < 0)[keep], err_msg=label)
    if tol[1] is not None:
        assert ed <= tol[1], f"{label}: dist error {ed:.3e} > {tol[1]:.1e}"
        assert eh <= tol[2], f"{label}: hitpos error {eh:.3e} > {tol[2]:.1e}"
    return dref, gref, keep


def _tol():
    t = rf.load_tolerances()
    return t["dist_tol"], t["dist_tol"], t["hitpos_tol"]


@pytest.fixture(scope="module", params=mjx_amd.BUILTIN_MODELS)
def setup(request):
    m = mjx_amd.load_model(request.param)
    Q = rf.poses(m)
    P, V = rf.world_rays(m, Q)
    return m, mjx.put_model(m), Q, P, V


def run_world(m, sys_, Q, P, V, tol, errs=None):
    d = _data(sys_, Q)
    tb = m.names["body"].index("torso")
    cut = rf.cutoff_of(m, Q, P, V)
    res = {}
    for label, kw, args in (("all", {}, {}), ("nostatic", {"flg_static": False}, {"flg_static": False}),
                            ("notorso", {"bodyexclude": tb}, {"bodyexclude": "torso"}),
                            ("cutoff", {"cutoff": cut}, {"cutoff": cut})):
        dist, gid = mjx.ray(sys_, d, _t(P), _t(V), **args)
        dist, gid = _np(dist), _np(gid)
        res[label] = (dist, gid, [compare(m, f"world {label} env {e}", Q[e], P[e], V[e], kw, dist[e], gid[e], None, tol, errs)
                                  for e in range(NENV)])
    return res, cut


def test_world_rays(setup):
    m, sys_, Q, P, V = setup
    res, cut = run_world(m, sys_, Q, P, V, _tol())
    A = m.arrays
    dist, gid, ref = res["all"]
    assert (gid == 0).any() and (gid > 0).any() and (gid < 0).any()  # floor, body and miss all occur
    for e in range(NENV):  # ray 0 lands on the floor; ray 2 starts inside the torso capsule and reports a way out
        assert gid[e, 0] == 0 and abs(dist[e, 0] - P[e, 0, 2]) < 1e-5
        assert gid[e, 2] > 0 and dist[e, 2] > 0
    dist, gid, _ = res["nostatic"]
    assert not (gid == 0).any() and (dist[gid < 0] == -1).all()
    dist, gid, _ = res["notorso"]
    tb = m.names["body"].index("torso")
    assert not np.isin(gid, np.flatnonzero(A["geom_bodyid"] == tb)).any()
    assert (res["notorso"][1] != res["all"][1]).any()  # the next hit behind the torso is reported somewhere
    # a cutoff below the median hit turns exactly the longer hits into misses
    dist, gid, cref = res["cutoff"]
    d_all, g_all, ref_all = res["all"]
    for e in range(NENV):
        dref, gref, keep = ref_all[e]
        keep = keep & cref[e][2]
        longer = (dref > cut) | (dref < 0)
        assert (dist[e][keep & longer] == -1).all() and (gid[e][keep & longer] == -1).all()
        np.testing.assert_array_equal(gid[e][keep & ~longer], gref[keep & ~longer])
    nhit = sum(int(((r[0] >= 0) & r[2]).sum()) for r in ref_all)
    ncut = sum(int(((r[0] >= 0) & r[2]).sum()) for r in cref)
    assert 0 < ncut < nhit and ncut <= nhit // 2 + 1
    # geomid = None is accepted, [nray, 3] and [3] inputs broadcast over the envs
    d = _data(sys_, Q)
    out = torch.full((NENV, rf.NRAY), SENTINEL, device="cuda")
    d1, g1 = mjx.ray(sys_, d, _t(P), _t(V), out=(out, None))
    assert g1 is None and d1 is out and np.array_equal(_np(out), d_all)
    d2, g2 = mjx.ray(sys_, d, P[0], V[0])
    np.testing.assert_array_equal(_np(d2)[0], d_all[0])
    d3, g3 = mjx.ray(sys_, d, P[0, 0], V[0, 0])
    assert tuple(d3.shape) == (NENV, 1) and _np(d3)[0, 0] == d_all[0, 0]
    # a vec that is not unit: the same surface point, dist scaled
    d4, g4 = mjx.ray(sys_, d, _t(P), _t(2.0 * V))
    np.testing.assert_array_equal(_np(g4), g_all)
    np.testing.assert_allclose(2.0 * _np(d4)[g_all >= 0], d_all[g_all >= 0], rtol=1e-6)


def test_mask_keeps_rows(setup):
    m, sys_, Q, P, V = setup
    d = _data(sys_, Q)
    mask = torch.tensor([1.0, 0.0, 1.0])
    dist = torch.full((NENV, rf.NRAY), SENTINEL, device="cuda")
    gid = torch.full((NENV, rf.NRAY), -7, dtype=torch.int32, device="cuda")
    hp = torch.full((NENV, rf.NRAY, 3), SENTINEL, device="cuda")
    mjx.ray(sys_, d, _t(P), _t(V), mask=mask, out=(dist, gid))
    assert (dist[1] == SENTINEL).all() and (gid[1] == -7).all()
    full_d, full_g = mjx.ray(sys_, d, _t(P), _t(V))
    for e in (0, 2):
        assert torch.equal(dist[e], full_d[e]) and torch.equal(gid[e], full_g[e])
        compare(m, f"mask env {e}", Q[e], P[e], V[e], {}, _np(dist[e]), _np(gid[e]), None, _tol())
    lp, lv = rf.patterns()["torso_pose_fan"][2]
    dist = torch.full((NENV, len(lp)), SENTINEL, device="cuda")
    mjx.ray_scan(sys_, d, "torso", lp, lv, mask=mask, out=(dist, None, hp[:, :len(lp)].contiguous()))
    assert (dist[1] == SENTINEL).all() and (dist[0] != SENTINEL).all()


def run_chunks(m, sys_, Q, tol, errs=None):
    for nray, seed in ((1, 9), (257, 10)):
        P, V = rf.world_rays(m, Q[:1], nray, seed=seed)
        d = _data(sys_, Q[:1])
        got = []
        for chunk in (0, 100, 65535):  # the library's choice, a ragged chunk, kinematics once per env
            d.set_option(abi.OPT_RAY_CHUNK, chunk)
            dist, gid = mjx.ray(sys_, d, _t(P), _t(V))
            got.append((_np(dist), _np(gid)))
        for dist, gid in got[1:]:  # the layout does not change a bit
            np.testing.assert_array_equal(dist, got[0][0])
            np.testing.assert_array_equal(gid, got[0][1])
        compare(m, f"chunk {nray}", Q[0], P[0], V[0], {}, got[0][0][0], got[0][1][0], None, tol, errs)


def test_chunking_edges(setup):
    m, sys_, Q, P, V = setup
    run_chunks(m, sys_, Q, _tol())


def run_scans(m, sys_, Q, tol, errs=None):
    res = {}
    for name, (fr, align, (lp, lv), excl) in rf.patterns().items():
        Qs = rf.poses(m, seed=6, pitch=0.5) if "grid" in name and fr == "torso" else Q
        kind, i, body = rf.frame_ids(m, fr)
        d = _data(sys_, Qs)
        frame = fr if name != "foot_site_grid" else ("site", i)  # both ways of naming a frame
        dist, gid, hp = (_np(x) for x in mjx.ray_scan(sys_, d, frame, lp, lv, align=align, bodyexclude=excl))
        for e in range(NENV):
            p, v = rf.scan_rays(m, rr.scene(m, Qs[e])["kin"], kind, i, align, lp, lv)
            compare(m, f"scan {name} env {e}", Qs[e], p, v, {"bodyexclude": body if excl == "self" else excl},
                    dist[e], gid[e], hp[e], tol, errs)
        res[name] = (dist, gid, hp)
    return res


def test_scans(setup):
    m, sys_, Q, P, V = setup
    res = run_scans(m, sys_, Q, _tol())
    A = m.arrays
    # the rangefinder never reports its own body
    foot = int(A["site_bodyid"][m.names["site"].index("site_foot_right")])
    assert not np.isin(res["foot_rangefinder"][1], np.flatnonzero(A["geom_bodyid"] == foot)).any()
    # a level grid 0.5 m above a torso pitched by 0.5 rad: the yaw result is not the pose result
    dy, dp = res["torso_yaw_grid"][0], res["torso_pose_grid"][0]
    assert np.abs(dy - dp).max() > 0.05
    # hitpos = None is accepted
    lp, lv = rf.patterns()["torso_pose_fan"][2]
    d = _data(sys_, Q)
    dist = torch.full((NENV, len(lp)), SENTINEL, device="cuda")
    out = mjx.ray_scan(sys_, d, "torso", lp, lv, bodyexclude="self", out=(dist, None, None))
    assert out[1] is None and out[2] is None
    np.testing.assert_array_equal(_np(dist), res["torso_pose_fan"][0])


def run_capture(m, sys_, tol, errs=None):
    cfg = resolve_ids(m, dataclasses.replace(reference_ppo_config().env_config, max_episode_steps=1000))
    fr, align, pattern, excl = rf.patterns()["torso_yaw_grid"]
    kind, i, body = rf.frame_ids(m, fr)
    Q1, Q2 = rf.poses(m, seed=6, pitch=0.5), rf.poses(m, seed=21)
    env = HumanoidEnv(sys_, cfg, NENV, seed=3)
    qbuf = _t(Q1)
    env.data.set("qpos", qbuf)
    dist, gid, hp = env.scan(fr, pattern, align=align)  # eager: allocates the buffers, warms the kernel up
    torch.cuda.synchronize()
    eager = _np(dist).copy()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.data.set("qpos", qbuf)
        out = env.scan(fr, pattern, align=align)
    assert out[0] is dist and out[1] is gid and out[2] is hp  # the preallocated tensors again
    qbuf.copy_(_t(Q2))
    g.replay()
    torch.cuda.synchronize()
    got = _np(dist), _np(gid), _np(hp)
    assert np.abs(got[0] - eager).max() > 1e-2  # the replay saw the new state
    for e in range(NENV):
        p, v = rf.scan_rays(m, rr.scene(m, Q2[e])["kin"], kind, i, align, *pattern)
        compare(m, f"capture replay env {e}", Q2[e], p, v, {"bodyexclude": body}, got[0][e], got[1][e], got[2][e], tol, errs)


def test_captured_scan(setup):
    m, sys_, Q, P, V = setup
    run_capture(m, sys_, _tol())


def measure():
    """{model: (max dist error, max hitpos error)} of the built kernel over the non-marginal rays of every case
    above (tools/ray_tolerances.py), marginal rays taken at the tolerance on file or, without one, 2.5e-5 m."""
    try:
        t0 = rf.load_tolerances()["dist_tol"]
    except (OSError, KeyError):
        t0 = 2.5e-5
    out = {}
    for name in mjx_amd.BUILTIN_MODELS:
        m = mjx_amd.load_model(name)
        sys_, errs = mjx.put_model(m), []
        Q = rf.poses(m)
        P, V = rf.world_rays(m, Q)
        tol = (t0, None, None)
        run_world(m, sys_, Q, P, V, tol, errs)
        run_chunks(m, sys_, Q, tol, errs)
        run_scans(m, sys_, Q, tol, errs)
        run_capture(m, sys_, tol, errs)
        out[name] = (max(e[0] for e in errs), max(e[1] for e in errs))
    return out


def test_argument_errors(setup):
    m, sys_, Q, P, V = setup
    L, err = lib(), HEADER.enums["MJL_ERR_ARG"]
    d = _data(sys_, Q)
    n = rf.NRAY
    dist = torch.full((NENV, n), SENTINEL, device="cuda")
    p, v = _t(P), _t(V)
    lp, lv = _t(P[0]), _t(V[0])
    ptr = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    XB, SITE = abi.SENSOR_OBJ["xbody"], abi.SENSOR_OBJ["site"]

    def ray(batch=d.handle, nray=n, pnt=ptr(p), vec=ptr(v), flags=1, excl=-1, out=ptr(dist)):
        return L.mjl_ray(batch, None, nray, pnt, vec, flags, excl, C.c_float(0.0), out, None, st)

    def scan(batch=d.handle, objtype=XB, objid=1, align=0, nray=n, pnt=ptr(lp), vec=ptr(lv), flags=1, excl=-1,
             out=ptr(dist)):
        return L.mjl_ray_scan(batch, None, objtype, objid, align, nray, pnt, vec, flags, excl, C.c_float(0.0), out,
                              None, None, st)
    for fn in (ray, scan):
        assert fn() == 0
        for kw, word in (({"batch": None}, b"batch"), ({"out": None}, b"dist"), ({"nray": 0}, b"nray"),
                         ({"nray": 65536}, b"nray"), ({"flags": 2}, b"flags"), ({"flags": -1}, b"flags"),
                         ({"excl": -2}, b"bodyexclude"), ({"excl": m.nbody}, b"bodyexclude")):
            assert fn(**kw) == err and word in L.mjl_last_error(), (fn.__name__, kw, L.mjl_last_error())
    assert ray(pnt=None) == err and b"pnt" in L.mjl_last_error()
    assert ray(vec=None) == err and b"vec" in L.mjl_last_error()
    assert scan(pnt=None) == err and b"lpnt" in L.mjl_last_error()
    assert scan(vec=None) == err and b"lvec" in L.mjl_last_error()
    for kw, word in (({"align": 2}, b"align"), ({"align": -1}, b"align"), ({"objtype": abi.SENSOR_OBJ["joint"]}, b"objtype"),
                     ({"objid": -1}, b"objid"), ({"objid": m.nbody}, b"objid"),
                     ({"objtype": SITE, "objid": m.nsite}, b"objid")):
        assert scan(**kw) == err and word in L.mjl_last_error(), (kw, L.mjl_last_error())
    assert scan(excl=m.nbody - 1, objtype=SITE, objid=m.nsite - 1, align=1) == 0
    with pytest.raises(MjlError, match="align"):
        mjx.ray_scan(sys_, d, "torso", lp, lv, align="roll")
    with pytest.raises(MjlError, match="no body or site"):
        mjx.ray_scan(sys_, d, "nosuchframe", lp, lv)
    with pytest.raises(MjlError, match="self"):
        mjx.ray(sys_, d, p, v, bodyexclude="self")
    torch.cuda.synchronize()
