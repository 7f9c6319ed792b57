"""Ray casts without a GPU: known answers of the float64 reference (tests/rays_ref.py), the marginal share of every
case tests/test_rays_gpu.py compares, the pattern helpers, the header's declarations and the binding, and the
null-batch errors."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import mjx_amd
from mjx_amd import abi, mjcf, rays
from mjx_amd._header import HEADER
from mjx_amd._lib import lib

import render_ref as rr
import rays_ref as rf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model():
    return mjx_amd.load_model("humanoid_mjx")


def test_reference_known_answers(model):
    m = model
    q = m.qpos0.copy()
    sc = rr.scene(m, q)
    head = m.names["geom"].index("head")
    assert sc["type"][head] == mjcf.GEOM_SPHERE and sc["type"][0] == mjcf.GEOM_PLANE
    c, r = sc["pos"][head], sc["r"][head]
    down, up = np.array([0.0, 0.0, -1.0]), np.array([0.0, 0.0, 1.0])
    # down onto the floor from height h, beside the robot
    d, g = rf.cast(m, sc, [[2.0, 1.0, 0.7]], [down])
    assert g[0] == 0 and d[0] == pytest.approx(0.7, abs=1e-12)
    # through the head sphere from above: the analytic entry; from its centre: the exit; a non-unit vec scales t
    d, g = rf.cast(m, sc, [c + [0.01, 0, 1.0]], [down])
    assert g[0] == head and d[0] == pytest.approx(1.0 - np.sqrt(r * r - 1e-4), abs=1e-12)
    d, g = rf.cast(m, sc, [c], [[1.0, 0, 0]], bodyexclude=-1)
    assert g[0] == head and d[0] == pytest.approx(r, abs=1e-12)
    d, g = rf.cast(m, sc, [c + [0.01, 0, 1.0]], [4 * down])
    assert g[0] == head and d[0] == pytest.approx((1.0 - np.sqrt(r * r - 1e-4)) / 4, abs=1e-12)
    # up from above the head misses; the floor is left out without flg_static; cutoff bounds t
    assert tuple(x[0] for x in rf.cast(m, sc, [c + [0, 0, 1.0]], [up])) == (-1.0, -1)
    assert tuple(x[0] for x in rf.cast(m, sc, [[2.0, 1.0, 0.7]], [down], flg_static=False)) == (-1.0, -1)
    assert tuple(x[0] for x in rf.cast(m, sc, [[2.0, 1.0, 0.7]], [down], cutoff=0.6)) == (-1.0, -1)
    assert rf.cast(m, sc, [[2.0, 1.0, 0.7]], [down], cutoff=0.8)[1][0] == 0
    # excluding the head's body reports what lies behind it (the torso side), further away
    hb = int(m.arrays["geom_bodyid"][head])
    d2, g2 = rf.cast(m, sc, [c + [0.01, 0, 1.0]], [down], bodyexclude=hb)
    assert g2[0] not in (head, -1) and d2[0] > 1.0
    # a rangefinder on a foot site looking down through the floor side (-z of an upright foot, floor excluded) sees
    # nothing; looking away from everything likewise
    kind, s, body = rf.frame_ids(m, "site_foot_right")
    p, v = rf.scan_rays(m, sc["kin"], kind, s, "pose", [[0, 0, 0]], [[0, 0, -1.0]])
    assert tuple(x[0] for x in rf.cast(m, sc, p, v, flg_static=False, bodyexclude=body)) == (-1.0, -1)
    hp = rf.hitpos(np.array([[2.0, 1.0, 0.7], [0, 0, 5.0]]), np.array([down, up]), np.array([0.7, -1.0]))
    np.testing.assert_allclose(hp, [[2.0, 1.0, 0.0], [0, 0, 5.0]], atol=1e-15)


def test_scan_alignments(model):
    m = model
    q = rf.poses(m, seed=6, pitch=0.5)[1]
    kin = rr.scene(m, q)["kin"]
    tb = m.names["body"].index("torso")
    lp, lv = rays.grid_pattern(5, 7, 0.15, 0.1, 0.5)
    p, v = rf.scan_rays(m, kin, "xbody", tb, "yaw", lp, lv)
    np.testing.assert_allclose(v, np.tile([0, 0, -1.0], (35, 1)), atol=1e-15)  # level: straight down
    np.testing.assert_allclose(p[:, 2], kin["xpos"][tb][2] + 0.5, atol=1e-12)
    yaw = 0.7 * 1 - 0.5  # poses(): env 1
    np.testing.assert_allclose(p[-1] - p[0], [np.cos(yaw) * 0.6 - np.sin(yaw) * 0.6, np.sin(yaw) * 0.6 + np.cos(yaw) * 0.6, 0],
                               atol=1e-6)
    pp, vp = rf.scan_rays(m, kin, "xbody", tb, "pose", lp, lv)
    np.testing.assert_allclose(vp, np.tile(-kin["xmat"][tb][:, 2], (35, 1)), atol=1e-12)
    assert abs(vp[0, 2] + np.cos(0.5)) < 1e-6
    R, o = rf.frame(m, kin, "site", 0)
    b = int(m.arrays["site_bodyid"][0])
    np.testing.assert_allclose(o, kin["xpos"][b] + kin["xmat"][b] @ m.arrays["site_pos"][0], atol=1e-15)


@pytest.mark.parametrize("name", mjx_amd.BUILTIN_MODELS)
def test_marginal_share_of_the_gpu_cases(name):
    m = mjx_amd.load_model(name)
    tol = rf.load_tolerances()["dist_tol"]
    worst = 0.0
    for label, q, pnt, vec, kw in rf.cases(m):
        marg = rf.marginal(m, rr.scene(m, q), pnt, vec, tol, **kw)
        worst = max(worst, marg.mean())
        assert marg.mean() <= rf.MARGINAL_CAP, f"{name} {label}: {int(marg.sum())} of {len(marg)} rays are marginal"
    print(name, "largest marginal share:", worst)


def test_patterns():
    lp, lv = rays.grid_pattern(5, 7, 0.15, 0.1, 0.5)
    assert lp.shape == lv.shape == (35, 3) and lp.dtype == lv.dtype == np.float32
    assert (lv == [0, 0, -1]).all() and (lp[:, 2] == 0.5).all()
    np.testing.assert_allclose(lp[:, :2].mean(0), 0, atol=1e-7)
    np.testing.assert_allclose(lp[7] - lp[0], [0.15, 0, 0], atol=1e-7)  # ray i * ny + j
    np.testing.assert_allclose(lp[1] - lp[0], [0, 0.1, 0], atol=1e-7)
    np.testing.assert_allclose(lp[-1, :2], [0.3, 0.3], atol=1e-7)
    lp, lv = rays.fan_pattern(9, 180.0)
    assert lp.shape == lv.shape == (9, 3) and not lp.any()
    np.testing.assert_allclose(np.linalg.norm(lv, axis=1), 1, atol=1e-6)
    np.testing.assert_allclose(lv[[0, 4, 8]], [[0, -1, 0], [1, 0, 0], [0, 1, 0]], atol=1e-6)
    lp, lv = rays.fan_pattern(4, 360.0, elevation_deg=-30.0)
    np.testing.assert_allclose(lv[:, 2], -0.5, atol=1e-6)
    np.testing.assert_allclose(lv[:, :2] / np.cos(np.deg2rad(30)), [[-1, 0], [0, -1], [1, 0], [0, 1]], atol=1e-6)
    assert rays.fan_pattern(1, 90.0)[1].tolist() == [[1.0, 0.0, 0.0]]
    with pytest.raises(ValueError):
        rays.grid_pattern(0, 3, 0.1, 0.1, 1.0)


def test_header_and_binding():
    protos = {name: (ret, args) for ret, name, args in HEADER.protos}
    assert protos["mjl_ray"] == ("int", ["mjlBatch*", "float*", "int", "float*", "float*", "int", "int", "float", "float*",
                                         "int32_t*", "void*"])
    assert protos["mjl_ray_scan"] == ("int", ["mjlBatch*", "float*", "int", "int", "int", "int", "float*", "float*", "int",
                                              "int", "float", "float*", "int32_t*", "float*", "void*"])
    E = HEADER.enums
    assert (E["MJL_RAY_STATIC"], E["MJL_SCAN_POSE"], E["MJL_SCAN_YAW"]) == (1, 0, 1)
    assert abi.RAY_STATIC == 1 and abi.SCAN_ALIGN == {"pose": 0, "yaw": 1}
    L = lib()
    assert L.mjl_ray.argtypes[7] is C.c_float and L.mjl_ray_scan.argtypes[10] is C.c_float


def test_null_batch_is_an_argument_error():
    L, err = lib(), HEADER.enums["MJL_ERR_ARG"]
    assert L.mjl_ray(None, None, 1, None, None, 0, -1, 0.0, None, None, None) == err
    assert b"batch" in L.mjl_last_error()
    assert L.mjl_ray_scan(None, None, 0, 0, 0, 1, None, None, 0, -1, 0.0, None, None, None, None) == err
    assert b"batch" in L.mjl_last_error()


def test_tolerance_file():
    """profiles/rays/tolerances.json: the bounds are four times the measured maxima, rounded up to one significant
    digit, and no more than 1e-3 m."""
    with open(os.path.join(ROOT, "profiles", "rays", "tolerances.json")) as f:
        t = json.load(f)

    def up1(x):
        e = np.floor(np.log10(x))
        return float(np.ceil(x / 10 ** e - 1e-9) * 10 ** e)
    md = max(v["dist"] for v in t["measured_max"].values())
    mh = max(v["hitpos"] for v in t["measured_max"].values())
    assert t["dist_tol"] == pytest.approx(up1(4 * md), rel=1e-9) and t["hitpos_tol"] == pytest.approx(up1(4 * mh), rel=1e-9)
    assert 0 < t["dist_tol"] <= 1e-3 and 0 < t["hitpos_tol"] <= 1e-3
