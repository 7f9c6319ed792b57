"""Geom distances without a GPU: known answers of the float64 reference (tests/distance_ref.py), its closest-segment
search against a dense sampling, the gradient formula of include/mjx355.h against central finite differences, the
degenerate share of every case tests/test_distance_gpu.py compares, the header's declaration and the binding, the
null-batch error, the Python argument errors and the tolerance file."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import mjx_amd
from mjx_amd import abi, mjcf, mjx
from mjx_amd._header import HEADER
from mjx_amd._lib import lib

import distance_ref as df
import rays_ref as rf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model():
    return mjx_amd.load_model("humanoid_mjx")


def _scene(types, pos, z, r, h):
    """A hand-placed scene (no kinematics): what distance_ref.pair reads."""
    z = np.asarray(z, float)
    return {"type": np.array(types), "pos": np.asarray(pos, float), "z": z / np.linalg.norm(z, axis=1, keepdims=True),
            "r": np.asarray(r, float), "h": np.asarray(h, float)}


def _check_pair(sc, a, b, dist, fr=None, to=None, n=None):
    d, f, t, nn = df.pair(sc, a, b)
    assert d == pytest.approx(dist, abs=1e-12)
    np.testing.assert_allclose(t, f + d * nn, atol=1e-12)   # to = from + dist normal, also when dist < 0
    assert np.linalg.norm(nn) == pytest.approx(1.0, abs=1e-12)
    assert abs(df.on_surface(sc, a, f)) < 1e-12 and abs(df.on_surface(sc, b, t)) < 1e-12
    for got, want in ((f, fr), (t, to), (nn, n)):
        if want is not None:
            np.testing.assert_allclose(got, want, atol=1e-12)
    # swapped order: the halves of fromto swap, the normal flips, the distance stays
    d2, f2, t2, n2 = df.pair(sc, b, a)
    assert d2 == pytest.approx(d, abs=1e-15)
    np.testing.assert_allclose(f2, t, atol=1e-15)
    np.testing.assert_allclose(t2, f, atol=1e-15)
    np.testing.assert_allclose(n2, -nn, atol=1e-15)


def test_reference_known_answers(model):
    P, S, K = mjcf.GEOM_PLANE, mjcf.GEOM_SPHERE, mjcf.GEOM_CAPSULE
    ez = [0, 0, 1.0]
    # sphere - sphere: apart, and overlapping (negative)
    sc = _scene([S, S, S], [[0, 0, 0], [1.0, 0, 0], [0.25, 0, 0]], [ez] * 3, [0.2, 0.3, 0.1], [0, 0, 0])
    _check_pair(sc, 0, 1, 0.5, [0.2, 0, 0], [0.7, 0, 0], [1, 0, 0])
    _check_pair(sc, 0, 2, -0.05, [0.2, 0, 0], [0.15, 0, 0], [1, 0, 0])
    # sphere - capsule: beside the cylinder part, and past a cap
    sc = _scene([S, K, S], [[0.5, 0, 0.1], [0, 0, 0], [0, 0, 1.0]], [ez] * 3, [0.1, 0.05, 0.1], [0, 0.3, 0])
    _check_pair(sc, 0, 1, 0.35, [0.4, 0, 0.1], [0.05, 0, 0.1], [-1, 0, 0])
    _check_pair(sc, 2, 1, 0.55, [0, 0, 0.9], [0, 0, 0.35], [0, 0, -1])
    # capsule - capsule: crossed axes (interior of both), and end against side, overlapping
    sc = _scene([K, K, K], [[0, 0, 0], [0, 0, 0.5], [0.6, 0.02, 0]], [[1, 0, 0], [0, 1, 0], [1, 0, 0]], [0.1, 0.1, 0.15],
                [0.4, 0.4, 0.1])
    _check_pair(sc, 0, 1, 0.3, [0, 0, 0.1], [0, 0, 0.4], [0, 0, 1])
    d = np.hypot(0.1, 0.02)
    _check_pair(sc, 0, 2, d - 0.25, n=np.array([0.1, 0.02, 0]) / d)
    assert d - 0.25 < 0
    # plane - sphere: above (exactly z - r), and sunk into the half-space
    sc = _scene([P, S, S], [[0, 0, 0], [0.3, -0.2, 0.7], [1.0, 1.0, 0.05]], [ez] * 3, [0, 0.25, 0.2], [0, 0, 0])
    assert df.pair(sc, 0, 1)[0] == 0.7 - 0.25
    _check_pair(sc, 0, 1, 0.45, [0.3, -0.2, 0], [0.3, -0.2, 0.45], ez)
    _check_pair(sc, 0, 2, -0.15, [1, 1, 0], [1, 1, -0.15], ez)
    # plane - capsule: the nearer end decides (tilted: the -z end; standing on its +z end)
    t = np.array([0.6, 0, 0.8])
    sc = _scene([P, K, K], [[0, 0, 0], [0, 0, 1.0], [2.0, 0, 0.45]], [ez, t, [0, 0, -1.0]], [0, 0.1, 0.05], [0, 0.5, 0.5])
    _check_pair(sc, 0, 1, 1.0 - 0.4 - 0.1, to=np.array([0, 0, 1.0]) - 0.5 * t - [0, 0, 0.1], n=ez)
    _check_pair(sc, 0, 2, -0.1, [2, 0, 0], [2, 0, -0.1], ez)
    # coincident centres: -(r1 + r2) and a finite unit normal (world +z)
    sc = _scene([S, S], [[0.3, 0.2, 0.1]] * 2, [ez] * 2, [0.2, 0.3], [0, 0])
    d, f, t_, n = df.pair(sc, 0, 1)
    assert d == -0.5 and n.tolist() == [0, 0, 1.0]
    with pytest.raises(ValueError):
        df.pair(_scene([P, P], [[0, 0, 0]] * 2, [ez] * 2, [0, 0], [0, 0]), 0, 1)

    # the model: at qpos0 and lifted by 0.5 m every body geom's floor distance is its lowest point's height
    m = model
    for lift in (0.0, 0.5):
        q = m.qpos0.copy()
        q[2] += lift
        sc = df.scene(m, q)
        head = m.names["geom"].index("head")
        assert sc["type"][head] == S and sc["type"][0] == P
        d, ft, n, J, capped = df.geom_distance(m, sc, [0, head], [head, 0])
        assert d[0] == sc["pos"][head][2] - sc["r"][head] and d[1] == d[0]
        np.testing.assert_allclose(ft[0], np.concatenate([ft[1, 3:], ft[1, :3]]), atol=1e-15)
        np.testing.assert_allclose(n, [[0, 0, 1], [0, 0, -1]], atol=1e-15)
        # the floor distance changes one for one with the root's z (dof 2), in either order
        assert J[0, 2] == pytest.approx(1.0, abs=1e-12) and J[1, 2] == pytest.approx(1.0, abs=1e-12)
    # the cap: dist = distmax and zeros
    d, ft, n, J, capped = df.geom_distance(m, sc, [0], [head], distmax=0.3)
    assert capped[0] and d[0] == 0.3 and not ft.any() and not n.any() and not J.any()


def test_closest_segments_against_sampling(model):
    """The analytic closest points are no further apart than any sampled pair, and within the grid's resolution of
    the best one: on random segments and on the model's capsule pairs."""
    rng = np.random.default_rng(0)
    segs = []
    for _ in range(40):
        z = rng.normal(size=(2, 3))
        z /= np.linalg.norm(z, axis=1, keepdims=True)
        segs.append((rng.uniform(-0.5, 0.5, 3), z[0], rng.uniform(0, 0.5), rng.uniform(-0.5, 0.5, 3), z[1], rng.uniform(0, 0.5)))
    z = np.array([0.6, 0.0, 0.8])  # parallel: overlapping and offset along the axis
    segs += [(np.zeros(3), z, 0.3, np.array([0.1, 0.2, 0]), z, 0.2), (np.zeros(3), z, 0.3, 1.5 * z + [0, 0.1, 0], -z, 0.2)]
    sc = df.scene(model, rf.poses(model)[0])
    caps = np.flatnonzero(sc["type"] == mjcf.GEOM_CAPSULE)
    segs += [df._seg(sc, a) + df._seg(sc, b) for a in caps[:6] for b in caps[6:12]]
    for s in segs:
        pa, pb = df.closest_segments(*s)
        d, ds = np.linalg.norm(pb - pa), df.sampled_segment_distance(*s)
        assert d <= ds + 1e-12 and ds - d <= 2 * (s[2] + s[5]) / 400 + 1e-12, (s, d, ds)


@pytest.mark.parametrize("name", mjx_amd.BUILTIN_MODELS)
def test_gradient_formula_against_finite_differences(name):
    """jac = normal' (jacp(to, body2) - jacp(from, body1)) is the derivative of dist along every dof."""
    m = mjx_amd.load_model(name)
    g1, g2 = df.all_pairs(m)
    worst = 0.0
    for q in rf.poses(m):
        sc = df.scene(m, q)
        keep = ~df.degenerate(m, sc, g1, g2)
        J = df.geom_distance(m, sc, g1, g2)[3]
        err = np.abs(J - df.fd_gradient(m, q, g1, g2))[keep].max()
        worst = max(worst, err)
        assert err <= df.FD_TOL, f"{name}: |jac - finite difference| = {err:.3e}"
    print(name, "largest |jac - central difference|:", worst)


@pytest.mark.parametrize("name", mjx_amd.BUILTIN_MODELS)
def test_degenerate_share_of_the_gpu_cases(name):
    m = mjx_amd.load_model(name)
    g1, g2 = df.all_pairs(m)
    assert len(g1) == 190
    ncapped = 0
    for distmax in (np.inf, df.DISTMAX):
        for q in rf.poses(m):
            sc = df.scene(m, q)
            deg = df.degenerate(m, sc, g1, g2, distmax)
            assert deg.mean() <= df.DEGENERATE_CAP, f"{name} distmax {distmax}: {int(deg.sum())} of {len(deg)} pairs"
            if np.isfinite(distmax):
                capped = df.geom_distance(m, sc, g1, g2, distmax, with_jac=False)[4]
                ncapped += int(capped.sum())
                assert 0 < capped.sum() < len(g1)  # both branches are exercised
    print(name, "capped pairs at distmax", df.DISTMAX, ":", ncapped, "of", 3 * len(g1))


def test_header_and_binding():
    protos = {name: (ret, args) for ret, name, args in HEADER.protos}
    assert protos["mjl_geom_distance"] == ("int", ["mjlBatch*", "float*", "int", "int32_t*", "int32_t*", "float", "float*",
                                                   "float*", "float*", "float*", "void*"])
    assert HEADER.enums["MJL_OPT_DISTANCE_CHUNK"] == 8 and abi.OPT_DISTANCE_CHUNK == 8
    assert lib().mjl_geom_distance.argtypes[5] is C.c_float


def test_null_batch_is_an_argument_error():
    L, err = lib(), HEADER.enums["MJL_ERR_ARG"]
    assert L.mjl_geom_distance(None, None, 1, None, None, 1.0, None, None, None, None, None) == err
    assert b"batch" in L.mjl_last_error()


def test_python_argument_errors(model):
    sys_ = mjx.put_model(model)
    ng = model.ngeom
    assert mjx.geom_pairs(sys_, "head", "floor") == ([model.names["geom"].index("head")], [0])
    assert mjx.geom_pairs(sys_, [1, "head"], [0, 2])[0][0] == 1
    for a, b, word in ((ng, 0, "outside"), (-1, 0, "outside"), ("nosuchgeom", 0, "no geom named"), (3, 3, "itself"),
                       ([1, 2], [3], "entries"), ([], [], "pairs")):
        with pytest.raises(ValueError, match=word):
            mjx.geom_pairs(sys_, a, b)
    two = mjcf.compile_xml_string(
        '<mujoco><worldbody><geom name="a" type="plane" size="1 1 1"/><geom name="b" type="plane" size="1 1 1" pos="0 0 -1"/>'
        '<body name="ball" pos="0 0 1"><freejoint/><geom name="s" type="sphere" size="0.1"/></body>'
        '<body name="empty" pos="0 0 2"/>'
        '</worldbody></mujoco>', "two_planes")
    sys2 = mjx.put_model(two)
    with pytest.raises(ValueError, match="both planes"):
        mjx.geom_pairs(sys2, "a", "b")
    with pytest.raises(ValueError, match="no geoms"):
        mjx.body_pairs(sys2, "ball", "empty")
    with pytest.raises(ValueError, match="no body named"):
        mjx.body_pairs(sys2, "ball", "nosuchbody")
    ids1, ids2, index = mjx.body_pairs(sys2, ["world", "ball"], ["ball", "world"])
    assert (ids1, ids2, index) == ([0, 1, 2, 2], [2, 2, 0, 1], [[0, 1], [2, 3]])
    g1, g2 = mjx.collision_pairs(sys_)
    assert g1 == model.arrays["pair_geom1"].tolist() and g2 == model.arrays["pair_geom2"].tolist() and len(g1) == model.npair
    assert mjx.geom_pairs(sys_, g1, g2) == (g1, g2)  # every collision pair is a valid distance pair


def test_tolerance_file():
    """profiles/distance/tolerances.json: each bound is four times the measured maximum, rounded up to one
    significant digit; the measured dist error is at fp32 resolution at metre scale."""
    t = df.load_tolerances()

    def up1(x):
        e = math.floor(math.log10(x))
        return math.ceil(x / 10 ** e - 1e-9) * 10 ** e
    for key, what in (("dist_tol", "dist"), ("point_tol", "point"), ("normal_tol", "normal"), ("jac_tol", "jac")):
        worst = max(v[what] for v in t["measured_max"].values())
        assert t[key] == pytest.approx(up1(4 * worst), rel=1e-9), key
    assert 0 < max(v["dist"] for v in t["measured_max"].values()) <= 1e-4
