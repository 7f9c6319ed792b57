"""Geom distances (mjl_geom_distance, mjx.geom_distance / body_distance / collision_pairs, HumanoidEnv.geom_distance)
on the GPU against the float64 reference tests/distance_ref.py.

Both humanoids, 3 envs with different poses (rays_ref.poses) written with d.set("qpos") and no forward call: the
launch does its own kinematics. All 190 geom pairs, uncapped and capped at 0.3 m.

dist is compared on every pair but those within 1e-4 m of the cap; fromto, normal and jac on the non-degenerate
pairs (distance_ref.degenerate; tests/test_distance.py asserts on the CPU that they are at most 5 % of every case
here); degenerate pairs are checked for the properties any valid answer has. The tolerances are
profiles/distance/tolerances.json: four times the largest error tools/distance_tolerances.py measured with this
file's `measure` on these cases, rounded up to one significant digit."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest
import torch

import mjx_amd
from mjx_amd import abi, mjcf, mjx
from mjx_amd._header import HEADER
from mjx_amd._lib import lib
from mjx_amd.config import reference_ppo_config
from mjx_amd.envs import HumanoidEnv, resolve_ids

import distance_ref as df
import generic_models as gm
import rays_ref as rf

pytestmark = pytest.mark.gpu

SENTINEL = -77.25
NENV = df.NENV
KEYS = ("dist", "point", "normal", "jac")


def _data(sys_, Q):
    d = mjx.make_data(sys_, Q.shape[0])
    d.set("qpos", torch.tensor(Q, dtype=torch.float32))  # and no forward
    return d


def _np(t):
    return None if t is None else t.cpu().numpy()


def _tol():
    t = df.load_tolerances()
    return {k: t[k + "_tol"] for k in KEYS}


_KEY = {}


@functools.lru_cache(maxsize=None)
def _model(name):
    m = mjx_amd.load_model(name)
    _KEY[id(m)] = name  # the built-in name `reference` is keyed by (m.name is the MJCF's own)
    return m


@functools.lru_cache(maxsize=None)
def reference(name, e, distmax):
    """The reference of env e of rays_ref.poses over all pairs, computed once and shared: (scene, dist, fromto, normal,
    jac, capped, degenerate, near the cap)."""
    m = _model(name)
    g1, g2 = df.all_pairs(m)
    sc = df.scene(m, rf.poses(m)[e])
    out = (sc,) + df.geom_distance(m, sc, g1, g2, distmax) + (df.degenerate(m, sc, g1, g2, distmax),
                                                             df.near_cap(m, sc, g1, g2, distmax))
    for x in out[1:]:
        x.setflags(write=False)
    return out


def compare(m, label, ref, g1, g2, distmax, got, tol, errs=None):
    """One env's rows against the reference. tol: {dist, point, normal, jac} bounds, None: nothing bounded
    (measurement); errs collects the four maxima."""
    sc, dref, ftref, nref, jref, capped, deg, near = ref
    dist, fromto, normal, jac = (np.asarray(x, np.float64) for x in got)
    cmp_d = ~near
    live = ~capped & ~near
    good = live & ~deg
    e = {"dist": np.abs(dist - dref)[cmp_d].max(), "point": np.abs(fromto - ftref)[good].max(),
         "normal": np.abs(normal - nref)[good].max(), "jac": np.abs(jac - jref)[good].max()}
    print(f"{m.name} {label}: {int(deg.sum())} degenerate, {int(capped.sum())} capped, {int(near.sum())} near the cap of "
          f"{len(deg)}; max errors " + ", ".join(f"{k} {v:.3e}" for k, v in e.items()))
    if errs is not None:
        errs.append(e)
    # capped pairs: dist == distmax bit for bit, everything else zero
    c = capped & ~near
    if c.any():
        assert (np.asarray(got[0])[c] == np.float32(distmax)).all(), label
        assert not fromto[c].any() and not normal[c].any() and not jac[c].any(), label
    assert np.isfinite(dist).all() and np.isfinite(jac).all()
    if tol is None:
        return e
    for k in KEYS:
        assert e[k] <= tol[k], f"{label}: {k} error {e[k]:.3e} > {tol[k]:.1e}"
    # degenerate pairs: another pair of witness points may be the right answer; what every answer satisfies
    for k in np.flatnonzero(live & deg):
        fr, to, n = fromto[k, :3], fromto[k, 3:], normal[k]
        assert abs(dist[k] - dref[k]) <= tol["dist"]
        assert abs(df.on_surface(sc, g1[k], fr)) <= tol["point"] and abs(df.on_surface(sc, g2[k], to)) <= tol["point"], (label, k)
        assert abs(np.linalg.norm(to - fr) - abs(dist[k])) <= tol["point"] + tol["dist"], (label, k)
        assert abs(np.linalg.norm(n) - 1.0) <= tol["normal"], (label, k)
    return e


@pytest.fixture(scope="module", params=mjx_amd.BUILTIN_MODELS)
def setup(request):
    m = _model(request.param)
    g1, g2 = df.all_pairs(m)
    return m, mjx.put_model(m), rf.poses(m), g1, g2


def run_all_pairs(m, sys_, Q, g1, g2, tol, errs=None):
    d = _data(sys_, Q)
    res = {}
    for distmax in (np.inf, df.DISTMAX):
        r = mjx.geom_distance(sys_, d, g1, g2, distmax=distmax, with_jac=True)
        got = [_np(x) for x in r]
        for e in range(NENV):
            compare(m, f"distmax {distmax} env {e}", reference(_KEY[id(m)], e, distmax), g1, g2, distmax, [x[e] for x in got], tol, errs)
        res[distmax] = got
    return res


def test_all_pairs_against_the_reference(setup):
    m, sys_, Q, g1, g2 = setup
    res = run_all_pairs(m, sys_, Q, g1, g2, _tol())
    dist, fromto, normal, jac = res[np.inf]
    assert (dist < 0).any() and (dist > df.DISTMAX).any()  # overlapping neighbours and distant limbs both occur
    # to = from + dist * normal on every pair, also the overlapping ones
    np.testing.assert_allclose(fromto[..., 3:], fromto[..., :3] + dist[..., None] * normal, atol=2e-6)
    # swapped order: the halves swap, the normal flips, the distance and its gradient stay
    d = _data(sys_, Q)
    sw = [_np(x) for x in mjx.geom_distance(sys_, d, g2, g1, with_jac=True)]
    keep = np.array([~reference(_KEY[id(m)], e, np.inf)[6] for e in range(NENV)])
    t = _tol()
    assert np.abs(sw[0] - dist).max() <= 2 * t["dist"]
    assert np.abs(sw[1][..., :3] - fromto[..., 3:])[keep].max() <= 2 * t["point"]
    assert np.abs(sw[2] + normal)[keep].max() <= 2 * t["normal"]
    assert np.abs(sw[3] - jac)[keep].max() <= 2 * t["jac"]
    # names and scalars; no jac unless asked for
    head = m.names["geom"].index("head")
    r = mjx.geom_distance(sys_, d, 0, "head")
    k = g2.index(head)  # pair (0, head)
    assert r.jac is None and tuple(r.dist.shape) == (NENV, 1) and np.array_equal(_np(r.dist)[:, 0], dist[:, k])


def test_chunking_is_bit_identical(setup):
    m, sys_, Q, g1, g2 = setup
    d = _data(sys_, Q)
    full = [_np(x) for x in mjx.geom_distance(sys_, d, g1, g2, distmax=df.DISTMAX, with_jac=True)]
    for chunk in (0, 100, 65535, 3):  # the library's choice, a ragged second tile, kinematics once per env, tiny
        d.set_option(abi.OPT_DISTANCE_CHUNK, chunk)
        for n in (1, 65, len(g1)):  # one pair, more than one wavefront's stride, all of them
            got = mjx.geom_distance(sys_, d, g1[:n], g2[:n], distmax=df.DISTMAX, with_jac=True)
            for a, b in zip(got, full):  # a shorter list gives the leading rows of the full one
                np.testing.assert_array_equal(_np(a), b[:, :n], err_msg=f"chunk {chunk}, {n} pairs")
    with pytest.raises(mjx.MjlError):
        d.set_option(abi.OPT_DISTANCE_CHUNK, -1)


def test_generic_model_at_the_capacities():
    """generic_models.full(): nv = 32 fills every dof lane, 32 geoms every record slot; 496 pairs. dist against the
    reference within 1e-4 m (fp32 resolution at metre scale with two digits of margin: the bound past which an
    error is a bug, not rounding), rows bit-identical across chunk settings. jac on the non-degenerate pairs whose
    axis points are at least 0.05 m apart: a witness point within 2e-6 m turns the normal by at most 2e-6 / 0.05 =
    4e-5, the columns (lever arms below 1 m) by about as much; 1e-3 leaves a digit of margin."""
    from test_dyn import generic_states
    m = gm.full()
    sys_ = mjx.put_model(m)
    Q = np.array([s[0] for s in generic_states(m, 2)])
    g1, g2 = df.all_pairs(m)
    assert (m.nv, m.ngeom, len(g1)) == (32, 32, 496)
    d = _data(sys_, Q)
    got = [_np(x) for x in mjx.geom_distance(sys_, d, g1, g2, with_jac=True)]
    d.set_option(abi.OPT_DISTANCE_CHUNK, 50)
    for a, b in zip(got, mjx.geom_distance(sys_, d, g1, g2, with_jac=True)):
        np.testing.assert_array_equal(a, _np(b))
    for e in range(2):
        sc = df.scene(m, Q[e])
        dref, ftref, nref, jref, _ = df.geom_distance(m, sc, g1, g2)
        axis = dref + sc["r"][g1] + sc["r"][g2]
        keep = ~df.degenerate(m, sc, g1, g2) & ((axis >= 0.05) | (sc["type"][g1] == mjcf.GEOM_PLANE))
        assert keep.mean() > 0.5
        assert np.abs(got[0][e] - dref).max() <= 1e-4
        assert np.abs(got[3][e] - jref)[keep].max() <= 1e-3


def test_mask_and_optional_outputs(setup):
    m, sys_, Q, g1, g2 = setup
    d = _data(sys_, Q)
    n, nv = len(g1), m.nv
    full = mjx.geom_distance(sys_, d, g1, g2, distmax=df.DISTMAX, with_jac=True)
    shapes = ((NENV, n), (NENV, n, 6), (NENV, n, 3), (NENV, n, nv))
    mask = torch.tensor([1.0, 0.0, 1.0])
    out = tuple(torch.full(s, SENTINEL, device="cuda") for s in shapes)
    r = mjx.geom_distance(sys_, d, g1, g2, distmax=df.DISTMAX, mask=mask, out=out)
    for got, buf, want in zip(r, out, full):
        assert got is buf                                # written in place
        assert (buf[1] == SENTINEL).all()                # the masked env keeps every row
        assert torch.equal(buf[0], want[0]) and torch.equal(buf[2], want[2])
    fresh = mjx.geom_distance(sys_, d, g1, g2, distmax=df.DISTMAX, mask=mask, with_jac=True)
    assert all(not t[1].any() for t in fresh)            # fresh tensors are zeros under a mask
    # every None combination of the optional outputs: the others identical, the skipped ones untouched
    for bits in range(8):
        out = [torch.full(s, SENTINEL, device="cuda") for s in shapes]
        arg = [out[0]] + [out[k + 1] if bits >> k & 1 else None for k in range(3)]
        r = mjx.geom_distance(sys_, d, g1, g2, distmax=df.DISTMAX, out=tuple(arg))
        for k in range(4):
            if arg[k] is None:
                assert r[k] is None
            else:
                assert r[k] is out[k] and torch.equal(out[k], full[k]), (bits, k)
    with pytest.raises(mjx.MjlError, match="dist"):
        mjx.geom_distance(sys_, d, g1, g2, out=(None, out[1], None, None))
    with pytest.raises(mjx.MjlError, match="shape"):
        mjx.geom_distance(sys_, d, g1, g2, out=(out[0][:, :5].contiguous(),))
    with pytest.raises(ValueError, match="distmax"):
        mjx.geom_distance(sys_, d, g1, g2, distmax=0.0)


def test_device_side_guard_and_argument_errors(setup):
    """Ids the host cannot see (device memory) are checked in the kernel before anything is read through them: an
    out-of-range, equal or plane - plane pair gets NaN and zeros, its neighbours their values."""
    m, sys_, Q, g1, g2 = setup
    L, err = lib(), HEADER.enums["MJL_ERR_ARG"]
    d = _data(sys_, Q)
    ng, nv = m.ngeom, m.nv
    a = [0, ng, 1, 2, 3, 1 << 30, 4, 0, 5]
    b = [5, 1, 2, -5, 3, 0, -(1 << 31), 0, 0]
    bad = np.array([False, True, False, True, True, True, True, True, False])
    n = len(a)
    ta, tb = (torch.tensor(x, dtype=torch.int32, device="cuda") for x in (a, b))
    out = [torch.full(s, SENTINEL, device="cuda") for s in ((NENV, n), (NENV, n, 6), (NENV, n, 3), (NENV, n, nv))]
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(batch=d.handle, npair=n, p1=ta, p2=tb, distmax=float("inf"), o=out):
        return L.mjl_geom_distance(batch, None, npair, ptr(p1), ptr(p2), C.c_float(distmax), *(ptr(t) for t in o), st)
    assert call() == 0
    torch.cuda.synchronize()
    dist, fromto, normal, jac = (_np(t) for t in out)
    assert np.isnan(dist[:, bad]).all()
    assert not fromto[:, bad].any() and not normal[:, bad].any() and not jac[:, bad].any()
    ok = np.flatnonzero(~bad)
    want = mjx.geom_distance(sys_, d, [a[k] for k in ok], [b[k] for k in ok], with_jac=True)
    for got, w in zip((dist, fromto, normal, jac), want):
        np.testing.assert_array_equal(got[:, ok], _np(w))
    for kw, word in (({"batch": None}, b"batch"), ({"o": [None] + out[1:]}, b"dist"), ({"p1": None}, b"geom1"),
                     ({"p2": None}, b"geom2"), ({"npair": 0}, b"npair"), ({"npair": -3}, b"npair"),
                     ({"distmax": 0.0}, b"distmax"), ({"distmax": -1.0}, b"distmax"), ({"distmax": float("nan")}, b"distmax")):
        assert call(**kw) == err and word in L.mjl_last_error(), (kw, L.mjl_last_error())
    torch.cuda.synchronize()


def test_coincident_centres():
    """Two spheres on bodies of their own at the same point: -(r1 + r2) exactly and a finite unit normal (world +z,
    include/mjx355.h), in either order; a sphere at a capsule's centre likewise."""
    m = mjcf.compile_xml_string(
        '<mujoco><worldbody><geom name="floor" type="plane" size="1 1 1"/>'
        '<body name="a" pos="0.3 -0.2 1"><freejoint/><geom name="sa" type="sphere" size="0.1"/></body>'
        '<body name="b" pos="0.3 -0.2 1"><freejoint/><geom name="sb" type="sphere" size="0.15"/></body>'
        '<body name="c" pos="0.3 -0.2 1"><freejoint/><geom name="cc" type="capsule" size="0.05 0.2"/></body>'
        '</worldbody></mujoco>', "coincident")
    sys_ = mjx.put_model(m)
    d = _data(sys_, np.tile(m.qpos0, (2, 1)))
    r = mjx.geom_distance(sys_, d, ["sa", "sb", "sa"], ["sb", "sa", "cc"], with_jac=True)
    dist, fromto, normal, jac = (_np(x) for x in r)
    ra, rb, rc = np.float32(0.1), np.float32(0.15), np.float32(0.05)
    assert (dist[:, 0] == -(ra + rb)).all() and (dist[:, 1] == -(rb + ra)).all() and (dist[:, 2] == -(ra + rc)).all()
    assert (normal == np.float32([0, 0, 1])).all() and np.isfinite(fromto).all() and np.isfinite(jac).all()
    np.testing.assert_allclose(fromto[..., 3:], fromto[..., :3] + dist[..., None] * normal, atol=1e-6)


def test_body_distance_and_collision_pairs(setup):
    m, sys_, Q, g1, g2 = setup
    d = _data(sys_, Q)
    tol = _tol()
    nb = m.nbody
    b1, b2 = [1, nb - 1, 0, 2, nb - 2], [0, 0, nb // 2, nb - 1, nb - 1]
    pair_index = {p: k for k, p in enumerate(zip(g1, g2))}
    for distmax in (np.inf, df.DISTMAX):
        r = mjx.body_distance(sys_, d, b1, b2, distmax=distmax, with_jac=True)
        dist, ga, gb = _np(r.dist), _np(r.geom1), _np(r.geom2)
        gids = m.arrays["geom_bodyid"]
        ids1, ids2, _ = mjx.body_pairs(sys_, b1, b2)
        rows = mjx.geom_distance(sys_, d, ids1, ids2, distmax=distmax, with_jac=True)
        plist = list(zip(ids1, ids2))
        for e in range(NENV):
            sc = reference(_KEY[id(m)], e, distmax)[0]
            for k in range(len(b1)):
                dref, ra, rb = df.body_distance(m, sc, b1[k], b2[k], distmax)
                assert abs(dist[e, k] - dref) <= tol["dist"], (e, k)
                a, b = int(ga[e, k]), int(gb[e, k])
                assert gids[a] == b1[k] and gids[b] == b2[k]
                # the reported pair is the nearest one (or within rounding of it)
                assert min(df.pair(sc, a, b)[0], distmax) <= dref + 2 * tol["dist"]
                if dref < distmax - 1e-4 and all(abs(min(df.pair(sc, int(x), int(y))[0], distmax) - dref) > 4 * tol["dist"]
                                                 for x in np.flatnonzero(gids == b1[k]) for y in np.flatnonzero(gids == b2[k])
                                                 if (x, y) != (ra, rb)):
                    assert (a, b) == (ra, rb)  # a clear winner is reported exactly
                # and its rows are that pair's geom_distance rows
                j = plist.index((a, b))
                for got, row in zip((r.fromto, r.normal, r.jac), (rows.fromto, rows.normal, rows.jac)):
                    assert torch.equal(got[e, k], row[e, j])
    # collision_pairs: the model's pair arrays; their clearances are rows of the all-pairs call
    c1, c2 = mjx.collision_pairs(sys_)
    assert c1 == m.arrays["pair_geom1"].tolist() and c2 == m.arrays["pair_geom2"].tolist()
    clear = _np(mjx.geom_distance(sys_, d, c1, c2, distmax=df.DISTMAX).dist)
    allp = _np(mjx.geom_distance(sys_, d, g1, g2, distmax=df.DISTMAX).dist)
    idx = [pair_index[(min(a, b), max(a, b))] for a, b in zip(c1, c2)]
    same = np.array([a < b for a, b in zip(c1, c2)])
    np.testing.assert_array_equal(clear[:, same], allp[:, idx][:, same])
    np.testing.assert_allclose(clear, allp[:, idx], atol=2 * tol["dist"])


def run_capture(m, sys_, g1, g2, tol, errs=None):
    """HumanoidEnv.geom_distance captured behind an env step; returns what the rate check needs."""
    cfg = resolve_ids(m, dataclasses.replace(reference_ppo_config().env_config, max_episode_steps=1000))
    Q1, Q2 = rf.poses(m, seed=6), rf.poses(m)
    rng = np.random.default_rng(4)
    V = np.float32(rng.uniform(-0.5, 0.5, (NENV, m.nv)))
    env = HumanoidEnv(sys_, cfg, NENV, seed=3)
    qbuf = torch.tensor(Q1, dtype=torch.float32, device="cuda")
    vbuf = torch.tensor(V, device="cuda")
    act = torch.zeros((NENV, m.nu), device="cuda")
    env.data.set("qpos", qbuf)
    env.data.set("qvel", vbuf)
    env.step(act, auto_reset=False)
    r0 = env.geom_distance(g1, g2, with_jac=True)  # eager: allocates the buffers, warms the kernel up
    torch.cuda.synchronize()
    eager = _np(r0.dist).copy()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.data.set("qpos", qbuf)
        env.data.set("qvel", vbuf)
        env.step(act, auto_reset=False, counter=1)
        r = env.geom_distance(g1, g2, with_jac=True)
    assert all(a is b for a, b in zip(r, r0))  # the preallocated tensors again
    qbuf.copy_(torch.tensor(Q2, dtype=torch.float32))
    # the state before the step, eagerly: dist and jac at (Q2, V)
    env.data.set("qpos", qbuf)
    before = [_np(x) for x in mjx.geom_distance(sys_, env.data, g1, g2, with_jac=True)]
    g.replay()
    torch.cuda.synchronize()
    after = [_np(x).copy() for x in r]
    assert np.abs(after[0] - eager).max() > 1e-2  # the replay saw the new state
    again = mjx.geom_distance(sys_, env.data, g1, g2, with_jac=True)  # the eager call on the post-step state
    for a, b in zip(after, again):
        np.testing.assert_array_equal(a, _np(b))
    q1, v1 = _np(env.data.get("qpos")).astype(np.float64), _np(env.data.get("qvel")).astype(np.float64)
    return Q2, q1, v1, before, after


def test_captured_with_the_env_step(setup):
    """The replay equals the eager call bit for bit, and jac qvel is the rate of dist: across the captured step,
    (dist_after - dist_before) / dt against the trapezoid (jac_before + jac_after) / 2 . qvel_after (qpos moves along
    the new qvel). The float64 reference gives the same two quantities at the same two states; the kernel's rate
    differs from the reference's by at most 2 dist_tol / dt and its trapezoid by at most jac_tol |qvel|_1, so the
    kernel's mismatch is at most the reference's own (the trapezoid's truncation) plus those two."""
    m, sys_, Q, g1, g2 = setup
    tol = _tol()
    q0, q1, v1, before, after = run_capture(m, sys_, g1, g2, tol)
    dt = float(m.timestep)
    trunc_all = []
    for e in range(NENV):
        s0, s1 = df.scene(m, q0[e]), df.scene(m, q1[e])
        keep = ~df.degenerate(m, s0, g1, g2) & ~df.degenerate(m, s1, g1, g2)
        d0, _, _, j0, _ = df.geom_distance(m, s0, g1, g2)
        d1, _, _, j1, _ = df.geom_distance(m, s1, g1, g2)
        trunc = np.abs((d1 - d0) / dt - 0.5 * (j0 + j1) @ v1[e])
        rate = (after[0][e].astype(np.float64) - before[0][e]) / dt
        trap = 0.5 * (after[3][e].astype(np.float64) + before[3][e]) @ v1[e]
        bound = trunc + 2 * tol["dist"] / dt + tol["jac"] * np.abs(v1[e]).sum()
        worst = np.abs(rate - trap)[keep] - bound[keep]
        print(f"{m.name} env {e}: max |rate - trapezoid| {np.abs(rate - trap)[keep].max():.3e}, median reference "
              f"truncation {np.median(trunc[keep]):.3e}, rounding allowance {2 * tol['dist'] / dt:.3e}")
        assert worst.max() <= 0.0, f"env {e}: pair {int(np.argmax(worst))} misses its bound by {worst.max():.3e}"
        trunc_all.append(trunc[keep])
        assert np.abs((d1 - d0) / dt)[keep].max() > 0.05  # the geoms do move
    assert np.median(np.concatenate(trunc_all)) < 1e-3  # the check is sharp on most pairs


def measure():
    """{model: {dist, point, normal, jac}}: the largest errors of the built kernel against the float64 reference over
    the cases of test_all_pairs_against_the_reference (tools/distance_tolerances.py)."""
    out = {}
    for name in mjx_amd.BUILTIN_MODELS:
        m = _model(name)
        g1, g2 = df.all_pairs(m)
        errs = []
        run_all_pairs(m, mjx.put_model(m), rf.poses(m), g1, g2, None, errs)
        out[name] = {k: max(e[k] for e in errs) for k in KEYS}
    return out
