"""Whole-body inverse kinematics (mjl_ik_wb / mjx.ik_wb), the part that needs no GPU: tests/ik_wb_ref.py is
ik_ref.solve when nothing is added, its CoM and clearance rows are the derivatives of its own subtree_com and dist,
it reaches a CoM target and separates overlapping geoms, and the declaration, its host-side refusals and the Python
surface.

The problems (shared with tests/test_ik_wb_gpu.py) come from tests/test_ik.py problem(): its first three envs, with
  com        the target of the subtree's centre of mass = the one at qpos* (reachable), roots 0 and SUBTREE[name]
  overlap    a start pose in which geoms overlap, made by ik_ref itself: the body TIP[name] brought to the origin of
             the body ONTO[name] (plus 2 cm, so that no two axis points coincide), and for the floor the root lowered
             until the pair's capsule is 2 cm into it. generic_models.full()'s hinges have ranges of about +-25
             degrees, inside which no two separable links of it can be made to overlap, so its overlap poses are
             built, and its overlap cases solved, with the limits off (OVERLAP[name])
  pairs      picked from the model's own collision pairs by their reference distance at the start poses."""
import functools

import numpy as np
import pytest

import mjx_amd
from mjx_amd import mjcf, mjx
from mjx_amd._header import HEADER
from mjx_amd._lib import lib

import distance_ref as dref
import ik_ref as ik
import ik_wb_ref as wb
from test_ik import DAMPING, ITERATIONS, problem

MODELS = list(mjx_amd.BUILTIN_MODELS) + ["full"]
NDISTINCT = 3                 # distinct envs; the GPU tests tile them to 3 and 65
# overlap poses: (TIP body, ONTO body, limits) per model
OVERLAP = {"humanoid_mjx": ("hand_left", "thigh_left", True), "humanoid": ("hand_left", "thigh_left", True),
           "full": ("l0_5", "l1_2", False)}
SUBTREE = {"humanoid_mjx": "thigh_right", "humanoid": "upper_arm_left", "full": 8}
CLEAR_MIN = 0.005             # m, the clearance asked of an overlapping pair
CLEAR_TOL = 1e-5              # m: ten float32 kinematics errors (1e-6 at this scale); the damped Gauss-Newton step leaves
                              # damping / (damping + |J|^2) ~ 1e-4 of the residual per iteration, nothing after ten
MARGIN = 1e-3                 # m: |dist - clear_min| every parity case keeps at every iterate
COM_TOL = 1e-5                # m


# tests/test_distance.py's two-plane model: the only way to a plane - plane pair of two different geoms
TWO_PLANES = ('<mujoco><worldbody><geom name="a" type="plane" size="1 1 1"/><geom name="b" type="plane" size="1 1 1" pos="0 0 -1"/>'
              '<body name="ball" pos="0 0 1"><freejoint/><geom name="s" type="sphere" size="0.1"/></body></worldbody></mujoco>')


def _bid(m, b):
    return m.name2id("body", b) if isinstance(b, str) else int(b)


def r32(x):
    return np.float32(x).astype(np.float64)


def pair_dists(m, q, g1, g2):
    return wb.pair_rows(m, wb.frames(m, q), list(g1), list(g2))[0]


def collision_pairs(m):
    A = m.arrays
    return [int(g) for g in A["pair_geom1"]], [int(g) for g in A["pair_geom2"]]


def _kind(m, a, b):
    T = m.arrays["geom_type"]
    return tuple(sorted((int(T[a]), int(T[b]))))


KINDS = {"capsule-capsule": (mjcf.GEOM_CAPSULE, mjcf.GEOM_CAPSULE),
         "sphere-capsule": tuple(sorted((mjcf.GEOM_SPHERE, mjcf.GEOM_CAPSULE))),
         "plane-capsule": tuple(sorted((mjcf.GEOM_PLANE, mjcf.GEOM_CAPSULE)))}


def _overlaps(m, name, qstar, g1, g2):
    """Per kind: of the collision pairs that are apart at qpos*, the one that is deepest in every env at its overlap
    pose (and not degenerate there), the poses and the pair's distances at them."""
    tip, onto, limits = _bid(m, OVERLAP[name][0]), _bid(m, OVERLAP[name][1]), OVERLAP[name][2]
    hit = []
    for q in qstar:
        goal = ik.kinematics(m, q)["xpos"][onto] + np.array([0.02, 0.0, 0.0])
        hit.append(r32(ik.solve(m, [tip], None, goal[None], qpos_start=q, dofmask=0xFFFFFFC0, iterations=15, damping=1e-3,
                                limits=limits)[0]))
    out = {}
    for kind, key in KINDS.items():
        ks = [k for k in range(len(g1)) if _kind(m, g1[k], g2[k]) == key]
        a, b = [g1[k] for k in ks], [g2[k] for k in ks]
        poses = np.array(hit) if kind != "plane-capsule" else qstar
        D = np.array([pair_dists(m, q, a, b) for q in poses])
        deg = np.array([dref.degenerate(m, wb.scene(m, wb.frames(m, q)), a, b) for q in poses])
        # pairs that are apart at qpos* only: an overlap the model has in every pose (full's first links around its
        # torso) cannot be undone by any solve
        apart = np.array([pair_dists(m, q, a, b) for q in qstar]).min(0) > 0
        i = int(np.where(deg.any(0) | ~apart, np.inf, D.max(0)).argmin())
        dist = D[:, i]
        if kind == "plane-capsule":  # the root lowered until this capsule is 2 cm into the floor
            poses = poses.copy()
            poses[:, 2] -= dist + 0.02
            poses = r32(poses)
            dist = np.array([pair_dists(m, q, a[i:i + 1], b[i:i + 1])[0] for q in poses])
        out[kind] = dict(pair=(a[i], b[i]), start=poses, dist=dist, limits=limits)
    return out


@functools.lru_cache(maxsize=None)
def wb_problem(name):
    P = dict(problem(name))
    m = P["m"]
    for k in ("qstar", "start", "tpos", "tquat", "fquat"):
        P[k] = P[k][:NDISTINCT]
    P["roots"] = [0, _bid(m, SUBTREE[name])]
    P["com"] = {b: r32(np.array([wb.subtree_com(m, wb.frames(m, q), b) for q in P["qstar"]])) for b in P["roots"]}
    g1, g2 = collision_pairs(m)
    P["overlap"] = _overlaps(m, name, P["qstar"], g1, g2)
    # the mixed set of the parity cases at `start`: two pairs asked for more clearance than they have (active), two
    # that have far more than asked (inactive)
    D = np.array([pair_dists(m, q, g1, g2) for q in P["start"]])
    deg = np.array([dref.degenerate(m, wb.scene(m, wb.frames(m, q)), g1, g2) for q in P["start"]])
    ok = ~deg.any(0)
    near = [k for k in np.argsort(D.max(0)) if ok[k]][:2]
    far = [k for k in np.argsort(-D.min(0)) if ok[k]][:2]
    ks = [near[0], far[0], near[1], far[1]]
    P["mixed"] = dict(geom1=[g1[k] for k in ks], geom2=[g2[k] for k in ks],
                      clear_min=np.float32([D[:, near[0]].max() + 0.05, 0.01, D[:, near[1]].max() + 0.05, 0.02]),
                      clear_weight=np.float32([1.0, 1.0, 2.0, 0.5]), start_dist=D[:, ks])
    return P


def fd_rows(m, q, fn, h=1e-6):
    """Central differences of fn(frames) along every dof through integrate_pos."""
    active = np.ones(m.nv, bool)
    cols = []
    for d in range(m.nv):
        dq = np.zeros(m.nv)
        dq[d] = h
        cols.append((fn(wb.frames(m, ik.integrate_pos(m, q, dq, active, False)))
                     - fn(wb.frames(m, ik.integrate_pos(m, q, -dq, active, False)))) / (2 * h))
    return np.stack(cols, -1)


@pytest.mark.parametrize("name", MODELS)
def test_without_added_tasks_it_is_ik_ref(name):
    P = wb_problem(name)
    for dtype in (np.float64, np.float32):
        for e in range(2):
            kw = dict(qpos_start=P["start"][e], iterations=3, damping=DAMPING, posture=0.02, max_step=0.05, dtype=dtype)
            a = ik.solve(P["m"], P["body"], P["local"], P["tpos"][e], P["tquat"][e], **kw)
            b = wb.solve(P["m"], P["body"], P["local"], P["tpos"][e], P["tquat"][e], **kw)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
            assert b[0].dtype == dtype and b[4].shape == (0,) and b[5].shape == (4, 0)


@pytest.mark.parametrize("name", MODELS)
def test_rows_against_central_differences(name):
    P = wb_problem(name)
    m, q = P["m"], P["start"][1]
    o = wb.frames(m, q)
    for b in P["roots"]:
        J = wb.com_rows(m, o, b)
        fd = fd_rows(m, q, lambda oo: wb.subtree_com(m, oo, b))
        print(name, "com root", b, "max |J - fd|", np.abs(J - fd).max())
        assert np.abs(J - fd).max() <= 1e-6 and np.abs(fd).max() > 0.01
    M = P["mixed"]
    dist, rows = wb.pair_rows(m, o, M["geom1"], M["geom2"])
    fd = fd_rows(m, q, lambda oo: wb.pair_rows(m, oo, M["geom1"], M["geom2"])[0])
    print(name, "pairs", list(zip(M["geom1"], M["geom2"])), "dist", dist, "max |jac - fd|", np.abs(rows - fd).max())
    assert np.abs(rows - fd).max() <= dref.FD_TOL and np.abs(fd).max() > 0.1


@pytest.mark.parametrize("name", MODELS)
def test_reference_reaches_the_com_target(name):
    P = wb_problem(name)
    m = P["m"]
    for b in P["roots"]:
        for e in range(NDISTINCT):
            r = wb.solve(m, qpos_start=P["start"][e], iterations=ITERATIONS, damping=DAMPING, com_body=b, com_target=P["com"][b][e])
            e0 = P["com"][b][e] - wb.subtree_com(m, wb.frames(m, P["start"][e]), b)
            assert np.abs(e0).max() > 100 * COM_TOL
            assert np.abs(r[3]).max() < COM_TOL, (name, b, e, r[3])
            assert np.abs((P["com"][b][e] - wb.subtree_com(m, wb.frames(m, r[0]), b)) - r[3]).max() < 1e-12
    # (1, 1, 0): the height is left alone, its row reads zero
    r = wb.solve(m, qpos_start=P["start"][0], iterations=ITERATIONS, damping=DAMPING, com_body=0, com_target=P["com"][0][0],
                 com_weight=[1, 1, 0])
    assert r[3][2] == 0 and np.abs(r[3][:2]).max() < COM_TOL


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("kind", list(KINDS))
def test_reference_separates_overlapping_geoms(name, kind):
    P = wb_problem(name)
    m, O = P["m"], P["overlap"][kind]
    print(name, kind, O["pair"], "start dist", O["dist"])
    assert (O["dist"] < 0).all()  # the geoms do overlap at the start
    for dtype in (np.float64, np.float32):
        for e in range(NDISTINCT):
            r = wb.solve(m, qpos_start=O["start"][e], iterations=ITERATIONS, damping=DAMPING, geom1=[O["pair"][0]],
                         geom2=[O["pair"][1]], clear_min=[CLEAR_MIN], limits=O["limits"], dtype=dtype)
            assert r[4][0] >= np.float32(CLEAR_MIN) - CLEAR_TOL, (name, kind, e, dtype, r[4])
            assert r[5].shape == (ITERATIONS + 1, 1)


def test_inactive_pair_leaves_the_start_alone():
    P = wb_problem("humanoid_mjx")
    M = P["mixed"]
    r = wb.solve(P["m"], qpos_start=P["start"][0], iterations=3, damping=DAMPING, geom1=M["geom1"][1:2], geom2=M["geom2"][1:2],
                 clear_min=[0.01])
    assert np.array_equal(r[0], P["start"][0]) and (r[5] > MARGIN).all()


def test_exported_declared_and_bound():
    L = lib()
    assert hasattr(L, "mjl_ik_wb")
    protos = {p[1]: p for p in HEADER.protos}
    ikp, wbp = protos["mjl_ik"][2], protos["mjl_ik_wb"][2]
    assert wbp[:len(ikp) - 1] == ikp[:-1] and wbp[-1] == "void*"  # mjl_ik's arguments first, the stream last
    assert wbp[len(ikp) - 1:-1] == ["int", "float*", "float*", "int", "int32_t*", "int32_t*", "float*", "float*", "float*", "float*"]
    assert len(L.mjl_ik_wb.argtypes) == 31
    err = HEADER.enums["MJL_ERR_ARG"]
    assert L.mjl_ik_wb(None, None, 0, *([None] * 7), -1, 1, 1e-3, 0.0, 0.0, 0.0, 0, None, None, None, 0, None, None, 0, None, None, None,
                       None, None, None, None) == err  # a null batch: refused on the host
    assert callable(mjx.ik_wb) and mjx.WBIKResult._fields == ("qpos", "err", "niter", "com_err", "clearance")
    assert mjx.IKResult._fields == ("qpos", "err", "niter")
    from mjx_amd.envs import HumanoidEnv
    assert callable(HumanoidEnv.ik_wb)


def test_tables_are_resolved_on_the_host():
    m = mjx_amd.load_model("humanoid_mjx")

    class Sys:  # what the checks read of a mjx.Model (no GPU here)
        nbody, nv = m.nbody, m.nv
    Sys.m = m
    cb, cw, i1, i2, cmin, cwt = mjx.ik_wb_tables(Sys, "thigh_right", [1, 1, 0], (["floor", "hand_left"], ["foot1_left", 6]), 0.01, [1, 2])
    assert cb == m.name2id("body", "thigh_right") and cw.tolist() == [1, 1, 0] and cw.dtype == np.float32
    assert i1 == [0, 19] and i2 == [12, 6] and cmin.tolist() == [np.float32(0.01)] * 2 and cwt.tolist() == [1, 2]
    assert mjx.ik_wb_tables(Sys)[1:4] == (None, [], [])
    g1, g2 = mjx.collision_pairs(Sys)
    assert len(g1) > mjx.MAX_IK_PAIRS
    with pytest.raises(ValueError, match="32"):
        mjx.ik_wb_tables(Sys, clearance=(g1, g2))
    assert len(mjx.ik_wb_tables(Sys, clearance=(g1[:32], g2[:32]))[2]) == 32
    bad = [dict(clearance=("no_such_geom", "floor")), dict(clearance=(0, m.ngeom)), dict(clearance=(3, 3)),
           dict(com_body="no_such_body"), dict(com_body=m.nbody), dict(com_weight=[1, -1, 1]),
           dict(clearance=(0, 6), clearance_min=-0.01), dict(clearance=(0, 6), clearance_weight=[np.inf]),
           dict(clearance=([0, 1], [6]))]
    for kw in bad:
        with pytest.raises(ValueError):
            mjx.ik_wb_tables(Sys, **kw)
    two = mjcf.compile_xml_string(TWO_PLANES, "two_planes")

    class Sys2:
        nbody, nv, m = two.nbody, two.nv, two
    with pytest.raises(ValueError, match="both planes"):
        mjx.ik_wb_tables(Sys2, clearance=("a", "b"))
    assert mjx.ik_wb_tables(Sys2, clearance=("a", "s"))[2:4] == ([0], [2])
