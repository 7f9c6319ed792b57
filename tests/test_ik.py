"""Batched inverse kinematics (mjl_ik / mjx.ik), the part that needs no GPU: tests/ik_ref.py converges on reachable
targets with the constants the GPU convergence test uses, its Jacobians are the derivatives of its own kinematics
through integratePos, its kinematics are the oracle's, and the declaration, its binding and the Python surface.

The problems (shared with tests/test_ik_gpu.py): per model 4-5 envs; a reachable target is the task frames' pose at
qpos*, the env's state with every limited hinge moved MARGIN inside its range, and the start is qpos* with every hinge moved
by up to PERTURB rad (kept MARGIN inside the range), every free joint moved by up to PERTURB / 3 m and turned by up to
PERTURB rad."""
import functools

import numpy as np
import pytest

import mjx_amd
from mjx_amd import abi, mjcf, mjx
from mjx_amd._header import HEADER
from mjx_amd._lib import lib
from oracle import Oracle, state_arrays

import generic_models as gm
import ik_ref as ik
from test_bodydata import build_states
from test_dyn import generic_states

# Chosen here so that the float64 reference alone reaches POS_TOL / ROT_TOL on every task of every problem below
# (test_reference_converges prints the residual after every iteration count it tries).
PERTURB = 0.1       # rad
DAMPING = 1e-4
ITERATIONS = 10
MARGIN = 0.1        # rad: qpos* and the start keep this distance from the ends of jnt_range
POS_TOL, ROT_TOL = 1e-4, 1e-3  # m, rad

MODELS = list(mjx_amd.BUILTIN_MODELS) + ["two_trees", "full"]


def load(name):
    if name == "two_trees":
        from test_dyn_gpu import TWO_TREES
        m = mjcf.compile_xml_string(TWO_TREES, name)
        return m, generic_states(m, 4)
    if name == "full":
        m = gm.full()
        return m, generic_states(m, 4)
    m = mjx_amd.load_model(name)
    return m, build_states(m)


def frames_of(name, m):
    """(frames, offsets [ntask, 3] in the frames): a handful of sites and bodies, one nonzero offset."""
    if name == "two_trees":
        frames, k = [("site", 0), ("xbody", m.name2id("body", "a2"))], 1
    elif name == "full":
        frames, k = [("xbody", 7), ("xbody", 13), ("xbody", 19), ("xbody", 31)], 2
    else:
        frames = [("site", 0), ("site", 1)] + [("xbody", m.name2id("body", b)) for b in ("foot_right", "foot_left", "hand_left")]
        k = 3
    off = np.zeros((len(frames), 3))
    off[k] = [0.05, -0.02, 0.03]
    return frames, off


def tasks_of(m, frames, off):
    """(body ids, body-frame offsets, the frames' rotations in their bodies) as mjx.ik_tables builds them."""
    body, local, fq = ik.frame_tasks(m, frames)
    for t in range(len(body)):
        local[t] = local[t] + mjcf.quat2mat(fq[t]).reshape(3, 3) @ off[t]
    return body, np.float32(local).astype(np.float64), fq


def _free_joints(m):
    A = m.arrays
    return [int(A["jnt_qposadr"][j]) for j in range(m.njnt) if A["jnt_type"][j] == mjcf.JNT_FREE]


def in_range(m, q, margin=0.0):
    A = m.arrays
    q = q.copy()
    for j in range(m.njnt):
        if A["jnt_type"][j] == mjcf.JNT_HINGE and A["jnt_limited"][j]:
            a = int(A["jnt_qposadr"][j])
            lo, hi = A["jnt_range"][j]
            q[a] = min(max(q[a], lo + margin), hi - margin)
    return q


def perturb(m, q, rng, size):
    A = m.arrays
    q = q.copy()
    for j in range(m.njnt):
        a = int(A["jnt_qposadr"][j])
        if A["jnt_type"][j] == mjcf.JNT_FREE:
            q[a:a + 3] += rng.uniform(-size / 3, size / 3, 3)
            v = rng.normal(size=3)
            v *= rng.uniform(0, size) / np.linalg.norm(v)
            ang = np.linalg.norm(v)
            q[a + 3:a + 7] = mjcf.quat_mul(q[a + 3:a + 7], np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * v / ang]))
        else:
            q[a] += rng.uniform(-size, size)
    return in_range(m, q, MARGIN)


@functools.lru_cache(maxsize=None)
def problem(name):
    """Everything both test files need of one model; float32-representable inputs, float64 arrays."""
    m, states = load(name)
    frames, off = frames_of(name, m)
    body, local, fq = tasks_of(m, frames, off)
    rng = np.random.default_rng(11)
    r32 = lambda x: np.float32(x).astype(np.float64)
    qstar = np.array([r32(in_range(m, np.asarray(st[0], np.float64), MARGIN)) for st in states])
    start = np.array([r32(perturb(m, q, rng, PERTURB)) for q in qstar])
    poses = [ik.frame_pose(m, q, body, local) for q in qstar]
    tpos = r32(np.array([p[0] for p in poses]))
    tquat = r32(np.array([p[1] for p in poses]))  # the bodies'
    fquat = r32(np.array([[mjcf.quat_mul(p[1][t], fq[t]) for t in range(len(body))] for p in poses]))  # the frames'
    return dict(name=name, m=m, states=states, frames=frames, off=off, body=body, local=local, fq=fq, qstar=qstar,
                start=start, tpos=tpos, tquat=tquat, fquat=fquat)


def residual_norms(e):
    return np.linalg.norm(e[..., :3], axis=-1), np.linalg.norm(e[..., 3:], axis=-1)


@pytest.mark.parametrize("name", MODELS)
def test_reference_converges(name):
    P = problem(name)
    m = P["m"]
    worst = {}
    for e in range(len(P["start"])):
        for n in (5, ITERATIONS):
            q, err, k = ik.solve(m, P["body"], P["local"], P["tpos"][e], P["tquat"][e], qpos_start=P["start"][e],
                                 iterations=n, damping=DAMPING)
            ep, er = residual_norms(err)
            worst[n] = (max(worst.get(n, (0, 0))[0], ep.max()), max(worst.get(n, (0, 0))[1], er.max()))
        assert k == ITERATIONS
        assert ep.max() < POS_TOL and er.max() < ROT_TOL, (name, e, ep.max(), er.max())
        assert np.array_equal(q, in_range(m, q))  # limits=True: inside jnt_range
        # the residual it reports is the pose error of the qpos it returns
        x, bq = ik.frame_pose(m, q, P["body"], P["local"])
        assert np.abs((P["tpos"][e] - x) - err[:, :3]).max() < 1e-12
    print(name, "worst (|e_p|, |e_r|) after n iterations:", {n: (float(f"{a:.3g}"), float(f"{b:.3g}")) for n, (a, b) in worst.items()})
    # the start is off the target by far more than the tolerance
    _, e0, _ = ik.solve(m, P["body"], P["local"], P["tpos"][0], P["tquat"][0], qpos_start=P["start"][0], iterations=0)
    assert residual_norms(e0)[0].max() > 100 * POS_TOL


@pytest.mark.parametrize("name", MODELS)
def test_reference_kinematics_are_the_oracles(name):
    m, states = load(name)
    orc = Oracle(m)
    for st in states[:2]:
        o = state_arrays(m, orc.forward(orc.new_state(*st)))
        k = ik.kinematics(m, st[0])
        assert np.abs(k["xpos"] - o["xpos"]).max() < 1e-12
        assert np.abs(np.abs((k["xquat"] * o["xquat"]).sum(-1)) - 1).max() < 1e-12


@pytest.mark.parametrize("name", MODELS)
def test_reference_jacobian_against_central_differences(name):
    """task_rows against the central differences of the reference's own kinematics through integrate_pos."""
    P = problem(name)
    m, body, local = P["m"], P["body"], P["local"]
    q = P["start"][-1]
    o = ik.kinematics(m, q)
    xs, _ = ik.residuals(m, o, body, local, P["tpos"][-1], None)
    J = ik.task_rows(m, o, body, xs)
    h, active = 1e-6, np.ones(m.nv, bool)
    fd = np.zeros_like(J)
    for d in range(m.nv):
        dq = np.zeros(m.nv)
        dq[d] = h
        xp, qp = ik.frame_pose(m, ik.integrate_pos(m, q, dq, active, False), body, local)
        xm, qm = ik.frame_pose(m, ik.integrate_pos(m, q, -dq, active, False), body, local)
        fd[:, :3, d] = (xp - xm) / (2 * h)
        for t in range(len(body)):
            fd[t, 3:, d] = ik.rotvec(ik.dr._qmul(qp[t], ik._conj(qm[t]))) / (2 * h)
    worst = np.abs(J - fd).max()
    print(name, "max |J - central differences|:", worst)
    assert worst <= 1e-6
    assert np.abs(fd[:, :3]).max() > 0.1 and np.abs(fd[:, 3:]).max() > 0.5


def test_differentiate_inverts_integrate():
    m, states = load("humanoid_mjx")
    rng = np.random.default_rng(3)
    q = np.asarray(states[0][0], np.float64)
    dq = rng.uniform(-0.3, 0.3, m.nv)
    q2 = ik.integrate_pos(m, q, dq, np.ones(m.nv, bool), False)
    assert np.abs(ik.differentiate_pos(m, q2, q) - dq).max() < 1e-12
    part = np.arange(m.nv) >= 6
    q3 = ik.integrate_pos(m, q, dq, part, False)
    assert np.array_equal(q3[:7], q[:7]) and not np.array_equal(q3[7:], q[7:])


def test_exported_declared_and_bound():
    L = lib()
    assert hasattr(L, "mjl_ik")
    assert HEADER.enums["MJL_IK_LIMITS"] == 1 and abi.IK_LIMITS == 1
    protos = {p[1]: p for p in HEADER.protos}
    assert protos["mjl_ik"][2] == (["mjlBatch*", "float*", "int", "int32_t*"] + ["float*"] * 6 + ["int32_t", "int"]
                                   + ["float"] * 4 + ["int", "float*", "float*", "int32_t*", "void*"])
    assert len(L.mjl_ik.argtypes) == 21
    err = HEADER.enums["MJL_ERR_ARG"]
    assert L.mjl_ik(None, None, 1, None, None, None, None, None, None, None, -1, 1, 1e-3, 0.0, 0.0, 0.0, 0, None, None,
                    None, None) == err  # a null batch: refused on the host
    assert callable(mjx.ik) and mjx.IKResult._fields == ("qpos", "err", "niter")
    from mjx_amd.envs import HumanoidEnv
    assert callable(HumanoidEnv.ik)


def test_dofs_and_tables_are_resolved_on_the_host():
    m = mjx_amd.load_model("humanoid_mjx")

    class Sys:  # what the checks read of a mjx.Model (no GPU here)
        nbody, nv = m.nbody, m.nv
    Sys.m = m
    assert mjx.ik_dofmask(Sys, None) == 0xFFFFFFFF
    assert mjx.ik_dofmask(Sys, [0, 3, 26]) == (1 | 8 | 1 << 26)
    assert mjx.ik_dofmask(Sys, [d >= 6 for d in range(m.nv)]) == (1 << 27) - 64
    assert mjx.ik_dofmask(Sys, np.arange(m.nv) >= 6) == (1 << 27) - 64
    names = m.names["joint"]
    assert m.arrays["jnt_type"][0] == mjcf.JNT_FREE and names[0] and names[1]
    assert mjx.ik_dofmask(Sys, [names[1]]) == 1 << int(m.arrays["jnt_dofadr"][1])
    assert mjx.ik_dofmask(Sys, [names[0], names[1]]) == 63 | 1 << int(m.arrays["jnt_dofadr"][1])
    for bad in ([m.nv], [-1], ["no_such_joint"], [True, False]):
        with pytest.raises(ValueError):
            mjx.ik_dofmask(Sys, bad)
    frames, off = frames_of("humanoid_mjx", m)
    bodies, local, conj, w = mjx.ik_tables(Sys, frames, off, [[1, 0.5]])
    body, loc, fq = tasks_of(m, frames, off)
    assert bodies == body and np.abs(local - loc).max() < 1e-7 and w.shape == (5, 2) and w.dtype == np.float32
    assert np.abs(conj - np.float32(fq * [1, -1, -1, -1])).max() < 1e-7
    assert mjx.ik_tables(Sys, [("xbody", 1)])[2] is None
    with pytest.raises(ValueError):
        mjx.ik_tables(Sys, [("xbody", 1)] * 33)
    with pytest.raises(ValueError):
        mjx.ik_tables(Sys, [("xbody", 1)], weight=[[1, -1]])
