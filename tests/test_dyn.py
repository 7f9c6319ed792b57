"""Jacobian and mass-matrix readout (mjl_jac / mjl_mass_matrix), the part that needs no GPU: tests/dyn_ref.py
against the oracle's M, against central differences of the oracle's kinematics and against its cdof, and the
declaration, its binding and the Python surface."""
import numpy as np
import pytest

import mjx_amd
from mjx_amd import abi, mjcf, mjx
from mjx_amd._header import HEADER
from mjx_amd._lib import lib
from oracle import Oracle, state_arrays

import dyn_ref as dr
import generic_models as gm
from test_bodydata import build_states

H = 1e-6  # the central differences' step along each dof


def generic_states(m, n=2, seed=3):
    """(qpos, qvel, qacc_warmstart, ctrl) x n for a model that need not be a humanoid: every free joint moved and
    turned, every hinge off its zero; rounded to float32."""
    rng = np.random.default_rng(seed)
    A, out = m.arrays, []
    for _ in range(n):
        q = np.array(m.qpos0, np.float64)
        for j in range(m.njnt):
            a = int(A["jnt_qposadr"][j])
            if A["jnt_type"][j] == mjcf.JNT_FREE:
                q[a:a + 3] += rng.uniform(-0.2, 0.2, 3)
                quat = np.asarray(q[a + 3:a + 7]) + rng.uniform(-0.4, 0.4, 4)
                q[a + 3:a + 7] = quat / np.linalg.norm(quat)
            else:
                q[a] += rng.uniform(-0.4, 0.4)
        out.append((q, rng.uniform(-1, 1, m.nv), np.zeros(m.nv), rng.uniform(-1, 1, m.nu)))
    return [tuple(np.float32(x).astype(np.float64) for x in st) for st in out]


def models():
    return [(n, mjx_amd.load_model(n)) for n in mjx_amd.BUILTIN_MODELS] + [("full", gm.full())]


def states_of(name, m):
    return generic_states(m) if name == "full" else build_states(m)[:2]


def forward(m, st):
    orc = Oracle(m)
    return state_arrays(m, orc.forward(orc.new_state(*st)))


def sample_points(m, rng):
    """(body, local offset): every body's origin and three bodies with an offset."""
    pts = [(b, None) for b in range(m.nbody)]
    return pts + [(b, rng.uniform(-0.3, 0.3, 3)) for b in (1, m.nbody // 2, m.nbody - 1)]


@pytest.mark.parametrize("name,m", models(), ids=lambda x: x if isinstance(x, str) else "")
def test_mass_matrix_against_the_oracle(name, m):
    for st in states_of(name, m):
        o = forward(m, st)
        M = dr.mass_matrix(m, o)
        err = np.abs(M - o["M"]).max() / np.abs(o["M"]).max()
        print(name, "max |M_ref - M_oracle| / max |M|:", err)
        assert err <= 1e-10
        assert np.array_equal(M, M.T) or np.abs(M - M.T).max() <= 1e-13 * np.abs(M).max()


def perturbed(m, q, d, eps):
    """qpos moved by eps along dof d: a hinge angle, a free joint's world translation, or its rotation advanced by
    the body-local quaternion exponential (as the integrator advances it)."""
    A = m.arrays
    j = int(A["dof_jntid"][d])
    a, k = int(A["jnt_qposadr"][j]), d - int(A["jnt_dofadr"][j])
    q = q.copy()
    if A["jnt_type"][j] != mjcf.JNT_FREE:
        q[a] += eps
    elif k < 3:
        q[a + k] += eps
    else:
        e = np.zeros(3)
        e[k - 3] = 1.0
        q[a + 3:a + 7] = mjcf.quat_mul(q[a + 3:a + 7], np.concatenate([[np.cos(eps / 2)], np.sin(eps / 2) * e]))
    return q


@pytest.mark.parametrize("name,m", models(), ids=lambda x: x if isinstance(x, str) else "")
def test_jacobian_against_finite_differences(name, m):
    rng = np.random.default_rng(1)
    st = states_of(name, m)[-1]
    o = forward(m, st)
    pts = sample_points(m, rng)
    xs = lambda oo: np.array([dr.local_point(oo, b, off) for b, off in pts])
    Rs = lambda oo: np.array([dr._q2m(np.asarray(oo["xquat"][b])) for b, _ in pts])
    R0 = Rs(o)
    fdp, fdr = np.zeros((len(pts), 3, m.nv)), np.zeros((len(pts), 3, m.nv))
    for d in range(m.nv):
        op = forward(m, (perturbed(m, st[0], d, H),) + st[1:])
        om = forward(m, (perturbed(m, st[0], d, -H),) + st[1:])
        fdp[:, :, d] = (xs(op) - xs(om)) / (2 * H)
        W = np.einsum("pij,pkj->pik", (Rs(op) - Rs(om)) / (2 * H), R0)  # [w]x = dR/dt R'
        fdr[:, :, d] = np.stack([W[:, 2, 1], W[:, 0, 2], W[:, 1, 0]], axis=1)
    worst = 0.0
    for k, (b, off) in enumerate(pts):
        jp, jr = dr.jac(m, o, b, dr.local_point(o, b, off))
        worst = max(worst, np.abs(jp - fdp[k]).max(), np.abs(jr - fdr[k]).max())
    print(name, "max |jac - central differences|:", worst)
    assert worst <= 1e-6
    assert np.abs(fdp).max() > 0.1 and np.abs(fdr).max() > 0.5  # the points do move


@pytest.mark.parametrize("name,m", models(), ids=lambda x: x if isinstance(x, str) else "")
def test_jacobian_against_cdof(name, m):
    rng = np.random.default_rng(2)
    for st in states_of(name, m):
        o = forward(m, st)
        for b, off in sample_points(m, rng):
            x = dr.local_point(o, b, off)
            jp, jr = dr.jac(m, o, b, x)
            wp, wr = np.zeros((3, m.nv)), np.zeros((3, m.nv))
            c0 = o["subtree_com"][int(m.arrays["body_rootid"][b])]
            for d in dr.body_dofs(m, b):
                wr[:, d] = o["cdof"][d][:3]
                wp[:, d] = o["cdof"][d][3:] + np.cross(o["cdof"][d][:3], x - c0)
            assert np.abs(jr - wr).max() <= 1e-12 and np.abs(jp - wp).max() <= 1e-12, (name, b)


def test_solve_is_the_inverse():
    m = mjx_amd.load_model("humanoid_mjx")
    o = forward(m, build_states(m)[0])
    M = dr.mass_matrix(m, o)
    v = np.random.default_rng(0).uniform(-1, 1, (3, m.nv))
    x = dr.solve(M, v)
    assert np.abs(x @ M - v).max() <= 1e-12 * np.abs(v).max() * np.linalg.cond(M)
    assert dr.solve(M, v[0]).shape == (m.nv,)


def test_exported_declared_and_bound():
    L = lib()
    assert hasattr(L, "mjl_jac") and hasattr(L, "mjl_mass_matrix")
    assert HEADER.enums["MJL_JAC_WORLD"] == 0 and HEADER.enums["MJL_JAC_LOCAL"] == 1
    assert abi.JAC_FRAME == {"world": 0, "local": 1}
    protos = {p[1]: p for p in HEADER.protos}
    assert protos["mjl_jac"][2] == ["mjlBatch*", "float*", "int", "int32_t*", "int", "float*", "float*", "float*",
                                    "float*", "void*"]
    assert protos["mjl_mass_matrix"][2] == ["mjlBatch*", "float*", "float*", "int", "float*", "float*", "float*", "void*"]
    assert len(L.mjl_jac.argtypes) == 10 and len(L.mjl_mass_matrix.argtypes) == 8
    err = HEADER.enums["MJL_ERR_ARG"]
    assert L.mjl_jac(None, None, 1, None, 0, None, None, None, None, None) == err  # a null batch: refused on the host
    assert L.mjl_mass_matrix(None, None, None, 0, None, None, None, None) == err
    for f in ("jac", "jac_local", "full_m", "mul_m", "solve_m"):
        assert callable(getattr(mjx, f)), f
    from mjx_amd.envs import HumanoidEnv
    assert callable(HumanoidEnv.jac) and callable(HumanoidEnv.full_m)


def test_body_and_frame_arguments_are_checked_on_the_host():
    m = mjx_amd.load_model("humanoid_mjx")

    class Sys:  # what the checks read of a mjx.Model (no GPU here)
        nbody, nv = m.nbody, m.nv
    Sys.m = m
    assert mjx._jac_bodies(Sys, ["pelvis", 2]) == [m.name2id("body", "pelvis"), 2]
    for bad in (-1, m.nbody, "no_such_body", []):
        with pytest.raises(ValueError):
            mjx._jac_bodies(Sys, bad)
    bodies, local = mjx.jac_frames(Sys, ["pelvis", ("site", 0), ("xbody", 3)], offset=[0.1, 0.0, 0.0])
    assert bodies == [m.name2id("body", "pelvis"), int(m.arrays["site_bodyid"][0]), 3]
    assert np.allclose(local[0], [0.1, 0, 0]) and local.dtype == np.float32
    R = mjcf.quat2mat(np.asarray(m.arrays["site_quat"][0], np.float64))
    assert np.allclose(local[1], np.asarray(m.arrays["site_pos"][0]) + R @ [0.1, 0, 0], atol=1e-7)
    with pytest.raises(ValueError):
        mjx.jac_frames(Sys, [("site", m.nsite)])
    with pytest.raises(ValueError):
        mjx.jac_frames(Sys, [("xbody", m.nbody)])
