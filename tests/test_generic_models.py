"""The models of tests/generic_models.py on the CPU: their dims, which side of mjl_model_create's dispatch rule
they fall on (the rule restated from the dims and pinned to the sources' Dims), that the host model build accepts
them, and the fp64 oracle pinned on them independently of any kernel (as tests/test_oracle_kat.py does for the
humanoids): gravity bias from the compiler's numpy Jacobians, the mass matrix from its numpy CRB, and the Newton
solution's KKT residual. Without these the GPU parity tests of tests/test_generic_gpu.py would compare the
generic kernels with an oracle nobody checked past 27 dofs."""
import ctypes as C
import re
import os

import numpy as np
import pytest

from mjx_amd import _lib, abi, mjcf
from oracle import Oracle, state_arrays

import generic_models as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (nv, nbody, njnt, ngeom)
DIMS = {
    "tail": (30, 20, 25, 23), "tail_euler": (30, 20, 25, 23),
    "nv_only": (28, 11, 18, 11), "nbody_only": (14, 18, 9, 18), "njnt_only": (23, 13, 23, 12),
    "ngeom_only": (6, 2, 1, 22), "full": (32, 32, 27, 32),
    "nv_at": (27, 11, 17, 11), "nbody_at": (14, 17, 9, 17), "njnt_at": (22, 12, 22, 11), "ngeom_at": (6, 2, 1, 20),
}


def test_dispatch_rule_restated_matches_the_sources():
    """generic_models.DHUM is csrc/step_kernels.hip's DHum, and the rule in capi.hip compares those four."""
    src = open(os.path.join(ROOT, "mujoco-mjx-lab_amd", "csrc", "step_kernels.hip")).read()
    nv, nb, nj, ng = map(int, re.search(r"using DHum = Dims<(\d+), (\d+), (\d+), (\d+),", src).groups())
    assert {"nv": nv, "nbody": nb, "njnt": nj, "ngeom": ng} == gm.DHUM
    gen = tuple(map(int, re.search(r"using DGen = Dims<(\d+), (\d+), (\d+), (\d+),", src).groups()))
    assert gen == (abi.MAXV, abi.MAXBODY, abi.MAXJNT, abi.MAXGEOM)
    capi = open(os.path.join(ROOT, "mujoco-mjx-lab_amd", "csrc", "capi.hip")).read()
    assert ("M->nvc = (d->nv <= DHum::NV && d->nbody <= DHum::NB && d->njnt <= DHum::NJ && d->ngeom <= DHum::NG) "
            "? 0 : 1;") in capi


@pytest.mark.parametrize("name", list(gm.MODELS))
def test_dims_and_side_of_the_rule(name):
    build, generic, over = gm.MODELS[name]
    m = build()
    assert (m.nv, m.nbody, m.njnt, m.ngeom) == DIMS[name]
    assert gm.within_capacities(m)
    assert gm.is_generic(m) == generic and gm.over(m) == over
    if not generic:  # a near miss sits exactly at the dim its family crosses
        fam = name.split("_")[0]
        assert getattr(m, fam) == gm.DHUM[fam]
        assert getattr(gm.MODELS[fam + "_only"][0](), fam) > gm.DHUM[fam]


def test_full_sits_at_the_capacities():
    m = gm.full()
    assert (m.nv, m.nbody, m.ngeom) == (abi.MAXV, abi.MAXBODY, abi.MAXGEOM)
    assert abi.MAXPAIR - 8 <= m.npair <= abi.MAXPAIR
    # a branching tree with welded bodies and two-joint bodies: the tree arrays are not a chain's
    assert sorted(set(np.bincount(m.body_parentid[1:]))) != [0, 1]
    assert (np.asarray(m.body_jntnum)[1:] == 0).sum() == 7 and (np.asarray(m.body_jntnum) == 2).sum() == 3
    assert len(set(np.asarray(m.body_level).tolist())) > 5
    assert (np.abs(np.asarray(m.body_quat)[2:, 1:]).max(axis=1) > 1e-3).all()
    assert np.abs(np.asarray(m.jnt_pos)[1:]).max() > 0
    inertia = np.asarray(m.body_inertia)  # [Ixx Iyy Izz Ixy Ixz Iyz] in the body frame
    assert inertia.shape == (m.nbody, 6) and (np.abs(inertia[2:, 3:]).max(axis=1) > 1e-3 * inertia[2:, :3].max(axis=1)).sum() > 10


def test_tail_keeps_the_humanoid_env_ingredients():
    for m in (gm.tail(), gm.tail_euler()):
        assert m.ntendon == 2 and m.nsensordata == 2 and m.nkey == 5 and m.nu == 24
        assert all(n in m.names["body"] for n in ("pelvis", "head") + gm.TAIL_LINKS)
        assert m.npair <= abi.MAXPAIR
        a = int(m.jnt_qposadr[m.names["joint"].index("tail1")])
        assert np.all(np.asarray(m.key_qpos)[:, a:a + 3] == 0)
    assert (gm.tail().integrator, gm.tail().eulerdamp) == (mjcf.INT_IMPLICITFAST, 0)
    assert (gm.tail_euler().integrator, gm.tail_euler().eulerdamp) == (mjcf.INT_EULER, 1)


@pytest.mark.parametrize("name", list(gm.MODELS))
def test_model_create_accepts(name):
    """mjl_model_create is host-only (tests/test_model_host.py): every model builds, with row / contact maxima."""
    L = _lib.lib()
    m = gm.MODELS[name][0]()
    d = abi.model_desc(m)
    h = C.c_void_p()
    rc = L.mjl_model_create(C.byref(d), C.byref(h))
    assert rc == 0, L.mjl_last_error().decode()
    try:
        assert L.mjl_model_nefc_max(h) >= m.njnt - 1 and L.mjl_model_ncon_max(h) >= m.npair
    finally:
        L.mjl_model_destroy(h)


def _poses(m, rng, n=3):
    out = []
    for _ in range(n):
        q = m.qpos0.copy()
        for j in range(m.njnt):
            a = int(m.jnt_qposadr[j])
            if m.jnt_type[j] == mjcf.JNT_FREE:
                q[a + 3:a + 7] = rng.normal(size=4)
                q[a + 3:a + 7] /= np.linalg.norm(q[a + 3:a + 7])
                q[a + 2] += 2.0   # off the floor
            else:
                q[a] += rng.uniform(-0.5, 0.5)
        out.append(q)
    return out


@pytest.mark.parametrize("name", list(gm.MODELS))
def test_oracle_gravity_bias_mass_matrix_and_fk(name):
    """qvel = 0: the oracle's qfrc_bias = sum_b -J_b(xipos_b)' m_b g, M and xpos equal the compiler's numpy ones."""
    m = gm.MODELS[name][0]()
    o = Oracle(m)
    for q in _poses(m, np.random.default_rng(1)):
        a = state_arrays(m, o.forward(o.new_state(q)))
        kin = mjcf._fk_and_mass(m, q)
        expect = np.zeros(m.nv)
        for b in range(1, m.nbody):
            jp, _ = mjcf.body_jacobian(m, kin, b, kin["xipos"][b])
            expect -= jp.T @ (m.body_mass[b] * m.gravity)
        np.testing.assert_allclose(a["qfrc_bias"], expect, atol=1e-9)
        np.testing.assert_allclose(a["M"], kin["M"], atol=1e-10)
        np.testing.assert_allclose(a["xpos"], kin["xpos"], atol=1e-12)


@pytest.mark.parametrize("name", list(gm.MODELS))
def test_oracle_newton_kkt(name):
    """At the oracle's Newton solution M (qacc - qacc_smooth) = qfrc_constraint with the compiler's numpy M, and
    every force is >= 0, on states with active rows (limits past their range; bodies in the floor)."""
    m = gm.MODELS[name][0]()
    assert m.solver == mjcf.SOLVER_NEWTON
    o = Oracle(m)
    rng = np.random.default_rng(2)
    checked = 0
    for k in range(3):
        q = m.qpos0.copy()
        for j in range(m.njnt):
            a = int(m.jnt_qposadr[j])
            if m.jnt_type[j] == mjcf.JNT_FREE:
                q[a + 2] -= 0.08 + 0.03 * k
            elif m.jnt_limited[j] and rng.uniform() < 0.4:
                q[a] = m.jnt_range[j][1] + 0.03
        s = o.forward(o.new_state(q, rng.uniform(-0.3, 0.3, m.nv), ctrl=rng.uniform(-1, 1, m.nu)))
        a = state_arrays(m, s)
        assert a["nefc"] > 0
        lhs = mjcf._fk_and_mass(m, q)["M"] @ (a["qacc"] - a["qacc_smooth"])
        np.testing.assert_allclose(lhs, a["qfrc_constraint"], atol=1e-6 * (1 + np.abs(lhs).max()))
        assert np.all(a["efc_force"] >= 0) and a["niter"] <= m.iterations
        checked += 1
    assert checked == 3
