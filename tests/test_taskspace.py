"""Task-space dynamics readout (mjl_jac_dot / mjl_centroidal), the part that needs no GPU: tests/taskspace_ref.py
against the definition (central differences of dyn_ref.jac along the motion, float64), its identities against
tests/bodydata_ref.py, and the declaration, its binding, the host-side argument checks and the Python surface.

Central differences: qpos+- = integrate(qpos, +-H qvel) (the free joint by the quaternion exponential of its
body-local rates), an oracle forward at each, the point fixed in its body. Bound: 1e-6 x max(1, max |value|). With
H = 3e-6 the truncation (O(H^2)) and the round-off (about 1e-16 x scale / H) are both near 1e-9 or below, three
orders under the bound, and a wrong formula is wrong at O(1)."""
import ctypes as C

import numpy as np
import pytest

import mjx_amd
from mjx_amd import mjcf, mjx
from mjx_amd._header import HEADER
from mjx_amd._lib import lib
from oracle import Oracle, state_arrays

import bodydata_ref as bref
import dyn_ref as dr
import generic_models as gm
import taskspace_ref as tr
from test_bodydata import build_states
from test_dyn import generic_states, sample_points

H = 3e-6
MODELS = list(mjx_amd.BUILTIN_MODELS) + ["two_trees", "full"]
_CACHE = {}


def load(name):
    """(model, states, oracle forward outputs), built once per model."""
    if name not in _CACHE:
        if name == "two_trees":
            m = mjcf.compile_xml_string(tr.TWO_TREES, name)
            states = generic_states(m, 4)
        elif name == "full":
            m = gm.full()
            states = generic_states(m)
        else:
            m = mjx_amd.load_model(name)
            states = build_states(m)
        orc = Oracle(m)
        _CACHE[name] = (m, states, [state_arrays(m, orc.forward(orc.new_state(*st))) for st in states])
    return _CACHE[name]


def roots_of(m):
    """Subtree roots: the whole model, the first body, a mid body and a leaf."""
    return [0, 1, m.nbody // 2, m.nbody - 1]


def _bound(*values):
    return 1e-6 * max(1.0, max(float(np.abs(v).max()) for v in values))


@pytest.mark.parametrize("name", MODELS)
def test_reference_against_central_differences(name):
    m, states, outs = load(name)
    orc = Oracle(m)
    pts = sample_points(m, np.random.default_rng(1))
    worst = {"jacp_dot": 0.0, "jacr_dot": 0.0, "com_bias": 0.0, "angmom_bias": 0.0}
    moved = 0.0
    for st, o in zip(states, outs):
        qpos, qvel = st[0], st[1]
        side = []
        for s in (1.0, -1.0):
            os_ = state_arrays(m, orc.forward(orc.new_state(tr.integrate(m, qpos, qvel, s * H), *st[1:])))
            axes = dr.dof_axes(m, os_)
            jacs = [dr.jac(m, os_, b, dr.local_point(os_, b, off), axes=axes) for b, off in pts]
            cen = [tr.centroidal(m, os_, qvel, b)[:2] for b in roots_of(m)]
            side.append((jacs, cen))
        axes = dr.dof_axes(m, o)
        rates = tr.dof_rates(m, o, qvel, axes=axes)
        for k, (b, off) in enumerate(pts):
            jpd, jrd, jdv = tr.jac_dot(m, o, b, dr.local_point(o, b, off), qvel, axes=axes, rates=rates)
            fdp = (side[0][0][k][0] - side[1][0][k][0]) / (2 * H)
            fdr = (side[0][0][k][1] - side[1][0][k][1]) / (2 * H)
            for f, got, want in (("jacp_dot", jpd, fdp), ("jacr_dot", jrd, fdr)):
                err = float(np.abs(got - want).max())
                worst[f] = max(worst[f], err / _bound(want))
                assert err <= _bound(want), (name, f, b, err)
            assert np.abs(jdv - np.concatenate([jpd @ qvel, jrd @ qvel])).max() <= 1e-12 * max(1.0, np.abs(jdv).max())
            moved = max(moved, float(np.abs(fdp).max()))
        for k, b in enumerate(roots_of(m)):
            bias = tr.centroidal(m, o, qvel, b, axes=axes, rates=rates)[2]
            want = np.concatenate([(side[0][1][k][i] - side[1][1][k][i]) / (2 * H) @ qvel for i in (0, 1)])
            for f, sl in (("com_bias", slice(0, 3)), ("angmom_bias", slice(3, 6))):
                err = float(np.abs(bias[sl] - want[sl]).max())
                worst[f] = max(worst[f], err / _bound(want[sl]))
                assert err <= _bound(want[sl]), (name, f, b, err)
    print(name, "worst error / bound:", {k: float(f"{v:.3g}") for k, v in worst.items()})
    assert moved > 0.1  # the Jacobians do change along the motion


@pytest.mark.parametrize("name", MODELS)
def test_centroidal_identities(name):
    """jac_com qvel / angmom_mat qvel against bodydata_ref's subtree_linvel / subtree_angmom; m_b jac_com of the
    whole model against sum_k m_k jacp_k; in float64, to rounding."""
    m, states, outs = load(name)
    mass = np.asarray(m.body_mass, np.float64)
    for st, o in zip(states, outs):
        qvel = st[1]
        ref = bref.body_data(m, dict(o, qvel=qvel))
        axes = dr.dof_axes(m, o)
        for b in roots_of(m):
            jc, am, _ = tr.centroidal(m, o, qvel, b, axes=axes)
            for got, want in ((jc @ qvel, ref["subtree_linvel"][b]), (am @ qvel, ref["subtree_angmom"][b])):
                assert np.abs(got - want).max() <= 1e-11 * max(1.0, np.abs(want).max()), (name, b)
        total = sum(mass[k] * dr.jac(m, o, k, o["xipos"][k], axes=axes)[0] for k in range(1, m.nbody))
        jc0 = tr.centroidal(m, o, qvel, 0, axes=axes)[0]
        assert np.abs(mass.sum() * jc0 - total).max() <= 1e-12 * np.abs(total).max()


def test_zero_velocity_and_massless_subtree():
    m, states, outs = load("two_trees")
    o, zero = outs[0], np.zeros(m.nv)
    jpd, jrd, jdv = tr.jac_dot(m, o, m.nbody - 2, o["xpos"][m.nbody - 2], zero)
    assert not jpd.any() and not jrd.any() and not jdv.any()
    assert not tr.centroidal(m, o, zero, 0)[2].any()
    out = tr.centroidal(m, o, states[0][1], 1, mass=np.zeros(m.nbody))
    assert all(not x.any() for x in out)


def test_exported_declared_and_bound():
    L = lib()
    assert hasattr(L, "mjl_jac_dot") and hasattr(L, "mjl_centroidal")
    protos = {p[1]: p for p in HEADER.protos}
    assert protos["mjl_jac_dot"][2] == ["mjlBatch*", "float*", "int", "int32_t*", "int", "float*", "float*", "float*",
                                        "float*", "void*"]
    assert protos["mjl_centroidal"][2] == ["mjlBatch*", "float*", "int", "int32_t*", "float*", "float*", "float*", "void*"]
    assert len(L.mjl_jac_dot.argtypes) == 10 and len(L.mjl_centroidal.argtypes) == 8
    for f in ("jac_dot", "jac_dot_local", "jac_subtree_com", "angmom_mat", "centroidal"):
        assert callable(getattr(mjx, f)), f
    from mjx_amd.envs import HumanoidEnv
    assert callable(HumanoidEnv.jac_dot) and callable(HumanoidEnv.centroidal)


def test_argument_checks_need_no_gpu():
    """A null batch, a null body, every output NULL, npoint / nsub out of range, an unknown frame and a world
    frame without points are refused before anything touches the device: the checks read no member of the batch,
    so a stand-in handle serves where there is no GPU to create one on."""
    L, err = lib(), HEADER.enums["MJL_ERR_ARG"]
    fake = C.create_string_buffer(1 << 16)
    h = C.cast(fake, C.c_void_p)
    buf = lambda: C.cast(C.create_string_buffer(64), C.c_void_p)
    body, pnt, a, b, c = buf(), buf(), buf(), buf(), buf()
    cases = [L.mjl_jac_dot(None, None, 1, body, 0, pnt, a, b, c, None),
             L.mjl_jac_dot(h, None, 1, None, 0, pnt, a, b, c, None),
             L.mjl_jac_dot(h, None, 1, body, 0, pnt, None, None, None, None),
             L.mjl_jac_dot(h, None, 0, body, 0, pnt, a, b, c, None),
             L.mjl_jac_dot(h, None, 257, body, 0, pnt, a, b, c, None),
             L.mjl_jac_dot(h, None, 1, body, 2, pnt, a, b, c, None),
             L.mjl_jac_dot(h, None, 1, body, 0, None, a, b, c, None),
             L.mjl_centroidal(None, None, 1, body, a, b, c, None),
             L.mjl_centroidal(h, None, 1, None, a, b, c, None),
             L.mjl_centroidal(h, None, 1, body, None, None, None, None),
             L.mjl_centroidal(h, None, 0, body, a, b, c, None),
             L.mjl_centroidal(h, None, 33, body, a, b, c, None)]
    for i, rc in enumerate(cases):
        assert rc == err, (i, rc)
    assert len(L.mjl_last_error()) > 10


def test_subtree_arguments_are_checked_on_the_host():
    m = mjx_amd.load_model("humanoid_mjx")

    class Sys:  # what the checks read of a mjx.Model (no GPU here)
        nbody, nv = m.nbody, m.nv
    Sys.m = m
    assert mjx._subtree_roots(Sys, ["pelvis", 0, 2]) == [m.name2id("body", "pelvis"), 0, 2]
    for bad in (-1, m.nbody, "no_such_body", [], [0] * 33):
        with pytest.raises(ValueError):
            mjx._subtree_roots(Sys, bad)
