"""Step linearization (mjl_step_jacobian / mjx.transition / mjx.step_jacobian), the part that needs no GPU: the
declaration, its binding and argument checks, and tests/linearize_ref.py's tangent-space reference against central
differences of the oracle's step taken through MuJoCo's own definitions of a tangent perturbation (integrate_pos)
and a tangent difference (differentiate_pos): the convention is pinned to those, not to the kernel."""
import numpy as np
import pytest

import mjx_amd
from mjx_amd import abi, mjx
from mjx_amd._header import HEADER
from mjx_amd._lib import lib
from oracle import Oracle, state_arrays

import linearize_ref as lr
from test_adjoint import _states


def generic_model_and_states():
    """The motor-only generic-dims model of the GPU test (tests/generic_models.py `tail`, which mjl_step_vjp
    accepts: tests/test_generic_gpu.py) with the four states that test uses."""
    import generic_models as gm
    from test_generic_gpu import states_of
    return gm.MODELS["tail"][0](), states_of("tail")[:4]


def test_exported_declared_and_bound():
    L = lib()
    assert hasattr(L, "mjl_step_jacobian")
    assert HEADER.enums["MJL_JAC_TANGENT"] == 1 and abi.JAC_TANGENT == 1
    assert abi.JAC_FRAME == {"world": 0, "local": 1}  # mjl_jac's frames keep their table
    assert abi.OPT_LINEARIZE_GROUPS == HEADER.enums["MJL_OPT_LINEARIZE_GROUPS"] == 7
    protos = {p[1]: p for p in HEADER.protos}
    assert protos["mjl_step_jacobian"][2] == ["mjlBatch*", "float*", "float*", "int", "float*", "float*", "void*"]
    assert len(L.mjl_step_jacobian.argtypes) == 7
    assert callable(mjx.transition) and callable(mjx.step_jacobian)
    from mjx_amd.envs import HumanoidEnv
    assert callable(HumanoidEnv.transition)


def test_argument_checks_need_no_gpu():
    """A null batch, both outputs null and an unknown flag bit are refused before anything touches the device: the
    checks read no member of the batch, so a stand-in handle serves where there is no GPU to create one on."""
    import ctypes as C
    L, err = lib(), HEADER.enums["MJL_ERR_ARG"]
    fake = C.create_string_buffer(1 << 16)
    h, out = C.cast(fake, C.c_void_p), C.cast(C.create_string_buffer(64), C.c_void_p)
    assert L.mjl_step_jacobian(None, None, None, 0, out, out, None) == err
    assert L.mjl_step_jacobian(None, None, None, abi.JAC_TANGENT, None, None, None) == err
    assert L.mjl_step_jacobian(h, None, None, abi.JAC_TANGENT, None, None, None) == err
    assert b"both NULL" in L.mjl_last_error()
    for flags in (2, 3, -1, 1 << 8):
        assert L.mjl_step_jacobian(h, None, None, flags, out, None, None) == err, flags
        assert L.mjl_step_jacobian(h, None, None, flags, None, out, None) == err, flags
    assert b"flags" in L.mjl_last_error()


def test_integrate_and_differentiate_pos_are_inverse():
    m = mjx_amd.load_model("humanoid_mjx")
    rng = np.random.default_rng(0)
    q0 = _states(m, 1, 1)[0][0]
    for scale in (1e-6, 1e-2, 1.0):
        dq = scale * rng.normal(size=m.nv)
        q1 = lr.integrate_pos(m, q0, dq)
        assert abs(np.linalg.norm(q1[3:7]) - 1) < 1e-14
        assert np.abs(lr.differentiate_pos(m, q1, q0) - dq).max() <= 1e-12


def _fd_check(m, states):
    """Reference (A, B) of every state against central differences of Oracle.step: inputs perturbed through
    integrate_pos, outputs differenced through differentiate_pos about the unperturbed post-step qpos; eps 1e-6,
    bound 1e-5 (1 + max|.|), tests/test_adjoint.py's rule for the raw Jacobian."""
    o = Oracle(m)
    nq, nv, nu = m.nq, m.nv, m.nu
    eps = 1e-6
    for q, v, w, c in states:
        J = o.step_jacobian(o.new_state(q, v, w, c))
        a0 = state_arrays(m, o.step(o.new_state(q, v, w, c)))
        qn = a0["qpos"]
        A, B = lr.tangent_AB(m, J, q, qn)
        assert A.shape == (2 * nv, 2 * nv) and B.shape == (2 * nv, nu)

        def F(dq, dv, du):
            a = state_arrays(m, o.step(o.new_state(lr.integrate_pos(m, q, dq), v + dv, w, c + du)))
            return np.concatenate([lr.differentiate_pos(m, a["qpos"], qn), a["qvel"]])

        cols = []
        for i in range(2 * nv + nu):
            e = np.zeros(2 * nv + nu)
            e[i] = eps
            cols.append((F(e[:nv], e[nv:2 * nv], e[2 * nv:]) - F(-e[:nv], -e[nv:2 * nv], -e[2 * nv:])) / (2 * eps))
        fd = np.stack(cols, 1)
        ref = np.concatenate([A, B], 1)
        err, bound = np.abs(ref - fd).max(), 1e-5 * (1 + np.abs(fd).max())
        print("tangent (A, B) vs central differences: %.3g (bound %.3g)" % (err, bound))
        assert err <= bound


@pytest.mark.parametrize("name", list(mjx_amd.BUILTIN_MODELS))
def test_reference_matches_central_differences(name):
    m = mjx_amd.load_model(name)
    _fd_check(m, _states(m, 2, 1))


def test_reference_matches_central_differences_generic_model():
    """The generic-dims model of the GPU test: its oracle Jacobian and the tangent maps satisfy the same check."""
    m, states = generic_model_and_states()
    assert m.nv > 27 and all(int(k) == 0 for k in np.asarray(getattr(m, "actuator_kind", np.zeros(m.nu)))[:m.nu])
    _fd_check(m, states[1:3])


def test_raw_split_is_the_oracles_matrix():
    m = mjx_amd.load_model("humanoid_mjx")
    o = Oracle(m)
    q, v, w, c = _states(m, 1, 1)[0]
    J = o.step_jacobian(o.new_state(q, v, w, c))
    A, B = lr.raw_AB(m, J)
    assert A.shape == (m.nq + m.nv, m.nq + m.nv) and B.shape == (m.nq + m.nv, m.nu)
    assert np.array_equal(np.concatenate([A, B], 1), J)
    # hinge-only directions of the tangent layout are the raw entries
    At, _ = lr.tangent_AB(m, J, q, state_arrays(m, o.step(o.new_state(q, v, w, c)))["qpos"])
    assert np.allclose(At[6:m.nv, 6:m.nv], A[7:m.nq, 7:m.nq], rtol=0, atol=1e-12)
