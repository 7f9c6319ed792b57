"""Inverse dynamics (mjl_inverse / mjx.inverse), the part that needs no GPU: tests/inverse_ref.py's rebuilt
constraint rows against the oracle's own forces, the declaration, its binding and argument checks, and the
conditions the GPU test's inputs (cases() below, shared with tests/test_inverse_gpu.py) have to meet."""
import functools

import numpy as np
import pytest

import mjx_amd
from mjx_amd import abi, mjx
from mjx_amd._header import HEADER
from mjx_amd._lib import lib
from oracle import Oracle, state_arrays

import inverse_ref as ir

MODELS = list(mjx_amd.BUILTIN_MODELS) + ["two_trees", "full"]
# The seeded perturbation of the second test acceleration, per dof: N(0, 1) x PERTURB. The forward solutions of
# these states have |qacc| of order 10 to 1000 (contacts), so a perturbation of this size moves J qacc by more
# than the rows' residuals and flips rows both ways (asserted below).
PERTURB = 50.0


@functools.lru_cache(maxsize=None)
def cases(name):
    """The model, its states, and per state the float64 and float32 oracle forward outputs (arrays, raw state)
    and the three test accelerations [3, nv] (rounded to float32): the float64 oracle's forward qacc, that plus
    the seeded perturbation, zeros."""
    from test_dyn_gpu import _model
    m, states = _model(name)
    rng = np.random.default_rng(12)
    out = []
    for st in states:
        rec = {}
        for key, orc in (("f64", Oracle(m)), ("f32", Oracle(m, use_float=True))):
            raw = orc.forward(orc.new_state(*st))
            rec[key] = (state_arrays(m, raw), raw)
        qacc = rec["f64"][0]["qacc"]
        acc = np.stack([qacc, qacc + PERTURB * rng.standard_normal(m.nv), np.zeros(m.nv)])
        rec["acc"] = np.float32(acc).astype(np.float64)
        out.append(rec)
    return m, states, out


@pytest.mark.parametrize("name", MODELS)
def test_rebuilt_rows_give_the_oracles_forces(name):
    m, _, recs = cases(name)
    nrow = 0
    for rec in recs:
        o, raw = rec["f64"]
        J, kinds = ir.constraint_jacobian(m, o)
        assert list(kinds) == [int(t) for t in o["efc_type"]]
        nefc = int(o["nefc"])
        nrow += nefc
        if nefc == 0:
            continue
        scale = max(np.abs(o["qfrc_constraint"]).max(), 1e-300)
        err = np.abs(J.T @ o["efc_force"] - o["qfrc_constraint"]).max() / scale
        D, aref = np.array(raw.efc_D)[:nefc], np.array(raw.efc_aref)[:nefc]
        force, jar = ir.efc_force(J, D, aref, o["qacc"])
        ferr = np.abs(force - o["efc_force"]).max() / max(np.abs(o["efc_force"]).max(), 1e-300)
        print(name, "nefc", nefc, "J'f rel err %.3g" % err, "efc_force rel err %.3g" % ferr)
        assert err <= 1e-9 and ferr <= 1e-9
        # at the forward solution the inverse returns the actuator force (the solver's residual aside)
        qfrc, fc, _, _ = ir.inverse(m, o, raw, o["qacc"], J=J)
        assert np.abs(fc - o["qfrc_constraint"]).max() <= 1e-9 * scale
        assert np.abs(qfrc - o["qfrc_actuator"]).max() <= 1e-6 * max(1.0, np.abs(o["qfrc_bias"]).max())
    if name in mjx_amd.BUILTIN_MODELS:
        assert nrow > 0


@pytest.mark.parametrize("name", MODELS)
def test_input_conditions(name):
    m, _, recs = cases(name)
    contact = limit = inactive = flipped = False
    for rec in recs:
        (o, raw), (o32, _) = rec["f64"], rec["f32"]
        # no contact or limit sits on its margin: both precisions see the same rows
        assert o["ncon"] == o32["ncon"] and list(o["efc_type"]) == list(o32["efc_type"])
        J, kinds = ir.constraint_jacobian(m, o)
        nefc = int(o["nefc"])
        if nefc == 0:
            continue
        D, aref = np.array(raw.efc_D)[:nefc], np.array(raw.efc_aref)[:nefc]
        act = [ir.efc_force(J, D, aref, a)[1] < 0 for a in rec["acc"]]
        contact |= bool((act[0] & (kinds >= 2)).any())
        limit |= bool((act[0] & (kinds == 0)).any())
        inactive |= any(bool((~a).any()) for a in act)
        flipped |= bool((act[0] != act[1]).any())
    if name in mjx_amd.BUILTIN_MODELS:
        assert contact and limit and inactive and flipped, (contact, limit, inactive, flipped)


def test_discrete_reference_inverts_the_integrators_solve():
    """(M + dt K) a' = M a_c: the reference's a_c, fed back through the integrator's matrix, is the input."""
    for name in mjx_amd.BUILTIN_MODELS:
        m, _, recs = cases(name)
        k = ir.integrator_diagonal(m)
        assert k is not None and (k != 0).any()
        o = recs[0]["f64"][0]
        a = recs[0]["acc"][1]
        M = o["M"]
        a_c = a + m.timestep * np.linalg.solve(M, k * a)
        back = np.linalg.solve(M + m.timestep * np.diag(k), M @ a_c)
        assert np.abs(back - a).max() <= 1e-9 * np.abs(a).max()
        qd, _, _, _ = ir.inverse(m, o, recs[0]["f64"][1], a, discrete=True)
        qc, _, _, _ = ir.inverse(m, o, recs[0]["f64"][1], a_c)
        assert np.abs(qd - qc).max() <= 1e-9 * np.abs(qc).max()


def test_exported_declared_and_bound():
    L = lib()
    assert hasattr(L, "mjl_inverse")
    assert HEADER.enums["MJL_INV_DISCRETE"] == 1 and abi.INV_DISCRETE == 1
    protos = {p[1]: p for p in HEADER.protos}
    assert protos["mjl_inverse"][2] == ["mjlBatch*", "float*", "float*", "int", "float*", "float*", "void*"]
    assert len(L.mjl_inverse.argtypes) == 7
    err = HEADER.enums["MJL_ERR_ARG"]
    assert L.mjl_inverse(None, None, None, 0, None, None, None) == err  # a null batch: refused on the host
    assert callable(mjx.inverse)
    from mjx_amd.envs import HumanoidEnv
    assert callable(HumanoidEnv.inverse)


def test_argument_checks_need_no_gpu():
    """A null output and an unknown flag bit are refused before anything touches the device: the checks read no
    member of the batch, so a stand-in handle serves where there is no GPU to create one on."""
    import ctypes as C
    L, err = lib(), HEADER.enums["MJL_ERR_ARG"]
    fake = C.create_string_buffer(1 << 16)
    h, out = C.cast(fake, C.c_void_p), C.cast(C.create_string_buffer(64), C.c_void_p)
    assert L.mjl_inverse(None, None, None, 0, out, None, None) == err
    assert L.mjl_inverse(h, None, None, 0, None, None, None) == err
    assert len(L.mjl_last_error()) > 10
    for flags in (2, 3, -1, 1 << 8):
        assert L.mjl_inverse(h, None, None, flags, out, None, None) == err, flags
