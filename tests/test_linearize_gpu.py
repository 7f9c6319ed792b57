"""Step linearization on the GPU (mjl_step_jacobian / mjx.transition / mjx.step_jacobian): every row of [A | B], in
both layouts, against the fp64 oracle's dual-number step Jacobian (tests/linearize_ref.py maps it to the tangent
layout; tests/test_linearize.py pins that map to central differences), under tests/test_adjoint.py's rule with the
row's basis cotangent: max|g - ref| / (max|ref| + 1e-3 max|J|) <= 2e-3 per input group. Then the properties of the
entry: agreement with the one-hot loop over mjx.step_vjp, independence of the row grouping, an untouched batch, the
ctrl argument, mask and partial outputs, the refusals, and capture with an env step.

MJX_LINEARIZE_PARITY=<path>: the worst error per model, layout and group goes there as JSON (the committed run:
profiles/linearize/parity.json)."""
import dataclasses
import functools
import json
import os

import numpy as np
import pytest
import torch

import mjx_amd
from mjx_amd import abi, actuators, mjx
from mjx_amd._lib import MjlError, lib
from mjx_amd.config import reference_ppo_config
from mjx_amd.envs import HumanoidEnv, resolve_ids
from oracle import Oracle, state_arrays

import linearize_ref as lr
from test_adjoint import _states
from test_linearize import generic_model_and_states

pytestmark = pytest.mark.gpu

MODELS = ["humanoid_mjx", "humanoid", "tail"]  # tail: generic dims (linearize_kernel<DGen>), motors only
TOL = 2e-3
MAX_GROUPS = 16  # the most row groups the host rule picks and MJL_OPT_LINEARIZE_GROUPS accepts
SENTINEL = -77.0
PARITY = {}


@pytest.fixture(scope="module", autouse=True)
def _write_parity():
    yield
    path = os.environ.get("MJX_LINEARIZE_PARITY")
    if path and PARITY:
        with open(path, "w") as f:
            json.dump({"rule": "max|g - ref| / (max|ref| + 1e-3 max|J|) over all rows and states, per input group",
                       "bound": TOL, "worst": PARITY}, f, indent=1, sort_keys=True)


@functools.lru_cache(maxsize=None)
def case(name):
    """The model, its states, and per state the oracle's raw Jacobian and post-step qpos (computed once)."""
    if name == "tail":
        m, states = generic_model_and_states()
    else:
        m = mjx_amd.load_model(name)
        states = _states(m, 12, 2)
    o = Oracle(m)
    refs = []
    for st in states:
        J = o.step_jacobian(o.new_state(*st))
        refs.append((J, state_arrays(m, o.step(o.new_state(*st)))["qpos"]))
    return m, mjx.put_model(m), states, refs


def load(sys_, states, reps=1):
    d = mjx.make_data(sys_, len(states) * reps)
    t = lambda i: torch.tensor(np.array([s[i] for s in states] * reps), dtype=torch.float32)  # noqa: E731
    for k, i in (("qpos", 0), ("qvel", 1), ("qacc_warmstart", 2), ("ctrl", 3)):
        d.set(k, t(i))
    return d


def reference(m, states, refs, i, layout):
    J, qn = refs[i]
    return lr.tangent_AB(m, J, states[i][0], qn) if layout == "tangent" else lr.raw_AB(m, J)


def both(sys_, d, layout, **kw):
    if layout == "tangent":
        return mjx.transition(sys_, d, **kw)
    A, B = mjx._step_jacobian(sys_, d, kw.get("ctrl"), kw.get("mask"), kw.get("out"), 0, sys_.nq + sys_.nv)
    return A, B


def note(name, layout, what, errs):
    for k, g in enumerate(("qpos" if layout == "raw" else "dq", "qvel", "ctrl")):
        key = f"{name}/{layout}/{what}/{g}"
        PARITY[key] = max(PARITY.get(key, 0.0), float(errs[..., k].max()))
        print(f"{key}: worst {PARITY[key]:.3e} (bound {TOL:g})")


# 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["tangent", "raw"])
@pytest.mark.parametrize("name", MODELS)
def test_parity_with_oracle(name, layout):
    m, sys_, states, refs = case(name)
    d = load(sys_, states)
    A, B = (x.cpu().numpy().astype(np.float64) for x in both(sys_, d, layout))
    nin = m.nv if layout == "tangent" else m.nq
    assert A.shape == (len(states), nin + m.nv, nin + m.nv) and B.shape == (len(states), nin + m.nv, m.nu)
    errs = np.stack([lr.row_errors(A[i], B[i], *reference(m, states, refs, i, layout), nin) for i in range(len(states))])
    note(name, layout, "oracle", errs)
    assert np.isfinite(A).all() and np.isfinite(B).all()
    assert errs.max() <= TOL, f"relative row errors, worst per state (pos, qvel, ctrl):\n{errs.max(1)}"
    if layout == "raw":  # mjx.step_jacobian is the two outputs side by side, the oracle's column order
        Jg = mjx.step_jacobian(sys_, d).cpu().numpy()
        assert Jg.shape == (len(states), m.nq + m.nv, m.nq + m.nv + m.nu)
        assert np.array_equal(Jg, np.concatenate([A, B], 2).astype(np.float32))


# 2 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
def test_rows_agree_with_step_vjp(name):
    m, sys_, states, _ = case(name)
    d = load(sys_, states)
    n, nq, nv = len(states), m.nq, m.nv
    A, B = (x.cpu().numpy().astype(np.float64) for x in both(sys_, d, "raw"))
    eye = torch.eye(nq + nv, device="cuda")
    rA, rB = np.zeros_like(A), np.zeros_like(B)
    for i in range(nq + nv):
        u = eye[i].expand(n, -1)
        oq, ov, oc = mjx.step_vjp(sys_, d, u[:, :nq], u[:, nq:])
        rA[:, i, :nq], rA[:, i, nq:], rB[:, i] = oq.cpu().numpy(), ov.cpu().numpy(), oc.cpu().numpy()
    errs = np.stack([lr.row_errors(A[e], B[e], rA[e], rB[e], nq) for e in range(n)])
    note(name, "raw", "step_vjp", errs)
    assert errs.max() <= TOL, errs.max(1)


# 3 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["tangent", "raw"])
def test_row_groups_do_not_change_a_bit(layout):
    """A row's sweep does not depend on which wave ran it: forced to one group, to the most the host rule can choose
    (54 / 55 rows over 16 groups: the last groups are short or empty), to group counts whose last group is short (7:
    8 rows each, 6 left; 5: 11 each, 10 left), and left to the host rule at two env counts (12, and 146, where the
    rule's simds / nenv gives a count that does not divide the rows)."""
    m, sys_, states, _ = case("humanoid_mjx")
    d = load(sys_, states)
    d.set_option(abi.OPT_LINEARIZE_GROUPS, 1)
    A1, B1 = (x.clone() for x in both(sys_, d, layout))
    assert torch.isfinite(A1).all() and A1.abs().max() > 0
    for g in (MAX_GROUPS, 7, 5, 0):
        d.set_option(abi.OPT_LINEARIZE_GROUPS, g)
        A, B = both(sys_, d, layout)
        assert torch.equal(A, A1) and torch.equal(B, B1), g
    with pytest.raises(MjlError):
        d.set_option(abi.OPT_LINEARIZE_GROUPS, MAX_GROUPS + 1)
    big = load(sys_, states[:2] * 73)  # 146 envs
    A, B = both(sys_, big, layout)
    for e in range(146):
        assert torch.equal(A[e], A1[e % 2]) and torch.equal(B[e], B1[e % 2]), e


# 4 ------------------------------------------------------------------------------------------------------------------
def test_batch_is_untouched():
    m, sys_, states, _ = case("humanoid")
    d, fresh = load(sys_, states), load(sys_, states)
    mjx.forward(sys_, d)
    mjx.forward(sys_, fresh)
    fields = ("qpos", "qvel", "qacc_warmstart", "ctrl", "time", "qacc")
    keep = {f: d.get(f).clone() for f in fields}
    mjx.transition(sys_, d)
    mjx.step_jacobian(sys_, d)
    for f, t in keep.items():
        assert torch.equal(d.get(f), t), f
    mjx.step(sys_, d)
    mjx.step(sys_, fresh)
    for f in fields + ("xpos", "qfrc_constraint"):
        assert torch.equal(d.get(f), fresh.get(f)), f


# 5 ------------------------------------------------------------------------------------------------------------------
def test_ctrl_argument():
    m, sys_, states, _ = case("humanoid_mjx")
    d = load(sys_, states)
    A0, B0 = (x.clone() for x in mjx.transition(sys_, d))
    A1, B1 = mjx.transition(sys_, d, ctrl=d.get("ctrl"))
    assert torch.equal(A0, A1) and torch.equal(B0, B1)
    # another ctrl, some entries outside the motors' range (their columns of B are zero there): the oracle at it
    rng = np.random.default_rng(8)
    c2 = np.float32(rng.uniform(-1.3, 1.3, (len(states), m.nu)))
    stored = d.get("ctrl").clone()
    A2, B2 = (x.cpu().numpy().astype(np.float64) for x in mjx.transition(sys_, d, ctrl=torch.tensor(c2)))
    assert torch.equal(d.get("ctrl"), stored)
    o = Oracle(m)
    errs = []
    for i, (q, v, w, _) in enumerate(states):
        c = c2[i].astype(np.float64)
        J = o.step_jacobian(o.new_state(q, v, w, c))
        qn = state_arrays(m, o.step(o.new_state(q, v, w, c)))["qpos"]
        rA, rB = lr.tangent_AB(m, J, q, qn)
        errs.append(lr.row_errors(A2[i], B2[i], rA, rB, m.nv))
        clipped = np.abs(c) > 1.0
        assert clipped.any() or i > 0
        assert (B2[i][:, clipped] == 0).all()
    errs = np.stack(errs)
    note("humanoid_mjx", "tangent", "ctrl_arg", errs)
    assert errs.max() <= TOL, errs.max(1)
    with pytest.raises(MjlError):
        mjx.transition(sys_, d, ctrl=torch.zeros((len(states), m.nu + 1)))


# 6 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["tangent", "raw"])
def test_mask_and_partial_outputs(layout):
    m, sys_, states, _ = case("humanoid_mjx")
    d = load(sys_, states)
    n = len(states)
    A0, B0 = (x.clone() for x in both(sys_, d, layout))
    mask = torch.tensor([1.0, 0.0] * (n // 2), device="cuda")
    A = torch.full_like(A0, SENTINEL)
    B = torch.full_like(B0, SENTINEL)
    both(sys_, d, layout, mask=mask, out=(A, B))
    for t, t0 in ((A, A0), (B, B0)):
        assert (t[mask < 0.5] == SENTINEL).all()
        assert torch.equal(t[mask > 0.5], t0[mask > 0.5])
    a, b = both(sys_, d, layout, out=(torch.full_like(A0, SENTINEL), None))
    assert b is None and torch.equal(a, A0)
    a, b = both(sys_, d, layout, out=(None, torch.full_like(B0, SENTINEL)))
    assert a is None and torch.equal(b, B0)
    if layout == "tangent":
        fresh = mjx.transition(sys_, d, mask=mask)
        assert (fresh[0][mask < 0.5] == 0).all() and (fresh[1][mask < 0.5] == 0).all()
        for bad in ((None, None), (A0[:, :-1], B0), (A0, B0[:, :, :-1]), (A0.cpu(), B0), (A0, B0.double()), A0):
            with pytest.raises(MjlError):
                mjx.transition(sys_, d, out=bad)
    else:
        J = torch.full((n, m.nq + m.nv, m.nq + m.nv + m.nu), SENTINEL, device="cuda")
        mjx.step_jacobian(sys_, d, mask=mask, out=J)
        assert (J[mask < 0.5] == SENTINEL).all() and torch.equal(J[mask > 0.5], torch.cat([A0, B0], 2)[mask > 0.5])
        with pytest.raises(MjlError):
            mjx.step_jacobian(sys_, d, out=J[:, :, :-1])


# 7 ------------------------------------------------------------------------------------------------------------------
def test_refusals():
    m, sys_, states, _ = case("humanoid_mjx")
    d = load(sys_, states)
    n = len(states)
    A0, B0 = (x.clone() for x in mjx.transition(sys_, d))
    L, unsupported = lib(), 2
    P = lambda t: mjx._ptr(t)  # noqa: E731

    def refused(dd, msg):
        A, B = torch.full_like(A0, SENTINEL), torch.full_like(B0, SENTINEL)
        for flags in (abi.JAC_TANGENT, 0):
            assert L.mjl_step_jacobian(dd.handle, None, None, flags, P(A), P(B), mjx._stream()) == unsupported
            assert msg in L.mjl_last_error(), L.mjl_last_error()
        torch.cuda.synchronize()
        assert (A == SENTINEL).all() and (B == SENTINEL).all()
        with pytest.raises(MjlError):
            mjx.transition(sys_, dd)

    def works():
        A, B = mjx.transition(sys_, d)
        assert torch.equal(A, A0) and torch.equal(B, B0)

    xfrc = torch.zeros((n, m.nbody, 6), device="cuda")
    d.attach_applied(None, xfrc)
    refused(d, b"applied forces attached")
    d.detach_applied()
    works()
    qfrc = torch.zeros((n, m.nv), device="cuda")
    d.attach_applied(qfrc, None)
    refused(d, b"applied forces attached")
    d.detach_applied()
    works()
    d.enable_model_params(True)
    refused(d, b"per-env model")
    d.enable_model_params(False)
    works()
    pd = actuators.pd_actuators(m, kp=40.0, kv=2.0)
    dpd = load(mjx.put_model(pd), states)
    refused(dpd, b"general actuators are not differentiated")
    works()


# 8 ------------------------------------------------------------------------------------------------------------------
def test_env_transition_captured_with_an_env_step():
    m, sys_, _, _ = case("humanoid_mjx")
    B = 8
    cfg = resolve_ids(m, dataclasses.replace(reference_ppo_config().env_config, max_episode_steps=1000))
    act = torch.tensor(np.random.default_rng(2).uniform(-1, 1, (B, m.nu)), dtype=torch.float32, device="cuda")

    def make():
        env = HumanoidEnv(sys_, cfg, B, seed=11)
        env.reset(counter=1)
        return env
    env = make()
    eager = []
    for i in range(2):
        env.step(act, auto_reset=False, counter=2 + i)
        eager.append([t.clone() for t in env.transition()])
    assert not torch.equal(eager[0][0], eager[1][0])
    # the env linearises mjx.step at the stored ctrl: the free function on the env's batch gives the same matrices
    for t, want in zip(mjx.transition(sys_, env.data), eager[1]):
        assert torch.equal(t, want)
    env = make()
    bufs = env.transition()  # the eager call: allocates the scratch and the env's tensors
    assert env.transition()[0] is bufs[0]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.step(act, auto_reset=False, counter=2)
        env.transition()
    for i in range(2):
        g.replay()
        torch.cuda.synchronize()
        for k, want in enumerate(eager[i]):
            assert torch.equal(bufs[k], want), (i, k)
    env2 = HumanoidEnv(sys_, cfg, B, seed=11, n_frames=2)
    with pytest.raises(MjlError):
        env2.transition()
