"""Applied forces on the GPU (mjl_batch_attach_applied, mjl_env_push) against the fp64 oracle.

The oracle has no applied-force input; three routes tie the new term to physics it already verifies:
  J' against fp64      qacc_smooth = oracle qacc_smooth + solve(M, qfrc_applied + sum_b jacp_b' f_b + jacr_b' t_b),
                       M from the oracle, the Jacobians from mjcf.body_jacobian at xipos
  gravity equivalence  xfrc_applied[b] = (-mass_b g, 0) on every body = the model with gravity zeroed
  motor equivalence    qfrc_applied[dof_u] = gear_u c_u with ctrl = 0 = motors driven with ctrl = c
States, loader and tolerances are tests/test_gpu_parity.py's (its header): qfrc_bias / passive / actuator
2e-5 * s, qacc_smooth / qacc / qfrc_constraint / qvel / qacc_warmstart 2e-3 * s, qpos atol 2e-5, counts exact."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import mjx_amd
from mjx_amd import abi, mjcf, mjx, ppo
from mjx_amd._header import HEADER
from mjx_amd._lib import MjlError, lib
from mjx_amd.config import reference_ppo_config
from mjx_amd.envs import HumanoidEnv, resolve_ids
from mjx_amd.mjx import _ptr, _stream
from oracle import Oracle, state_arrays

from applied_ref import push_step, push_uniforms
from test_gpu_parity import _close, _load, _states

pytestmark = pytest.mark.gpu

MODELS = ["humanoid_mjx", "humanoid"]
UNSUPPORTED = HEADER.enums["MJL_ERR_UNSUPPORTED"]
STATE = ("qpos", "qvel", "qacc_warmstart", "ctrl", "time", "qacc", "xpos", "xquat", "sensordata", "qfrc_actuator",
         "qfrc_bias", "qfrc_passive", "qfrc_constraint", "qacc_smooth", "stats")


def _dev(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device="cuda").contiguous()


@pytest.fixture(scope="module", params=MODELS)
def setup(request):
    """Model, states, and per state the oracle's unperturbed forward pass plus the fp64 Jacobians
    [nbody, 6, nv] (rows: jacp, jacr) of every body at its xipos; computed once, read by every test."""
    m = mjx_amd.load_model(request.param)
    states = _states(m)
    orc = Oracle(m)
    base, jac = [], []
    for q, v, w, c in states:
        a = state_arrays(m, orc.forward(orc.new_state(q, v, w, c)))
        kin = mjcf._fk_and_mass(m, q)
        np.testing.assert_allclose(kin["xipos"], a["xipos"], atol=1e-9)
        J = np.zeros((m.nbody, 6, m.nv))
        for b in range(1, m.nbody):
            J[b, :3], J[b, 3:] = mjcf.body_jacobian(m, kin, b, kin["xipos"][b])
        base.append(a)
        jac.append(J)
    return m, mjx.put_model(m), states, base, jac, request.param


def _forward_fields(sys_, states, qfrc=None, xfrc=None, fields=("qacc_smooth", "qfrc_bias", "qfrc_passive",
                                                              "qfrc_actuator")):
    d = _load(sys_, states)
    d.attach_applied(qfrc, xfrc)
    mjx.forward(sys_, d)
    return {f: d.get(f).cpu().numpy() for f in fields}


def _check_jt(m, base, jac, G, qfrc, xfrc, what):
    for i, (a, J) in enumerate(zip(base, jac)):
        gen = np.float64(qfrc[i]) + np.einsum("bkv,bk->v", J[1:], np.float64(xfrc[i][1:]))
        _close(G["qacc_smooth"][i], a["qacc_smooth"] + np.linalg.solve(a["M"], gen), 2e-3, f"{what} state {i} qacc_smooth")
        for f in ("qfrc_bias", "qfrc_passive", "qfrc_actuator"):
            _close(G[f][i], a[f], 2e-5, f"{what} state {i} {f}")


def _random_forces(m, n, seed):
    rng = np.random.default_rng(seed)
    xfrc = np.concatenate([rng.uniform(-50, 50, (n, m.nbody, 3)), rng.uniform(-10, 10, (n, m.nbody, 3))], 2)
    xfrc[:, 0] = 0
    return np.float32(rng.uniform(-10, 10, (n, m.nv))), np.float32(xfrc)


def test_jt_against_fp64_all_bodies(setup):
    m, sys_, states, base, jac, _ = setup
    qfrc, xfrc = _random_forces(m, len(states), 1)
    G = _forward_fields(sys_, states, _dev(qfrc), _dev(xfrc))
    _check_jt(m, base, jac, G, qfrc, xfrc, "all bodies")
    # either buffer may be absent
    _check_jt(m, base, jac, _forward_fields(sys_, states, None, _dev(xfrc)), 0 * qfrc, xfrc, "xfrc only")
    _check_jt(m, base, jac, _forward_fields(sys_, states, _dev(qfrc), None), qfrc, 0 * xfrc, "qfrc only")
    # row 0 (the world body) is ignored: bit for bit the result with a zero row
    x0 = xfrc.copy()
    x0[:, 0] = (40, -30, 20, 5, -6, 7)
    G0 = _forward_fields(sys_, states, _dev(qfrc), _dev(x0))
    for f in G:
        np.testing.assert_array_equal(G0[f], G[f])


def test_jt_against_fp64_one_body_at_a_time(setup):
    """A wrong ancestor walk or subtree range cannot cancel out when a single body carries the wrench."""
    m, sys_, states, base, jac, _ = setup
    _, full = _random_forces(m, len(states), 2)
    zero = np.zeros((len(states), m.nv), np.float32)
    for b in range(1, m.nbody):
        xfrc = np.zeros_like(full)
        xfrc[:, b] = full[:, b]
        _check_jt(m, base, jac, _forward_fields(sys_, states, None, _dev(xfrc)), zero, xfrc, f"body {b}")


def _check_dynamics(m, sys_, states, orc, octrl, gstates, qfrc, xfrc, actuator_zero):
    """Forward (qacc, qfrc_constraint, counts) and step (qpos, qvel, qacc_warmstart) of the GPU with the
    applied forces against the oracle `orc` driven with controls `octrl`."""
    d = _load(sys_, gstates)
    d.attach_applied(qfrc, xfrc)
    mjx.forward(sys_, d)
    G = {f: d.get(f).cpu().numpy() for f in ("qacc", "qfrc_constraint", "qfrc_actuator", "stats")}
    for i, (q, v, w, _) in enumerate(states):
        a = state_arrays(m, orc.forward(orc.new_state(q, v, w, octrl[i])))
        assert (G["stats"][i][0], G["stats"][i][1]) == (a["ncon"], a["nefc"]), f"state {i}: contact/row counts"
        for f in ("qacc", "qfrc_constraint"):
            _close(G[f][i], a[f], 2e-3, f"state {i} {f}")
        if actuator_zero:
            assert not G["qfrc_actuator"][i].any()
    d = _load(sys_, gstates)
    d.attach_applied(qfrc, xfrc)
    mjx.step(sys_, d)
    q1, v1, w1 = (d.get(f).cpu().numpy() for f in ("qpos", "qvel", "qacc_warmstart"))
    for i, (q, v, w, _) in enumerate(states):
        a = state_arrays(m, orc.step(orc.new_state(q, v, w, octrl[i])))
        np.testing.assert_allclose(q1[i], a["qpos"], atol=2e-5)
        _close(v1[i], a["qvel"], 2e-3, f"state {i} qvel")
        _close(w1[i], a["qacc_warmstart"], 2e-3, f"state {i} qacc_warmstart")


def test_gravity_equivalence(setup):
    """-mass_b g on every body's centre of mass is the model without gravity, contacts included."""
    m, sys_, states, base, _, name = setup
    m0 = mjx_amd.load_model(name)
    m0.gravity = np.zeros(3)
    xfrc = np.zeros((len(states), m.nbody, 6), np.float32)
    xfrc[:, 1:, :3] = -np.asarray(m.body_mass)[None, 1:, None] * np.asarray(m.gravity)[None, None, :]
    _check_dynamics(m, sys_, states, Oracle(m0), [s[3] for s in states], states, None, _dev(xfrc), False)


def test_motor_equivalence(setup):
    """gear_u c_u applied on the actuated dof with ctrl = 0 is the motor driven with ctrl = c."""
    m, sys_, states, base, _, name = setup
    dof = np.asarray(m.jnt_dofadr)[np.asarray(m.actuator_trnid)]
    qfrc = np.zeros((len(states), m.nv))
    for i, st in enumerate(states):
        np.add.at(qfrc[i], dof, np.asarray(m.actuator_gear) * st[3])
        np.testing.assert_allclose(base[i]["qfrc_actuator"], qfrc[i], rtol=0, atol=1e-9)  # the oracle's motors
    gstates = [(q, v, w, np.zeros(m.nu)) for q, v, w, _ in states]
    _check_dynamics(m, sys_, states, Oracle(m), [s[3] for s in states], gstates, _dev(qfrc), None, True)


# ------------------------------------------------------------------------------------------------ pinned to the base path
def _fields(d):
    return [d.get(f).cpu().numpy() for f in STATE]


def test_zero_buffers_and_detach_are_the_base_step(setup):
    m, sys_, states, base, _, name = setup
    n = len(states)
    ref, d = _load(sys_, states), _load(sys_, states)
    for dd in (ref, d):
        dd.set_option(abi.OPT_STORE_DERIVED, 1)
    d.attach_applied(torch.zeros((n, m.nv), device="cuda"), torch.zeros((n, m.nbody, 6), device="cuda"))
    mjx.step(sys_, ref)
    mjx.step(sys_, d)
    for f, a, b in zip(STATE, _fields(ref), _fields(d)):
        np.testing.assert_array_equal(a, b, err_msg=f"zero buffers: {f}")
    d.detach_applied()
    mjx.step(sys_, ref)
    mjx.step(sys_, d)
    for f, a, b in zip(STATE, _fields(ref), _fields(d)):
        np.testing.assert_array_equal(a, b, err_msg=f"detached: {f}")


def _env(name, B, seed=3, max_steps=None):
    m = mjx_amd.load_model(name)
    ecfg = reference_ppo_config().env_config
    if max_steps is not None:
        ecfg = dataclasses.replace(ecfg, max_episode_steps=max_steps)
    return m, HumanoidEnv(mjx.put_model(m), resolve_ids(m, ecfg), B, seed=seed, store_derived=True)


@pytest.mark.parametrize("name", MODELS)
def test_zero_buffers_and_detach_are_the_base_env_step(name):
    """Auto-reset on, episodes of 3 steps: every env resets (in place) twice within the 7 steps."""
    B = 40
    m, ref = _env(name, B, max_steps=3)
    _, env = _env(name, B, max_steps=3)
    env.attach_applied(torch.zeros((B, m.nv), device="cuda"), torch.zeros((B, m.nbody, 6), device="cuda"))
    g = torch.Generator().manual_seed(1)
    resets = 0
    for e in (ref, env):
        e.reset()
    for t in range(7):
        if t == 4:
            env.attach_applied(None, None)
        act = (torch.rand((B, m.nu), generator=g) * 2 - 1).cuda()
        a, b = [x.clone() for x in ref.step(act)], [x.clone() for x in env.step(act)]
        for what, x, y in zip(("obs", "rew", "term", "trunc"), a, b):
            assert torch.equal(x, y), f"step {t}: {what}"
        assert torch.equal(ref.get_state(), env.get_state()), f"step {t}: state"
        resets += int(torch.maximum(a[2], a[3]).sum())
    assert resets >= 2 * B


def test_global_rows_bit_identical_with_forces(setup):
    m, sys_, states, base, _, name = setup
    qfrc, xfrc = _random_forces(m, len(states), 3)
    res = []
    for force in (0, 1):
        d = _load(sys_, states)
        d.set_option(abi.OPT_FORCE_GLOBAL_ROWS, force)
        d.attach_applied(_dev(qfrc), _dev(xfrc))
        mjx.step(sys_, d)
        res.append([d.get(f).cpu().numpy() for f in ("qpos", "qvel", "qacc", "sensordata")])
    for a, b in zip(*res):
        np.testing.assert_array_equal(a, b)
    base = _load(sys_, states)
    mjx.step(sys_, base)
    assert not np.array_equal(base.get("qvel").cpu().numpy(), res[0][1])  # the forces did act


# ------------------------------------------------------------------------------------------------ scope
def _big(m, B):
    return torch.full((B, m.nbody, 6), 1000.0, device="cuda")


def test_resets_pool_and_speedtest_ignore_attached_forces():
    B = 32
    m, ref = _env("humanoid_mjx", B, max_steps=1)
    _, env = _env("humanoid_mjx", B, max_steps=1)
    env.attach_applied(None, _big(m, B))
    assert torch.equal(ref.reset().clone(), env.reset().clone())
    assert torch.equal(ref.get_state(), env.get_state())
    # every step finishes (max_episode_steps 1) and merges a pooled reset: the post-step state and obs are the
    # pool's, so they are equal exactly when the pooled resets are; the third step resets in place
    for e in (ref, env):
        e.enable_reset_pool(2)
        e.fill_reset_pool(torch.tensor([2], dtype=torch.int32, device="cuda"))
    act = torch.zeros((B, m.nu), device="cuda")
    for t in range(3):
        a, b = ref.step(act)[0].clone(), env.step(act)[0].clone()
        assert torch.equal(a, b), f"step {t}: reset obs"
        assert torch.equal(ref.get_state(), env.get_state()), f"step {t}: reset state"
    vel = torch.linspace(0, 1, B, device="cuda")
    assert torch.equal(mjx.speedtest_step(ref.sys, ref.data, vel), mjx.speedtest_step(env.sys, env.data, vel))
    assert float(env.xfrc_applied.min()) == 1000.0  # an input: no reset or step cleared or wrote it


def test_masked_forward_leaves_masked_envs_untouched(setup):
    m, sys_, states, base, _, name = setup
    n = len(states)
    d = _load(sys_, states)
    d.attach_applied(None, _big(m, n))
    before = d.get("qacc").cpu().numpy()
    mask = torch.tensor([1.0, 0.0] * (n // 2) + [1.0] * (n % 2), device="cuda")
    mjx.forward(sys_, d, mask)
    after = d.get("qacc").cpu().numpy()
    keep = mask.cpu().numpy() < 0.5
    np.testing.assert_array_equal(after[keep], before[keep])
    assert np.abs(after[~keep]).max() > 0


def test_vjp_entries_are_unsupported_while_attached():
    B = 4
    m, env = _env("humanoid_mjx", B)
    env.reset()
    env.data.set_option(abi.OPT_VJP_TAPE, 1)
    L, h, s = lib(), env.data.handle, _stream()
    f = lambda *shape: torch.zeros(shape, device="cuda")  # noqa: E731
    act, gq, gv, gw, gr, ga = f(B, m.nu), f(B, m.nq), f(B, m.nv), f(B, m.nv), f(B), f(B, abi.AUX_DIM)
    oq, ov, ow, oa, oaux, oc = f(B, m.nq), f(B, m.nv), f(B, m.nv), f(B, m.nu), f(B, abi.AUX_DIM), f(B, m.nu)
    p = _ptr
    io = (p(env.obs), p(env.rew), p(env.term), p(env.trunc))
    nul = (None,) * 32
    calls = {
        "mjl_step_vjp": lambda: L.mjl_step_vjp(h, p(gq), p(gv), p(oq), p(ov), p(oc), s),
        "mjl_step_vjp_full": lambda: L.mjl_step_vjp_full(h, p(gq), p(gv), p(gw), p(oq), p(ov), p(ow), p(oc), s),
        "mjl_env_step_vjp": lambda: L.mjl_env_step_vjp(h, p(act), p(gq), p(gv), p(gr), p(ga), p(oq), p(ov), p(oa),
                                                       p(oaux), s),
        "mjl_env_step_vjp_guarded": lambda: L.mjl_env_step_vjp_guarded(h, p(act), p(gq), p(gv), p(gr), p(ga), p(oq),
                                                                       p(ov), p(oa), p(oaux), None, s),
        "mjl_env_step_vjp_full": lambda: L.mjl_env_step_vjp_full(h, p(act), p(gq), p(gv), p(gw), p(gr), p(ga), p(oq),
                                                                 p(ov), p(ow), p(oa), p(oaux), None, s),
        "mjl_env_step_record": lambda: L.mjl_env_step_record(h, 0, p(act), *io, s),
        "mjl_env_step_vjp_replay": lambda: L.mjl_env_step_vjp_replay(h, 0, p(act), p(gq), p(gv), p(gw), p(gr), p(ga),
                                                                     p(oq), p(ov), p(ow), p(oa), p(oaux), None, s),
    }
    # the entries with a policy / APG tail: refused before any other argument is looked at
    refused_only = {
        "mjl_env_step_record_apg": lambda: L.mjl_env_step_record_apg(h, 0, *nul[:5], 0.99, 1e3, *nul[:6], s),
        "mjl_env_step_record_apg_next": lambda: L.mjl_env_step_record_apg_next(h, 0, *nul[:5], 0.99, 1e3, *nul[:8], 0,
                                                                               *nul[:3], 0, *nul[:4], s),
        "mjl_env_step_vjp_replay_apg": lambda: L.mjl_env_step_vjp_replay_apg(h, 0, *nul[:12], 0, *nul[:7], 0, s),
    }
    named = [n for n in lib_exports() if any(k in n for k in ("step_vjp", "step_record"))]
    assert sorted(named) == sorted(list(calls) + list(refused_only)), "an entry of the VJP family is not covered"
    env.attach_applied(torch.zeros((B, m.nv), device="cuda"), None)
    for name, call in {**calls, **refused_only}.items():
        assert call() == UNSUPPORTED, name
        assert b"applied forces" in L.mjl_last_error()
    with pytest.raises(MjlError, match="applied forces"):  # the wrappers raise the library's exception
        env.step_vjp(act, gq, gv, gr)
    with pytest.raises(MjlError, match="applied forces"):
        mjx.step_vjp(env.sys, env.data, gq, gv)
    env.attach_applied(None, None)
    for name in ("mjl_step_vjp", "mjl_step_vjp_full", "mjl_env_step_vjp", "mjl_env_step_vjp_guarded",
                 "mjl_env_step_vjp_full", "mjl_env_step_record", "mjl_env_step_vjp_replay"):
        assert calls[name]() == 0, (name, L.mjl_last_error())
    torch.cuda.synchronize()


def lib_exports():
    from mjx_amd import _lib
    return _lib.EXPORTS


# ------------------------------------------------------------------------------------------------ push kernel
def _push_env(B=8, seed=0x5EED5EED1234):
    m, env = _env("humanoid_mjx", B, seed=seed)
    xfrc = torch.zeros((B, m.nbody, 6), device="cuda")
    env.attach_applied(None, xfrc)
    return m, env, xfrc


def test_push_with_explicit_noise_matches_the_restatement():
    B, body, interval, duration, force = 8, 3, (3, 5), 2, (50.0, 150.0)
    m, env, xfrc = _push_env(B)
    rng = np.random.default_rng(4)
    timer, row = np.zeros((B, 2), np.int32), np.zeros((B, 6), np.float32)
    pushed = 0
    for t in range(40):
        u = rng.uniform(0, 1, (B, 3)).astype(np.float32)
        done = (rng.uniform(0, 1, B) < 0.3).astype(np.float32) if t % 4 == 3 else None
        env.push(body, interval, duration, force, None if done is None else _dev(done), _dev(u))
        push_step(timer, row, u, done, interval, duration, force)
        np.testing.assert_array_equal(env.push_timer.cpu().numpy(), timer, err_msg=f"call {t}")
        x = xfrc.cpu().numpy()
        np.testing.assert_allclose(x[:, body], row, rtol=1e-6, atol=0, err_msg=f"call {t}")
        assert not np.delete(x, body, axis=1).any(), "a row other than `body` was written"
        pushed += int((np.abs(row).sum(1) > 0).sum())
    assert pushed > 20


def test_push_device_draws_follow_the_librarys_generator():
    B, body, interval, duration, force = 8, 1, (3, 5), 2, (50.0, 150.0)
    m, env, xfrc = _push_env(B)
    timer, row = np.zeros((B, 2), np.int32), np.zeros((B, 6), np.float32)
    for t in range(12):
        c = 100 + t
        before_t, before_x = env.push_timer.clone(), xfrc.clone()
        env.push(body, interval, duration, force, counter=c)
        got_t, got_x = env.push_timer.clone(), xfrc.clone()
        env.push_timer.copy_(before_t)
        xfrc.copy_(before_x)
        env.push(body, interval, duration, force, counter=c)  # the same (seed, counter) again: the same output
        assert torch.equal(env.push_timer, got_t) and torch.equal(xfrc, got_x)
        push_step(timer, row, push_uniforms(env.seed, c, B), None, interval, duration, force)
        np.testing.assert_array_equal(got_t.cpu().numpy(), timer)
        np.testing.assert_allclose(got_x.cpu().numpy()[:, body], row, rtol=1e-6, atol=0)
        assert not np.delete(got_x.cpu().numpy(), body, axis=1).any()
    # the attached counter base joins the counter: base b with counter c draws as counter b + c
    env.push_timer.zero_()
    xfrc.zero_()
    env.ctr_base.fill_(1000)
    env.push(body, interval, duration, force, counter=7)
    shifted = xfrc.clone()
    t2, r2 = np.zeros((B, 2), np.int32), np.zeros((B, 6), np.float32)
    push_step(t2, r2, push_uniforms(env.seed, 1007, B), None, interval, duration, force)
    np.testing.assert_allclose(shifted.cpu().numpy()[:, body], r2, rtol=1e-6, atol=0)
    env.ctr_base.zero_()
    env.push_timer.zero_()
    xfrc.zero_()
    env.push(body, interval, duration, force, counter=7)
    assert not torch.equal(xfrc, shifted)


def test_push_argument_errors():
    m, env, xfrc = _push_env(4)
    ok = dict(body=1, interval=(1, 1), duration=1, force=(1.0, 2.0))
    env.push(**ok)
    for bad in (dict(body=0), dict(body=m.nbody), dict(interval=(0, 3)), dict(interval=(4, 3)), dict(duration=0)):
        with pytest.raises(MjlError, match="error 1 "):
            env.push(**{**ok, **bad})
    L = lib()
    assert L.mjl_env_push(env.data.handle, 1, None, 1, 1, 1, 1.0, 2.0, None, 0, 0, None, _stream()) == HEADER.enums["MJL_ERR_ARG"]
    env.data.attach_applied(torch.zeros((4, m.nv), device="cuda"), None)  # no xfrc_applied attached
    assert L.mjl_env_push(env.data.handle, 1, C.c_void_p(env.push_timer.data_ptr()), 1, 1, 1, 1.0, 2.0, None, 0, 0, None,
                          _stream()) == HEADER.enums["MJL_ERR_ARG"]


def test_captured_push_and_step_replay_equals_eager():
    """Five replays of one captured (push, env step) pair, the counter base advanced between them, are the
    eager sequence bit for bit (pushes of 300..600 N on the torso, so the steps do differ from unpushed ones)."""
    B, body, interval, duration, force = 64, 1, (1, 2), 2, (300.0, 600.0)
    runs = []
    for captured in (False, True):
        m, env, xfrc = _push_env(B, seed=77)
        env.reset()
        act = torch.zeros((B, m.nu), device="cuda")
        done = torch.zeros(B, device="cuda")
        out = []

        def pair(counter):
            env.push(body, interval, duration, force, done=done, counter=counter)
            env.step(act, counter=counter)
            torch.maximum(env.term, env.trunc, out=done)

        if captured:
            env.ctr_base.fill_(1)
            pair(1)  # eager first: loads the code objects outside the capture
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with ppo.graph_capture(graph):
                pair(1)
        for k in range(6):
            if not captured:
                pair(k + 2)
            elif k > 0:
                env.ctr_base.fill_(k + 1)
                graph.replay()
            else:
                continue
            out.append([x.clone() for x in (env.obs, env.rew, env.term, env.trunc, env.get_state(), xfrc,
                                            env.push_timer)])
        runs.append(out)
    eager, replay = runs[0][1:], runs[1]  # eager call k + 2 = base k + 1 with counter 1
    assert len(eager) == len(replay) == 5
    for k, (a, b) in enumerate(zip(eager, replay)):
        for x, y in zip(a, b):
            assert torch.equal(x, y), f"replay {k}"
    assert any(float(a[5].abs().sum()) > 0 for a in eager)


# ------------------------------------------------------------------------------------------------ trainer
def _trainer(push, seed=11):
    m = mjx_amd.load_model("humanoid_mjx")
    cfg = reference_ppo_config()
    cfg.num_envs, cfg.rollout_length, cfg.minibatch_size, cfg.epochs, cfg.seed = 64, 8, 128, 1, 5
    env = HumanoidEnv(mjx.put_model(m), resolve_ids(m, cfg.env_config), cfg.num_envs, seed=seed)
    return ppo.PPOTrainer(cfg, env, None, device="cuda", push=push), env


def test_trainer_with_pushes_and_without():
    """Two iterations (the second replays the captured rollout) with pushes: finite, and a push is live at
    some step. Without `push` the trainer attaches nothing and launches nothing new."""
    body = resolve_ids(mjx_amd.load_model("humanoid_mjx"), reference_ppo_config().env_config).pelvis_body_id
    tr, env = _trainer({"body": body, "interval": (2, 4), "duration": 2, "force": (100.0, 300.0)})
    live = 0
    for it in range(2):
        met = tr.iteration(it)
        assert all(np.isfinite(v) for v in met.values()), met
        assert torch.isfinite(tr.obs).all()
        live += int((tr.push_xfrc[:, body].abs().sum(1) > 0).sum())
        assert not np.delete(tr.push_xfrc.cpu().numpy(), body, axis=1).any()
    assert live > 0
    plain, penv = _trainer(None)
    assert plain.push is None and getattr(penv, "xfrc_applied", None) is None and not hasattr(penv, "push_timer")
    assert getattr(penv.data, "_applied", None) is None
    ref, _ = _trainer(None)
    for it in range(2):
        a, b = plain.iteration(it), ref.iteration(it)
        assert {k: v for k, v in a.items() if k != "env_steps_per_sec"} == \
            {k: v for k, v in b.items() if k != "env_steps_per_sec"}
        assert torch.equal(plain.obs, ref.obs)
