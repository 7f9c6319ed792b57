"""General actuators on the GPU against the fp64 oracle, which has motors only: the feature is tied to physics
the oracle verifies through the exact equivalences of tests/actuators_ref.py (forces in float64; a motor model
driven with ctrl' = F, and under implicitfast with the actuators' velocity derivative moved into dof_damping).
States, loader and tolerances are tests/test_gpu_parity.py's: qfrc_* 2e-5 * s, qacc*, qvel, qacc_warmstart
2e-3 * s, qpos atol 2e-5, counts exact."""
import dataclasses

import numpy as np
import pytest
import torch

import mjx_amd
from mjx_amd import abi, mjx
from mjx_amd._header import HEADER
from mjx_amd._lib import MjlError, lib
from mjx_amd.actuators import pd_actuators
from mjx_amd.config import reference_ppo_config
from mjx_amd.envs import HumanoidEnv, resolve_ids
from mjx_amd.mjx import _ptr, _stream
from oracle import Oracle, state_arrays

import actuators_ref as ar
from test_gpu_parity import _close, _load, _states
from test_reset_pool import STATE as RESET_STATE, _reset_at, slot_counter

pytestmark = pytest.mark.gpu

UNSUPPORTED = HEADER.enums["MJL_ERR_UNSUPPORTED"]
KP, KV = 20.0, 1.5
FIELDS = ("qpos", "qvel", "qacc_warmstart", "qacc", "qacc_smooth", "qfrc_actuator", "qfrc_bias", "qfrc_passive",
          "qfrc_constraint", "stats", "sensordata", "xpos")


@pytest.fixture(scope="module", params=ar.MODELS)
def base(request):
    m = mjx_amd.load_model(request.param)
    return request.param, m, _states(m, n_random=6)


def _gpu(g, states, step):
    sys_ = mjx.put_model(g)
    d = _load(sys_, states)
    (mjx.step if step else mjx.forward)(sys_, d)
    return {f: d.get(f).cpu().numpy() for f in FIELDS}


def _check_forward(g, states, what):
    G = _gpu(g, states, step=False)
    M = _gpu(ar.motor_model(g, False), [(q, v, w, ar.motor_ctrl(g, q, v, c, False)) for q, v, w, c in states], step=False)
    orc = Oracle(ar.motor_model(g, False))
    for i, (q, v, w, c) in enumerate(states):
        _, _, qfrc = ar.forces(g, q, v, c)
        _close(G["qfrc_actuator"][i], qfrc, 2e-5, f"{what} state {i} qfrc_actuator")
        a = state_arrays(g, orc.forward(orc.new_state(q, v, w, ar.motor_ctrl(g, q, v, c, False))))
        assert (G["stats"][i][0], G["stats"][i][1]) == (a["ncon"], a["nefc"]), f"{what} state {i}: contact/row counts"
        for f in ("qacc", "qacc_smooth", "qfrc_constraint"):
            _close(G[f][i], a[f], 2e-3, f"{what} state {i} {f}")
    for f in ("qfrc_bias", "qfrc_passive"):  # unchanged from the motor model
        np.testing.assert_array_equal(G[f], M[f], err_msg=f"{what} {f}")


def _check_step(g, states, what):
    implicit = g.integrator == ar.INTEGRATORS["implicitfast"]
    G = _gpu(g, states, step=True)
    orc = Oracle(ar.motor_model(g, implicit))
    for i, (q, v, w, c) in enumerate(states):
        a = state_arrays(g, orc.step(orc.new_state(q, v, w, ar.motor_ctrl(g, q, v, c, implicit))))
        np.testing.assert_allclose(G["qpos"][i], a["qpos"], atol=2e-5, err_msg=f"{what} state {i}")
        _close(G["qvel"][i], a["qvel"], 2e-3, f"{what} state {i} qvel")
        _close(G["qacc_warmstart"][i], a["qacc_warmstart"], 2e-3, f"{what} state {i} qacc_warmstart")


# 1, 2, 3 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("integrator", list(ar.INTEGRATORS))
def test_forward_and_one_step(base, integrator):
    name, m, states = base
    g = ar.general_model(m, KP, KV, seed=1, integrator=integrator)
    _check_forward(g, states, f"{name} {integrator}")
    _check_step(g, states, f"{name} {integrator}")
    moved = _gpu(ar.with_arrays(m, integrator), states, step=True)["qvel"]
    assert not np.array_equal(moved, _gpu(g, states, step=True)["qvel"])  # the actuators did act


def test_implicitfast_without_damping_and_without_velocity_term(base):
    """dof_damping all 0 with b2 != 0: the matrix still gets the actuators' term (the damping flag of the block
    is off). b2 = 0: pure stiffness, nothing joins the matrix."""
    name, m, states = base
    _check_step(ar.general_model(m, KP, KV, seed=2, integrator="implicitfast", damping=0.0), states, f"{name} undamped")
    _check_step(ar.general_model(m, KP, 0.0, seed=3, integrator="implicitfast"), states, f"{name} stiffness only")
    _check_step(ar.general_model(m, KP, 0.0, seed=3, integrator="implicitfast", damping=0.0), states, f"{name} neither")
    # Euler takes the damping alone, also with eulerdamp on and every dof_damping 0
    e = dataclasses.replace(ar.general_model(m, KP, KV, seed=2, integrator="euler", damping=0.0), eulerdamp=1)
    _check_step(e, states, f"{name} euler undamped")


# 4 ---------------------------------------------------------------------------------------------------------------
def test_force_clamp_and_the_derivative_that_ignores_it(base):
    name, m, states = base
    g = ar.general_model(m, KP, KV, seed=4, integrator="implicitfast", forcerange=0.35)
    for i, (q, v, w, c) in enumerate(states):
        F, raw, _ = ar.forces(g, q, v, c)
        assert (F != raw).any() and (F == raw).any(), f"state {i}: needs clamped and unclamped actuators"
    _check_forward(g, states, f"{name} clamp")
    _check_step(g, states, f"{name} clamp")  # damping' carries every actuator's gear^2 b2, clamped or not


# 5 ---------------------------------------------------------------------------------------------------------------
def test_two_actuators_on_one_dof(base):
    name, m, states = base
    rng = np.random.default_rng(9)
    ext = [(q, v, w, np.concatenate([c, np.float64(np.float32(rng.uniform(-1, 1, 3)))])) for q, v, w, c in states]
    for integrator in ar.INTEGRATORS:
        g = ar.general_model(m, KP, KV, seed=5, integrator=integrator, extra_velocity=3)
        assert g.nu == m.nu + 3 <= abi.MAXU and len(set(g.actuator_trnid)) == m.nu
        _check_forward(g, ext, f"{name} {integrator} two per dof")
        _check_step(g, ext, f"{name} {integrator} two per dof")


# 6 ---------------------------------------------------------------------------------------------------------------
def test_carried_rollout():
    """Ten carried steps from the standing keyframe with random targets on the PD humanoid (implicitfast, force
    clamp on): the GPU against the oracle stepped one step at a time, ctrl' recomputed from the oracle's own
    state. Tolerance of test_gpu_parity.test_trajectory_parity, which carries 20 steps: qpos atol 1e-3.
    Observed on an MI355X: worst |qpos - oracle| 5.1e-7."""
    m = mjx_amd.load_model("humanoid_mjx")
    g = pd_actuators(m, 30.0, 2.0, 0.5)
    sys_ = mjx.put_model(g)
    rng = np.random.default_rng(5)
    B, T = 8, 10
    ctrl = rng.uniform(-1, 1, (T, B, g.nu)).astype(np.float32)
    d = mjx.make_data(sys_, B)
    for t in range(T):
        mjx.step(sys_, d, torch.tensor(ctrl[t], device="cuda"))
    q = d.get("qpos").cpu().numpy()
    orc = Oracle(ar.motor_model(g, True))
    worst = 0.0
    for i in range(B):
        a = state_arrays(g, orc.new_state())
        for t in range(T):
            c = ar.motor_ctrl(g, a["qpos"], a["qvel"], ctrl[t, i].astype(np.float64), True)
            a = state_arrays(g, orc.step(orc.new_state(a["qpos"], a["qvel"], a["qacc_warmstart"], c)))
        worst = max(worst, np.abs(q[i] - a["qpos"]).max())
        np.testing.assert_allclose(q[i], a["qpos"], atol=1e-3)
    print(f"carried rollout: worst |qpos - oracle| {worst:.3e}")
    assert np.abs(q - np.asarray(g.qpos0)).max() > 1e-2  # it moved


# 7 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("integrator", list(ar.INTEGRATORS))
def test_motor_written_as_general_actuator(base, integrator):
    name, m, states = base
    mm = ar.with_arrays(m, integrator)
    nu = m.nu
    g = ar.with_arrays(mm, **ar.general_actuator_arrays(np.ones(nu, np.int32), np.ones(nu), np.zeros((nu, 3)),
                                                         np.zeros(nu, np.int32), np.zeros((nu, 2))))
    for step in (False, True):
        G, M = _gpu(g, states, step), _gpu(mm, states, step)
        for i in range(len(states)):
            assert tuple(G["stats"][i][:2]) == tuple(M["stats"][i][:2])
            np.testing.assert_allclose(G["qpos"][i], M["qpos"][i], atol=2e-5)
            for f in ("qfrc_actuator", "qfrc_bias", "qfrc_passive"):
                _close(G[f][i], np.float64(M[f][i]), 2e-5, f"state {i} {f}")
            for f in ("qacc", "qacc_smooth", "qfrc_constraint", "qvel", "qacc_warmstart"):
                _close(G[f][i], np.float64(M[f][i]), 2e-3, f"state {i} {f}")


# 8 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("integrator", list(ar.INTEGRATORS))
def test_per_env_gear_and_damping(base, integrator):
    """Env e with a replaced gear / damping is, bit for bit, env e of a plain batch on the model compiled with
    those values: length, velocity, moment and the integrator's gear^2 b2 follow the gear, also where the env's
    damping is all zero."""
    name, m, states = base
    g = ar.general_model(m, KP, KV, seed=6, integrator=integrator, forcerange=0.5, extra_velocity=3)
    rng = np.random.default_rng(12)
    n = len(states)
    ext = [(q, v, w, np.concatenate([c, np.float64(np.float32(rng.uniform(-1, 1, 3)))])) for q, v, w, c in states]
    gear = np.float32(np.asarray(g.actuator_gear) * rng.uniform(0.5, 1.5, (n, g.nu)))
    damp = np.float32(np.asarray(g.dof_damping) * rng.uniform(0.5, 1.5, (n, g.nv)))
    damp[n // 2] = 0.0
    sys_ = mjx.put_model(g)
    out = []
    for step in (False, True):
        d = _load(sys_, ext)
        d.enable_model_params()
        d.set_model_params(None, actuator_gear=torch.tensor(gear, device="cuda"), dof_damping=torch.tensor(damp, device="cuda"))
        (mjx.step if step else mjx.forward)(sys_, d)
        out.append({f: d.get(f).cpu().numpy() for f in FIELDS})
    for i in sorted({0, n // 2, n - 1}):
        sub = ar.with_arrays(g, actuator_gear=np.float64(gear[i]), dof_damping=np.float64(damp[i]))
        for step in (False, True):
            S = _gpu(sub, ext, step)
            for f in FIELDS:
                np.testing.assert_array_equal(out[step][f][i], S[f][i], err_msg=f"env {i} step {step} {f}")
    plain = _gpu(g, ext, True)
    assert not np.array_equal(plain["qvel"], out[1]["qvel"])


# 9 ---------------------------------------------------------------------------------------------------------------
def _env(m, B, max_steps=1000, seed=5):
    cfg = resolve_ids(m, dataclasses.replace(reference_ppo_config().env_config, max_episode_steps=max_steps))
    return HumanoidEnv(mjx.put_model(m), cfg, B, seed=seed, store_derived=True)


def _env_step_against_step(m, B=16):
    """(|qpos| error, |qvel| relative error, bitwise equal) of one mjl_env_step against mjl_step from the same
    state with the ctrl the env step wrote (the action after the flip)."""
    env = _env(m, B)
    env.reset(counter=3)
    pre = {f: env.data.get(f).clone() for f in ("qpos", "qvel", "qacc_warmstart")}
    act = (torch.rand((B, m.nu), generator=torch.Generator().manual_seed(2)) * 2 - 1).cuda()
    _, _, term, trunc = env.step(act, auto_reset=False)
    assert float(term.sum() + trunc.sum()) == 0
    ctrl = env.data.get("ctrl").clone()
    assert float(env.data.get("aux")[:, 0].sum()) > 0 and not torch.equal(ctrl, act)  # some envs are flipped
    d = mjx.make_data(env.sys, B)
    for f, x in pre.items():
        d.set(f, x)
    mjx.step(env.sys, d, ctrl)
    q1, v1, q2, v2 = (x.cpu().numpy() for x in (env.data.get("qpos"), env.data.get("qvel"), d.get("qpos"), d.get("qvel")))
    return np.abs(q1 - q2).max(), np.abs(v1 - v2).max() / (1 + np.abs(v2).max()), np.array_equal(q1, q2) and np.array_equal(v1, v2)


def test_env_step_is_the_step_with_the_flipped_action():
    m = mjx_amd.load_model("humanoid_mjx")
    motors_bitwise = _env_step_against_step(m)[2]
    eq, ev, bitwise = _env_step_against_step(pd_actuators(m, 30.0, 2.0, 0.5))
    print(f"env step vs step: motors bitwise {motors_bitwise}, PD bitwise {bitwise}, |dq| {eq:.2e}, |dv|/s {ev:.2e}")
    if motors_bitwise:  # then the PD model must be as well
        assert bitwise
    assert eq <= 2e-5 and ev <= 2e-3


def test_auto_reset_and_pool_give_the_resets_of_env_reset():
    """test_reset_pool's check on a PD model: every step finishes (max_episode_steps 1); slots 0 and 1 of the
    pool, then the in-place reset of the step's counter, each bit for bit mjl_env_reset at that counter."""
    B = 16
    g = pd_actuators(mjx_amd.load_model("humanoid_mjx"), 30.0, 2.0, 0.5)
    env, ref = _env(g, B, max_steps=1), _env(g, B, max_steps=1)
    env.enable_reset_pool(2)
    env.reset()
    act = torch.zeros((B, g.nu), device="cuda")
    c0 = env.counter
    env.fill_reset_pool(torch.tensor([2], dtype=torch.int32, device="cuda"))
    for j in range(3):
        obs = env.step(act)[0].clone()
        want = _reset_at(ref, slot_counter(c0, j) if j < 2 else env.counter)
        assert torch.equal(obs, want), f"step {j}: obs"
        for f in RESET_STATE:
            assert torch.equal(env.data.get(f), ref.data.get(f)), f"step {j}: {f}"
    assert float(env.data.get("qfrc_actuator").abs().max()) > 0  # the PD forces are part of the reset's forward pass


# 10 --------------------------------------------------------------------------------------------------------------
def test_vjp_record_and_replay_refuse_general_actuators():
    from test_applied_gpu import lib_exports
    B = 4
    m = pd_actuators(mjx_amd.load_model("humanoid_mjx"), 30.0, 2.0, 0.5)
    env = _env(m, B)
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
        "mjl_env_step_record_apg": lambda: L.mjl_env_step_record_apg(h, 0, *nul[:5], 0.99, 1e3, *nul[:6], s),
        "mjl_env_step_record_apg_next": lambda: L.mjl_env_step_record_apg_next(h, 0, *nul[:5], 0.99, 1e3, *nul[:8], 0,
                                                                               *nul[:3], 0, *nul[:4], s),
        "mjl_env_step_vjp_replay_apg": lambda: L.mjl_env_step_vjp_replay_apg(h, 0, *nul[:12], 0, *nul[:7], 0, s),
    }
    named = [n for n in lib_exports() if any(k in n for k in ("step_vjp", "step_record"))]
    assert sorted(named) == sorted(calls), "an entry of the VJP family is not covered"
    for name, call in calls.items():
        assert call() == UNSUPPORTED, name
        assert b"general actuators are not differentiated" in L.mjl_last_error(), name
    with pytest.raises(MjlError, match="non-motor"):
        mjx.step_vjp(env.sys, env.data, gq, gv)
    torch.cuda.synchronize()


# 11 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ar.MODELS)
def test_speedtest_step(name):
    """mjl_speedtest_step on a PD model (the model's own integrator) against the oracle's speed test on the
    equivalent motor model: from make_data with qvel[0] = vel and ctrl 0, F does not depend on vel (the root's
    dofs carry no actuator), so one ctrl' serves every env. Tolerance: qpos atol 2e-5."""
    m = mjx_amd.load_model(name)
    g = ar.general_model(m, KP, KV, seed=8, forcerange=0.35)
    implicit = g.integrator == ar.INTEGRATORS["implicitfast"]
    sys_ = mjx.put_model(g)
    B = 12
    vel = np.linspace(0.0, 1.0, B)
    out = mjx.speedtest_step(sys_, mjx.make_data(sys_, B), torch.tensor(vel, dtype=torch.float32, device="cuda")).cpu().numpy()
    orc = Oracle(ar.motor_model(g, implicit))
    c = ar.motor_ctrl(g, np.asarray(g.qpos0, np.float64), np.zeros(g.nv), np.zeros(g.nu), implicit)
    assert np.abs(c).max() > 0.05  # b0 and the stiffness at qpos0 do act
    for i in range(B):
        v = np.zeros(g.nv)
        v[0] = np.float32(vel[i])
        a = state_arrays(g, orc.step(orc.new_state(np.asarray(g.qpos0, np.float64), v, np.zeros(g.nv), c)))
        assert abs(out[i] - a["qpos"][0]) <= 2e-5, (i, out[i], a["qpos"][0])
