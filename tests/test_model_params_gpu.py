"""Per-env model parameters on the GPU (MJL_OPT_PER_ENV_MODEL, mjl_batch_set_model_params).

The rule under test: env e's model block is byte for byte what mjl_model_create makes of the descriptor with
env e's values substituted. Seen through behaviour: env e of a heterogeneous batch equals, array_equal on every
readable field, env e of a plain batch on that substituted model (tests 1-3, 5, 6, 8), and independently the
fp64 oracle on it at tests/test_gpu_parity.py's tolerances (test 4; its precondition on the draw is
tests/test_model_params_abi.py's float32-oracle test). States, loader and tolerances are test_gpu_parity's."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import mjx_amd
from mjx_amd import abi, mjx, ppo
from mjx_amd._header import HEADER
from mjx_amd._lib import MjlError, lib
from mjx_amd.config import reference_ppo_config
from mjx_amd.envs import HumanoidEnv, resolve_ids
from mjx_amd.mjx import _ptr, _stream
from mjx_amd.randomize import FIELDS
from oracle import Oracle, state_arrays

from model_params_ref import MODELS, draw, nominal_params, substituted
from test_gpu_parity import _close, _load, _states

pytestmark = pytest.mark.gpu

UNSUPPORTED, ARG = HEADER.enums["MJL_ERR_UNSUPPORTED"], HEADER.enums["MJL_ERR_ARG"]
STATE = ("qpos", "qvel", "qacc_warmstart", "ctrl", "time", "qacc", "xpos", "xquat", "sensordata", "qfrc_actuator",
         "qfrc_bias", "qfrc_passive", "qfrc_constraint", "qacc_smooth", "stats")
CONTACT = ("ncon", "geom", "dim", "efc_address", "dist", "pos", "frame", "force", "body_force")


def _dev(p):
    return {k: torch.tensor(np.asarray(v), dtype=torch.float32, device="cuda").contiguous() for k, v in p.items()}


def _np(t):
    return t.detach().cpu().numpy().copy()


def _env(m, B, max_steps=3, seed=3):
    ecfg = dataclasses.replace(reference_ppo_config().env_config, max_episode_steps=max_steps)
    return HumanoidEnv(mjx.put_model(m), resolve_ids(m, ecfg), B, seed=seed, store_derived=True)


def _run(m, states, prepare=None, env_level=True, xfrc=None):
    """Everything the option touches, on model m from the given states, as {name: array with a leading env
    axis}: forward, forward_contacts, step; then a HumanoidEnv: reset with explicit noise, 5 env steps with
    auto-reset in place (episodes of 3 steps), pooled resets filled and 4 more steps merging them.
    prepare(data): called on each fresh batch (sets the option / the parameters)."""
    sys_, n, out = mjx.put_model(m), len(states), {}
    prepare = prepare or (lambda d: None)

    def fields(d, tag):
        for f in STATE:
            out[f"{tag}/{f}"] = _np(d.get(f))

    d = _load(sys_, states)
    prepare(d)
    if xfrc is not None:
        d.attach_applied(None, xfrc)
    mjx.forward(sys_, d)
    fields(d, "forward")
    c = mjx.forward_contacts(sys_, d, body_force=True)
    for f in CONTACT:
        out[f"contacts/{f}"] = _np(getattr(c, f))
    d = _load(sys_, states)
    prepare(d)
    if xfrc is not None:
        d.attach_applied(None, xfrc)
    mjx.step(sys_, d)
    fields(d, "step")
    if not env_level:
        return out
    env = _env(m, n)
    prepare(env.data)
    if xfrc is not None:
        env.attach_applied(None, xfrc)
    g = torch.Generator().manual_seed(5)
    noise = torch.rand((n, m.nq - 7 + m.nv + 2), generator=g)
    out["reset/obs"] = _np(env.reset(noise=noise))
    out["reset/state"] = _np(env.get_state())
    fields(env.data, "reset")
    resets = 0
    for t in range(9):
        if t == 5:
            env.enable_reset_pool(2)
            env.fill_reset_pool(torch.tensor([2], dtype=torch.int32, device="cuda"))
        act = (torch.rand((n, m.nu), generator=g) * 2 - 1).cuda()
        for what, x in zip(("obs", "rew", "term", "trunc"), env.step(act)):
            out[f"envstep{t}/{what}"] = _np(x)
        out[f"envstep{t}/state"] = _np(env.get_state())
        resets += int(np.maximum(out[f"envstep{t}/term"], out[f"envstep{t}/trunc"]).sum())
    fields(env.data, "envstep8")
    assert resets >= 2 * n  # every env reset in place and from the pool
    return out


def _same(a, b, rows_a, rows_b, what):
    assert a.keys() == b.keys()
    for k in a:
        np.testing.assert_array_equal(a[k][rows_a], b[k][rows_b], err_msg=f"{what}: {k}")


def _setter(params, mask=None):
    def prepare(d):
        d.enable_model_params()
        if params is not None:
            d.set_model_params(mask, **_dev(params))
    return prepare


@pytest.fixture(scope="module", params=MODELS)
def setup(request):
    """Per model: the states, the tests' draw, the plain run on the model itself and the heterogeneous run;
    computed once, read by the tests."""
    name = request.param
    m = mjx_amd.load_model(name)
    states = _states(m)
    p = draw(m, len(states))
    return name, m, states, p, _run(m, states), _run(m, states, _setter(p))


# 1 ---------------------------------------------------------------------------------------------------------------
def test_option_on_and_nothing_set_is_the_plain_batch(setup):
    name, m, states, p, plain, het = setup
    on = _run(m, states, _setter(None))
    _same(on, plain, slice(None), slice(None), "option on, nothing set")
    d = _load(mjx.put_model(m), states)
    d.enable_model_params()
    for k, v in nominal_params(m, len(states)).items():  # the blocks hold the model's values
        np.testing.assert_array_equal(_np(d.get_model_params(k)).reshape(v.shape), v, err_msg=k)


# 2 ---------------------------------------------------------------------------------------------------------------
def test_each_env_is_its_substituted_model(setup):
    name, m, states, p, plain, het = setup
    n = len(states)
    picks = sorted({0, n // 3, n // 2, (2 * n) // 3, n - 1})  # n // 2: the env without damping
    assert len(picks) >= 4 and not p["dof_damping"][n // 2].any() and np.asarray(m.dof_damping).any()
    for i in picks:
        sub = _run(substituted(name, p, i), states)
        _same(het, sub, i, i, f"env {i}")
    differs = [k for k in het if not np.array_equal(het[k], plain[k])]
    assert any(k.startswith("forward/") for k in differs) and any(k.startswith("envstep") for k in differs)


def test_undamped_model_with_one_damped_env():
    """The reverse of the draw's undamped env: a model whose damping is all zero (any_damping = 0 in the shared
    block) and one env that is damped: that env's block must carry the flag and both homes of the damping."""
    name = "humanoid_mjx"
    m = substituted(name, nominal_params(mjx_amd.load_model(name), 1), 0, fields=(), zero_damping=True)
    assert not np.asarray(m.dof_damping).any()
    states = _states(mjx_amd.load_model(name))[:8]
    n, j = len(states), 5
    damp = np.zeros((n, m.nv), np.float32)
    damp[j] = np.float32(mjx_amd.load_model(name).dof_damping) * 1.5
    het = _run(m, states, _setter({"dof_damping": damp}))
    _same(het, _run(substituted(name, {"dof_damping": damp}, j, fields=("dof_damping",), zero_damping=True), states),
          j, j, "the damped env")
    keep = [e for e in range(n) if e != j]
    _same(het, _run(m, states), keep, keep, "the undamped envs")


# 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
def test_one_field_at_a_time(setup, field):
    name, m, states, p, plain, het = setup
    n, j = len(states), 7
    one = {field: nominal_params(m, n)[field]}
    one[field][j] = p[field][j]
    assert not np.array_equal(one[field][j], one[field][0])
    got = _run(m, states, _setter(one), env_level=False)
    _same(got, _run(substituted(name, p, j, fields=(field,)), states, env_level=False), j, j, f"{field}: env {j}")
    keep = [e for e in range(n) if e != j]
    ref = {k: v for k, v in plain.items() if k in got}
    _same(got, ref, keep, keep, f"{field}: the other envs")


# 4 ---------------------------------------------------------------------------------------------------------------
def test_against_the_fp64_oracle(setup):
    name, m, states, p, plain, het = setup
    for i, (q, v, w, c) in enumerate(states):
        sub = substituted(name, p, i)
        orc = Oracle(sub)
        a = state_arrays(sub, orc.forward(orc.new_state(q, v, w, c)))
        st = het["forward/stats"][i]
        assert (st[0], st[1]) == (a["ncon"], a["nefc"]), f"env {i}: contact / row counts"
        for f in ("qfrc_bias", "qfrc_passive", "qfrc_actuator"):
            _close(het[f"forward/{f}"][i], a[f], 2e-5, f"env {i} {f}")
        for f in ("qacc", "qfrc_constraint"):
            _close(het[f"forward/{f}"][i], a[f], 2e-3, f"env {i} {f}")
        a = state_arrays(sub, orc.step(orc.new_state(q, v, w, c)))
        np.testing.assert_allclose(het["step/qpos"][i], a["qpos"], atol=2e-5)
        _close(het["step/qvel"][i], a["qvel"], 2e-3, f"env {i} qvel")
        _close(het["step/qacc_warmstart"][i], a["qacc_warmstart"], 2e-3, f"env {i} qacc_warmstart")


# 5 ---------------------------------------------------------------------------------------------------------------
def test_mask_and_null_entries_keep_what_they_should(setup):
    name, m, states, p, plain, het = setup
    sys_, n = mjx.put_model(m), len(states)
    mask = torch.tensor([float(e % 3 != 1) for e in range(n)], device="cuda")
    on = np.array([e % 3 != 1 for e in range(n)])
    d = _load(sys_, states)
    d.enable_model_params()
    d.set_model_params(mask, **_dev(p))
    nom = nominal_params(m, n)
    for k in FIELDS:
        got = _np(d.get_model_params(k)).reshape(p[k].shape)
        np.testing.assert_array_equal(got[on], p[k][on], err_msg=k)
        np.testing.assert_array_equal(got[~on], nom[k][~on], err_msg=k)
    mjx.step(sys_, d)
    for f in STATE:
        x = _np(d.get(f))
        np.testing.assert_array_equal(x[on], het[f"step/{f}"][on], err_msg=f)
        np.testing.assert_array_equal(x[~on], plain[f"step/{f}"][~on], err_msg=f)
    # a null entry keeps the field: everything set, then the gear alone overwritten with the model's
    d = _load(sys_, states)
    d.enable_model_params()
    d.set_model_params(**_dev(p))
    d.set_model_params(actuator_gear=_dev(nom)["actuator_gear"], body_mass=None)
    for k in FIELDS:
        want = nom[k] if k == "actuator_gear" else p[k]
        np.testing.assert_array_equal(_np(d.get_model_params(k)).reshape(want.shape), want, err_msg=k)
    with pytest.raises(MjlError):
        d.set_model_params(body_masses=_dev(p)["body_mass"])
    with pytest.raises(MjlError):
        d.set_model_params(body_mass=_dev(p)["body_mass"][:, :-1].contiguous())


# 6 ---------------------------------------------------------------------------------------------------------------
def test_captured_set_and_env_step_reads_the_values_at_replay(setup):
    name, m, states, p, plain, het = setup
    n = len(states)
    first, second = _dev(nominal_params(m, n)), _dev(p)
    g = torch.Generator().manual_seed(9)
    noise = torch.rand((n, m.nq - 7 + m.nv + 2), generator=g)
    act = (torch.rand((n, m.nu), generator=g) * 2 - 1).cuda()
    res = []
    for captured in (False, True):
        env = _env(m, n)
        env.enable_model_params()
        env.reset(noise=noise)
        buf = {k: v.clone() for k, v in first.items()}

        def pair():
            env.set_model_params(**buf)
            env.step(act, counter=1)

        if captured:
            state0 = env.get_state().clone()
            pair()  # eager first: loads the code objects outside the capture
            torch.cuda.synchronize()
            env.set_state(state0)
            graph = torch.cuda.CUDAGraph()
            with ppo.graph_capture(graph):
                pair()
            env.set_state(state0)
        for k in buf:
            buf[k].copy_(second[k])  # in place: the captured launch reads the new values
        graph.replay() if captured else pair()
        res.append([_np(x) for x in (env.obs, env.rew, env.term, env.trunc, env.get_state())]
                   + [_np(env.get_model_params(k)) for k in FIELDS])
    for a, b in zip(*res):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(res[0][5], p["body_mass"])


# 7 ---------------------------------------------------------------------------------------------------------------
def test_refusals():
    B = 4
    m = mjx_amd.load_model("humanoid_mjx")
    env = _env(m, B, max_steps=1000)
    env.reset()
    env.data.set_option(abi.OPT_VJP_TAPE, 1)
    L, h, s = lib(), env.data.handle, _stream()
    vals = (C.c_void_p * abi.NMP)()
    assert L.mjl_batch_set_model_params(h, vals, None, s) == ARG  # the option is off
    assert b"MJL_OPT_PER_ENV_MODEL" in L.mjl_last_error()
    out = torch.zeros((B, m.nbody), device="cuda")
    assert L.mjl_batch_get_model_params(h, 0, _ptr(out), s) == ARG
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
    refused_only = {  # refused before any other argument is looked at
        "mjl_env_step_record_apg": lambda: L.mjl_env_step_record_apg(h, 0, *nul[:5], 0.99, 1e3, *nul[:6], s),
        "mjl_env_step_record_apg_next": lambda: L.mjl_env_step_record_apg_next(h, 0, *nul[:5], 0.99, 1e3, *nul[:8], 0,
                                                                               *nul[:3], 0, *nul[:4], s),
        "mjl_env_step_vjp_replay_apg": lambda: L.mjl_env_step_vjp_replay_apg(h, 0, *nul[:12], 0, *nul[:7], 0, s),
    }
    from mjx_amd import _lib
    named = [n for n in _lib.EXPORTS if any(k in n for k in ("step_vjp", "step_record"))]
    assert sorted(named) == sorted(list(calls) + list(refused_only)), "an entry of the VJP family is not covered"
    env.enable_model_params()
    for name, call in {**calls, **refused_only}.items():
        assert call() == UNSUPPORTED, name
        assert b"per-env model parameters" in L.mjl_last_error()
    with pytest.raises(MjlError, match="per-env model parameters"):
        env.step_vjp(act, gq, gv, gr)
    env.enable_model_params(False)
    for name, call in calls.items():
        assert call() == 0, (name, L.mjl_last_error())
    torch.cuda.synchronize()
    assert L.mjl_batch_set_model_params(h, vals, None, s) == ARG  # off again


# 8 ---------------------------------------------------------------------------------------------------------------
def test_with_applied_forces(setup):
    name, m, states, p, plain, het = setup
    n, i = len(states), len(states) // 3
    rng = np.random.default_rng(8)
    xfrc = np.concatenate([rng.uniform(-50, 50, (n, m.nbody, 3)), rng.uniform(-10, 10, (n, m.nbody, 3))], 2)
    xfrc = torch.tensor(xfrc, dtype=torch.float32, device="cuda")
    both = _run(m, states, _setter(p), xfrc=xfrc)
    _same(both, _run(substituted(name, p, i), states, xfrc=xfrc), i, i, f"pushed env {i}")
    assert not np.array_equal(both["step/qvel"], het["step/qvel"])  # the forces did act


# trainer -------------------------------------------------------------------------------------------------------
def _trainer(randomize, seed=11):
    m = mjx_amd.load_model("humanoid_mjx")
    cfg = reference_ppo_config()
    cfg.num_envs, cfg.rollout_length, cfg.minibatch_size, cfg.epochs, cfg.seed = 64, 8, 128, 1, 5
    env = HumanoidEnv(mjx.put_model(m), resolve_ids(m, cfg.env_config), cfg.num_envs, seed=seed)
    return ppo.PPOTrainer(cfg, env, None, device="cuda", randomize=randomize), env, m


def test_trainer_with_randomisation_and_without():
    """Two iterations (the second replays the captured rollout) on randomised training envs: finite, and the
    env's blocks hold the trainer's draw. Without `randomize` no option is set: the set call is refused and
    the run is the plain trainer's, metric for metric."""
    tr, env, m = _trainer({"mass": (0.5, 1.5), "friction": (0.3, 1.5), "gear": (0.7, 1.3)})
    for it in range(2):
        met = tr.iteration(it)
        assert all(np.isfinite(v) for v in met.values()), met
        assert torch.isfinite(tr.obs).all()
    for k in FIELDS:
        assert torch.equal(env.get_model_params(k).reshape(tr.model_params[k].shape), tr.model_params[k]), k
    mass = _np(env.get_model_params("body_mass"))
    assert len({tuple(r) for r in mass.tolist()}) == env.num_envs
    np.testing.assert_array_equal(_np(env.get_model_params("dof_damping"))[3], np.float32(m.dof_damping))  # no range
    plain, penv, _ = _trainer(None)
    assert plain.randomize is None
    with pytest.raises(MjlError, match="MJL_OPT_PER_ENV_MODEL"):
        penv.get_model_params("body_mass")
    ref, _, _ = _trainer(None)
    for it in range(2):
        a, b = plain.iteration(it), ref.iteration(it)
        assert {k: v for k, v in a.items() if k != "env_steps_per_sec"} == \
            {k: v for k, v in b.items() if k != "env_steps_per_sec"}
        assert torch.equal(plain.obs, ref.obs)
