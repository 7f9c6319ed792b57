"""Inverse dynamics (mjl_inverse, mjx.inverse, HumanoidEnv.inverse) on the GPU against tests/inverse_ref.py in fp64.

Batches: those of tests/test_dyn_gpu.py (5 build_states envs of both humanoids, 4 states of the two-tree model and
of generic_models.full()), each state with the three accelerations of tests/test_inverse.py cases(): the oracle's
forward qacc, that plus a seeded perturbation that changes the active set, zeros. tests/test_inverse.py asserts
what these inputs have to provide (no contact on its margin, active contact / limit rows, an inactive row, a flip).

Tolerances (the rule of tests/test_dyn_gpu.py): per field the yardstick is max |inverse_ref in float32 on the
float32 oracle's output - inverse_ref in float64| over the states and accelerations; the kernel gets
bound = max(8 x yardstick, 1e-6 x max(1, scale)), scale = max |value|. The identities (forward agreement, discrete
round trip) take 8 x the residual of the same identity evaluated with the float32 oracle and the float32
reference. The figures are printed (pytest -s) and, with MJX_INVERSE_PARITY=<path> in the environment, written
there as JSON (profiles/inverse/parity.json is such a run)."""
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

import mjx_amd
from mjx_amd import abi, mjx
from mjx_amd._header import HEADER
from mjx_amd.actuators import pd_actuators
from mjx_amd.config import reference_ppo_config
from mjx_amd.envs import HumanoidEnv, resolve_ids
from oracle import Oracle, state_arrays

import actuators_ref as ar
import dyn_ref as dr
import inverse_ref as ir
import model_params_ref as mp
from test_dyn_gpu import _load
from test_inverse import MODELS, cases

pytestmark = pytest.mark.gpu

SENTINEL = -77.25
FIELDS = ("qfrc_inverse", "qfrc_constraint", "qfrc_inverse_discrete", "qfrc_constraint_discrete")
PARITY = {}


def _reference(m, recs, key, dtype):
    """{field: [nstate, 3, nv]} of inverse_ref on the `key` oracle's outputs."""
    out = {f: [] for f in FIELDS}
    for rec in recs:
        o, raw = rec[key]
        J, kinds = ir.constraint_jacobian(m, o, dtype)
        assert list(kinds) == [int(t) for t in o["efc_type"]]
        for disc, sfx in ((False, ""), (True, "_discrete")):
            r = [ir.inverse(m, o, raw, a, disc, dtype, J)[:2] for a in rec["acc"]]
            out["qfrc_inverse" + sfx].append(np.array([x[0] for x in r], np.float64))
            out["qfrc_constraint" + sfx].append(np.array([x[1] for x in r], np.float64))
    return {f: np.array(v) for f, v in out.items()}


def tolerances(r64, r32):
    tol = {}
    for f in r64:
        yard = float(np.abs(r32[f] - r64[f]).max())
        scale = max(1.0, float(np.abs(r64[f]).max()))
        tol[f] = {"yardstick": yard, "scale": scale, "bound": max(8 * yard, 1e-6 * scale)}
    return tol


@pytest.fixture(scope="module", params=MODELS)
def setup(request):
    name = request.param
    m, states, recs = cases(name)
    r64 = _reference(m, recs, "f64", np.float64)
    tol = tolerances(r64, _reference(m, recs, "f32", np.float32))
    PARITY[name] = {f: dict(t, worst_gpu_error=0.0) for f, t in tol.items()}
    print(name, "tolerances:", {f: {k: float(f"{v:.3g}") for k, v in t.items()} for f, t in tol.items()})
    acc = torch.tensor(np.array([rec["acc"] for rec in recs]), dtype=torch.float32, device="cuda")  # [n, 3, nv]
    return dict(name=name, m=m, sys=mjx.put_model(m), states=states, recs=recs, r64=r64, tol=tol, acc=acc)


def _run_all(S, d):
    """{field: [n, 3, nv]} from the GPU: every acceleration, continuous and discrete."""
    got = {f: [] for f in FIELDS}
    for k in range(3):
        for disc, sfx in ((False, ""), (True, "_discrete")):
            q, c = mjx.inverse(S["sys"], d, S["acc"][:, k].contiguous(), discrete=disc, with_constraint=True)
            got["qfrc_inverse" + sfx].append(q.cpu().numpy().astype(np.float64))
            got["qfrc_constraint" + sfx].append(c.cpu().numpy().astype(np.float64))
    return {f: np.stack(v, axis=1) for f, v in got.items()}


def _check(S, got, want, what, record=True):
    fails = []
    for f in FIELDS:
        err, bound = float(np.abs(got[f] - want[f]).max()), S["tol"][f]["bound"]
        if record:
            rec = PARITY[S["name"]][f]
            rec["worst_gpu_error"] = max(rec["worst_gpu_error"], err)
        print(S["name"], what, f, "yardstick %.3g bound %.3g worst GPU error %.3g" % (S["tol"][f]["yardstick"], bound, err))
        if err > bound:
            fails.append((f, err, bound))
    assert not fails, (what, fails)


# 1, 4 ---------------------------------------------------------------------------------------------------------------
def test_parity_and_global_rows(setup):
    S = setup
    d = _load(S["sys"], S["states"])
    lds = _run_all(S, d)
    _check(S, lds, S["r64"], "LDS rows")
    d.set_option(abi.OPT_FORCE_GLOBAL_ROWS, 1)
    glb = _run_all(S, d)
    _check(S, glb, S["r64"], "global rows")
    _check(S, glb, lds, "global rows against LDS rows", record=False)
    if S["name"] in mjx_amd.BUILTIN_MODELS:  # the constraint force and the discrete correction do take part
        assert np.abs(S["r64"]["qfrc_constraint"]).max() > 1.0
        assert np.abs(S["r64"]["qfrc_inverse_discrete"] - S["r64"]["qfrc_inverse"]).max() > 100 * S["tol"]["qfrc_inverse"]["bound"]


def _applied_total(m, o, qfrc_actuator, qfrc, xfrc):
    """qfrc_actuator + qfrc_applied + sum_b J_b' xfrc_b (force and torque at xipos) in float64."""
    tot = np.float64(qfrc_actuator) + qfrc
    axes = dr.dof_axes(m, o)
    for b in range(1, m.nbody):
        if xfrc[b].any():
            jp, jr = dr.jac(m, o, b, o["xipos"][b], np.float64, axes)
            tot = tot + jp.T @ xfrc[b, :3] + jr.T @ xfrc[b, 3:]
    return tot


def _applied(m, n):
    """Applied forces on envs 1 and 3 (float32 values): a generalized force on every dof, a wrench on two bodies."""
    rng = np.random.default_rng(8)
    qfrc, xfrc = np.zeros((n, m.nv), np.float32), np.zeros((n, m.nbody, 6), np.float32)
    for e in (1, 3):
        qfrc[e] = rng.uniform(-2, 2, m.nv)
        for b in (1, m.nbody - 1):
            xfrc[e, b] = rng.uniform(-5, 5, 6)
    return qfrc, xfrc


# 2 ------------------------------------------------------------------------------------------------------------------
def test_agrees_with_the_forward_solve(setup):
    S = setup
    m, sys_, n = S["m"], S["sys"], len(S["states"])
    yard = 0.0
    for rec in S["recs"]:  # the identity in float32: the float32 oracle's solution through the float32 reference
        o32, raw32 = rec["f32"]
        q32 = ir.inverse(m, o32, raw32, o32["qacc"], False, np.float32)[0]
        yard = max(yard, float(np.abs(np.float64(q32) - o32["qfrc_actuator"]).max()))
    d = _load(sys_, S["states"])
    qfrc, xfrc = _applied(m, n)
    d.attach_applied(torch.tensor(qfrc, device="cuda"), torch.tensor(xfrc, device="cuda"))
    mjx.forward(sys_, d)
    got = mjx.inverse(sys_, d).cpu().numpy().astype(np.float64)
    act = d.get("qfrc_actuator").cpu().numpy()
    want = np.array([_applied_total(m, S["recs"][e]["f64"][0], act[e], np.float64(qfrc[e]), np.float64(xfrc[e]))
                     for e in range(n)])
    err = float(np.abs(got - want).max())
    PARITY[S["name"]]["forward_identity"] = {"yardstick": yard, "bound": 8 * yard, "worst_gpu_error": err}
    print(S["name"], "forward identity: yardstick %.3g bound %.3g worst GPU error %.3g" % (yard, 8 * yard, err))
    assert np.abs(want - act).max() > 1.0  # the applied forces are part of the total
    assert err <= 8 * yard, (err, 8 * yard)


def _round_trip(name, g, states, orc_model, orc_ctrl):
    """Discrete round trip of model g on the GPU; the yardstick from the float32 oracle on orc_model."""
    sys_, n, dt = mjx.put_model(g), len(states), g.timestep
    orc = Oracle(orc_model, use_float=True)
    yard = 0.0
    for st, c in zip(states, orc_ctrl):
        raw = orc.forward(orc.new_state(st[0], st[1], st[2], c))
        o32 = state_arrays(orc_model, raw)
        s1 = state_arrays(orc_model, orc.step(orc.new_state(st[0], st[1], st[2], c)))
        a = (np.float64(np.float32(s1["qvel"])) - np.float64(np.float32(st[1]))) / dt
        q32 = ir.inverse(orc_model, o32, raw, a, True, np.float32)[0]
        yard = max(yard, float(np.abs(np.float64(q32) - o32["qfrc_actuator"]).max()))
    d = _load(sys_, states)
    qfrc, xfrc = _applied(g, n)
    d.attach_applied(torch.tensor(qfrc, device="cuda"), torch.tensor(xfrc, device="cuda"))
    keep = {f: d.get(f).clone() for f in ("qpos", "qvel", "qacc_warmstart", "time")}
    mjx.step(sys_, d)
    a = (d.get("qvel").cpu().numpy().astype(np.float64) - keep["qvel"].cpu().numpy().astype(np.float64)) / dt
    for f, t in keep.items():
        d.set(f, t)
    mjx.forward(sys_, d)  # qfrc_actuator of the restored state
    act = d.get("qfrc_actuator").cpu().numpy()
    got = mjx.inverse(sys_, d, torch.tensor(a, dtype=torch.float32), discrete=True).cpu().numpy().astype(np.float64)
    o64 = Oracle(orc_model)
    want = np.array([_applied_total(g, state_arrays(orc_model, o64.forward(o64.new_state(*states[e][:3]))), act[e],
                                    np.float64(qfrc[e]), np.float64(xfrc[e])) for e in range(n)])
    err = float(np.abs(got - want).max())
    PARITY.setdefault(name, {})["round_trip"] = {"yardstick": yard, "bound": 8 * yard, "worst_gpu_error": err}
    print(name, "discrete round trip: yardstick %.3g bound %.3g worst GPU error %.3g" % (yard, 8 * yard, err))
    cont = mjx.inverse(sys_, d, torch.tensor(a, dtype=torch.float32)).cpu().numpy()
    assert np.abs(cont - want).max() > 10 * max(err, 8 * yard)  # without the correction the identity is off
    assert err <= 8 * yard, (name, err, 8 * yard)


# 3 ------------------------------------------------------------------------------------------------------------------
def test_discrete_round_trip(setup):
    """humanoid_mjx integrates with implicitfast, humanoid with Euler + eulerdamp."""
    S = setup
    if S["name"] not in mjx_amd.BUILTIN_MODELS:
        return
    assert {mjx_amd.load_model(k).integrator for k in mjx_amd.BUILTIN_MODELS} == {0, 3}
    _round_trip(S["name"], S["m"], S["states"], S["m"], [st[3] for st in S["states"]])


def test_discrete_round_trip_pd_actuators():
    """Position-derivative actuators under implicitfast: gear^2 biasprm[2] joins the integrator's diagonal. The
    oracle has motors only, so its model is the equivalent motor model of tests/actuators_ref.py."""
    m, states, _ = cases("humanoid_mjx")
    g = pd_actuators(m, 20.0, 1.5, 0.5)
    assert g.integrator == 3 and (np.asarray(g.arrays["actuator_biasprm"])[:, 2] != 0).all()
    assert np.abs(ir.integrator_diagonal(g) - ir.integrator_diagonal(m)).max() > 1.0
    octrl = [ar.motor_ctrl(g, st[0], st[1], st[3], True) for st in states]
    _round_trip("humanoid_mjx_pd", g, states, ar.motor_model(g, True), octrl)


# 5 ------------------------------------------------------------------------------------------------------------------
def test_per_env_model_parameters(setup):
    S = setup
    if S["name"] not in mp.MODELS:
        return
    name, m, sys_, n = S["name"], S["m"], S["sys"], len(S["states"])
    fields = ("body_mass", "body_inertia", "dof_damping", "dof_armature", "actuator_gear")
    p = mp.draw(m, n)
    envs = (0, 1, 2, 4)  # env 2 = n // 2 has no damping at all
    d = _load(sys_, S["states"])
    d.enable_model_params(True)
    mask = torch.zeros(n, device="cuda")
    mask[list(envs)] = 1
    d.set_model_params(mask, **{k: torch.tensor(p[k], device="cuda") for k in fields})
    got = _run_all(S, d)
    r64, r32 = ({f: [] for f in FIELDS} for _ in range(2))
    for e in envs:
        sub = mp.substituted(name, p, e, fields)
        rec = dict(S["recs"][e])
        for key, orc in (("f64", Oracle(sub)), ("f32", Oracle(sub, use_float=True))):
            raw = orc.forward(orc.new_state(*S["states"][e]))
            rec[key] = (state_arrays(sub, raw), raw)
        a, b = _reference(sub, [rec], "f64", np.float64), _reference(sub, [rec], "f32", np.float32)
        for f in FIELDS:
            r64[f].append(a[f][0])
            r32[f].append(b[f][0])
    r64, r32 = ({f: np.array(v) for f, v in r.items()} for r in (r64, r32))
    tol = tolerances(r64, r32)
    fails = []
    for f in FIELDS:
        err = float(np.abs(got[f][list(envs)] - r64[f]).max())
        print(name, "per-env", f, "yardstick %.3g bound %.3g worst GPU error %.3g" % (tol[f]["yardstick"], tol[f]["bound"], err))
        if err > tol[f]["bound"]:
            fails.append((f, err, tol[f]["bound"]))
    assert not fails, fails
    f = "qfrc_inverse"
    assert np.abs(r64[f] - S["r64"][f][list(envs)]).max() > 10 * tol[f]["bound"]  # the values did move
    _check(S, {f: v[[3]] for f, v in got.items()}, {f: v[[3]] for f, v in S["r64"].items()}, "nominal env", record=False)


# 6, 7 ---------------------------------------------------------------------------------------------------------------
def test_mask_and_untouched_state(setup):
    S = setup
    sys_, n, nv = S["sys"], len(S["states"]), S["m"].nv
    d = _load(sys_, S["states"])
    mjx.forward(sys_, d)
    keep = {f: d.get(f).clone() for f in abi.FIELD}
    assert len(keep) == HEADER.enums["MJL_NFIELD"]
    mask = torch.tensor(([1, 0, 1, 1, 0])[:n], dtype=torch.float32, device="cuda")
    full = lambda: torch.full((n, nv), SENTINEL, device="cuda")
    for glob in (0, 1):
        d.set_option(abi.OPT_FORCE_GLOBAL_ROWS, glob)
        for disc in (False, True):
            for qacc in (None, S["acc"][:, 1].contiguous()):
                q, c = mjx.inverse(sys_, d, qacc, discrete=disc, mask=mask, out=(full(), full()), with_constraint=True)
                for t in (q, c):
                    assert (t[mask < 0.5] == SENTINEL).all() and not (t[mask > 0.5] == SENTINEL).any()
                    assert torch.isfinite(t).all()
                alone = mjx.inverse(sys_, d, qacc, discrete=disc)  # without the second output: the same values
                assert torch.equal(alone[mask > 0.5], q[mask > 0.5])
    for f, t in keep.items():
        assert torch.equal(d.get(f), t), f
    fresh = mjx.inverse(sys_, d, mask=mask)
    assert (fresh[mask < 0.5] == 0).all()


# 8 ------------------------------------------------------------------------------------------------------------------
def test_captured_with_an_env_step(setup):
    S = setup
    if S["name"] not in mjx_amd.BUILTIN_MODELS:
        return  # the env is the humanoid's
    m, sys_ = S["m"], S["sys"]
    B = 8
    cfg = resolve_ids(m, dataclasses.replace(reference_ppo_config().env_config, max_episode_steps=1000))
    act = torch.tensor(np.random.default_rng(2).uniform(-1, 1, (B, m.nu)), dtype=torch.float32, device="cuda")
    qacc = torch.tensor(np.random.default_rng(3).uniform(-20, 20, (B, m.nv)), dtype=torch.float32, device="cuda")

    def make():
        env = HumanoidEnv(sys_, cfg, B, seed=11)
        env.reset(counter=1)
        return env
    env = make()
    eager = []
    for i in range(2):
        env.step(act, auto_reset=False, counter=2 + i)
        eager.append([t.clone() for t in env.inverse(qacc, discrete=True)])
    assert not torch.equal(eager[0][0], eager[1][0])
    warm = make()  # warm-up launches outside the capture, on another batch
    warm.step(act, auto_reset=False, counter=2)
    warm.inverse(qacc, discrete=True)
    env = make()
    bufs = env.inverse(qacc, discrete=True)
    assert env.inverse(qacc, discrete=True)[0] is bufs[0]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.step(act, auto_reset=False, counter=2)
        env.inverse(qacc, discrete=True)
    for i in range(2):
        g.replay()
        torch.cuda.synchronize()
        for k, want in enumerate(eager[i]):
            assert torch.equal(bufs[k], want), (i, k)


def test_zz_parity_table():
    """Runs last in this module: the table of every model the tests above covered."""
    assert set(MODELS) <= set(PARITY)
    for name, rec in PARITY.items():
        for f, r in rec.items():
            print(name, f, {k: float(f"{v:.3g}") for k, v in r.items()})
    path = os.environ.get("MJX_INVERSE_PARITY")
    if path:
        with open(path, "w") as fh:
            json.dump(PARITY, fh, indent=1, sort_keys=True)
