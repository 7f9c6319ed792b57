"""Batched inverse kinematics (mjl_ik / mjx.ik / HumanoidEnv.ik) on the GPU against tests/ik_ref.py in fp64.

Problems: tests/test_ik.py problem() for both humanoids (5 envs), the two-tree model of tests/test_dyn_gpu.py and
generic_models.full() (4 envs each); 2-5 tasks on sites and bodies, one with an offset.

Tolerances (the rule of tests/test_bodydata_gpu.py tolerances): per output the yardstick is max |ik_ref in float32 -
in float64| over the envs after the same number of iterations; the kernel gets bound = max(8 x yardstick, 1e-6 x
max(1, scale)), scale = max |value|. The figures are printed (pytest -s) and, with MJX_IK_PARITY=<path> in the
environment, written there as JSON (profiles/ik/parity.json is such a run)."""
import ctypes as C
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

import mjx_amd
from mjx_amd import abi, mjcf, mjx
from mjx_amd._header import HEADER
from mjx_amd._lib import lib
from mjx_amd.config import reference_ppo_config
from mjx_amd.envs import HumanoidEnv, resolve_ids

import ik_ref as ik
from test_ik import DAMPING, ITERATIONS, MODELS, problem, residual_norms

pytestmark = pytest.mark.gpu

SENTINEL = -77.25
PARITY = {}
# one-iteration cases: (position targets, orientation targets, posture, max_step); 0.01 rad is below every first step
ONE = [(True, False, 0.0, 0.0), (False, True, 0.0, 0.0), (True, True, 0.0, 0.0),
       (True, False, 0.05, 0.01), (False, True, 0.05, 0.01), (True, True, 0.05, 0.01),
       (True, True, 0.05, 0.0), (True, True, 0.0, 0.01)]
TEN = dict(posture=0.01, max_step=0.05)  # the bound is active in the first iterations and inactive in the last


def dev(x, dtype=torch.float32):
    return torch.tensor(np.asarray(x), dtype=dtype, device="cuda")


def _load(sys_, states):
    d = mjx.make_data(sys_, len(states))
    for i, f in enumerate(("qpos", "qvel", "qacc_warmstart", "ctrl")):
        d.set(f, torch.tensor(np.array([s[i] for s in states]), dtype=torch.float32))
    return d


@pytest.fixture(scope="module", params=MODELS)
def setup(request):
    P = dict(problem(request.param))
    P["sys"] = mjx.put_model(P["m"])
    P["d"] = _load(P["sys"], P["states"])
    P["ref"] = np.float32(np.random.default_rng(8).uniform(-0.1, 0.1, P["start"].shape)) + np.float32(P["start"])
    PARITY.setdefault(P["name"], {})
    return P


def _ref(P, envs, dtype, pos, rot, iterations, **kw):
    out = [ik.solve(P["m"], P["body"], P["local"], P["tpos"][e] if pos else None, P["tquat"][e] if rot else None,
                    qpos_start=P["start"][e], qpos_ref=P["ref"][e], iterations=iterations, damping=DAMPING,
                    dtype=dtype, **kw) for e in envs]
    return np.array([np.float64(o[0]) for o in out]), np.array([np.float64(o[1]) for o in out])


def _gpu(P, pos=True, rot=True, **kw):
    kw.setdefault("damping", DAMPING)
    kw.setdefault("qpos_start", dev(P["start"]))
    return mjx.ik(P["sys"], P["d"], P["frames"], dev(P["tpos"]) if pos else None, dev(P["fquat"]) if rot else None,
                  offset=P["off"], **kw)


def _bounds(r64, r32):
    out = {}
    for f, a, b in (("qpos", r64[0], r32[0]), ("err", r64[1], r32[1])):
        yard, scale = float(np.abs(a - b).max()), max(1.0, float(np.abs(a).max()))
        out[f] = {"yardstick": yard, "scale": scale, "bound": max(8 * yard, 1e-6 * scale)}
    return out


def _check(P, key, got, r64, r32, envs):
    tol = _bounds(r64, r32)
    fails = []
    for f, g, want in (("qpos", got.qpos, r64[0]), ("err", got.err, r64[1])):
        err = float(np.abs(g.cpu().numpy().astype(np.float64)[envs] - want).max())
        tol[f]["worst_gpu_error"] = err
        print(P["name"], key, f, {k: float(f"{v:.3g}") for k, v in tol[f].items()})
        if not err <= tol[f]["bound"]:
            fails.append((f, err, tol[f]["bound"]))
    PARITY[P["name"]][key] = tol
    return tol, fails


@pytest.mark.parametrize("case", ONE, ids=lambda c: "%s%s-posture%g-maxstep%g" % ("p" if c[0] else "", "r" if c[1] else "", c[2], c[3]))
def test_one_iteration_parity(setup, case):
    P = setup
    pos, rot, posture, max_step = case
    envs = list(range(len(P["start"])))
    kw = dict(posture=posture, max_step=max_step)
    r64, r32 = _ref(P, envs, np.float64, pos, rot, 1, **kw), _ref(P, envs, np.float32, pos, rot, 1, **kw)
    got = _gpu(P, pos, rot, iterations=1, qpos_ref=dev(P["ref"]), **kw)
    assert (got.niter == 1).all()
    tol, fails = _check(P, "one/%s%s/%g/%g" % ("p" if pos else "", "r" if rot else "", posture, max_step), got, r64, r32, envs)
    assert not fails, fails
    assert np.abs(r64[0] - P["start"]).max() > 0.005  # the iteration did move the state (max_step is 0.01 where active)
    if not pos:
        assert (got.err[:, :, :3] == 0).all()
    if not rot:
        assert (got.err[:, :, 3:] == 0).all()


def test_ten_iteration_parity(setup):
    P = setup
    envs = list(range(4))
    r64, r32 = _ref(P, envs, np.float64, True, True, 10, **TEN), _ref(P, envs, np.float32, True, True, 10, **TEN)
    got = _gpu(P, iterations=10, qpos_ref=dev(P["ref"]), **TEN)
    _, fails = _check(P, "ten", got, r64, r32, envs)
    assert not fails, fails


def _independent_residual(P, qpos):
    """(|e_p|, |e_r|, e [nenv, ntask, 6]) of qpos from a fresh Data: jac_local's world points, and the frames'
    orientations from the stored xquat of a forward pass times the frames' rotations in their bodies."""
    d = mjx.make_data(P["sys"], qpos.shape[0])
    d.set("qpos", qpos)
    x = mjx.jac_local(P["sys"], d, P["frames"], P["off"])[2].cpu().numpy().astype(np.float64)
    mjx.forward(P["sys"], d)
    xq = d.get("xquat").cpu().numpy().astype(np.float64)
    e = np.zeros(x.shape[:2] + (6,))
    e[..., :3] = P["tpos"] - x
    for i in range(x.shape[0]):
        for t, b in enumerate(P["body"]):
            fq = mjcf.quat_mul(xq[i, b], P["fq"][t])
            e[i, t, 3:] = ik.rotvec(ik.dr._qmul(P["fquat"][i, t] / np.linalg.norm(P["fquat"][i, t]), ik._conj(fq / np.linalg.norm(fq))))
    return e


def test_convergence(setup):
    P = setup
    n = len(P["start"])
    got = _gpu(P, iterations=ITERATIONS)
    ref32 = [ik.solve(P["m"], P["body"], P["local"], P["tpos"][e], P["tquat"][e], qpos_start=P["start"][e],
                      iterations=ITERATIONS, damping=DAMPING, dtype=np.float32)[1] for e in range(n)]
    rp, rr = residual_norms(np.float64(np.array(ref32)))
    e = _independent_residual(P, got.qpos)
    ep, er = residual_norms(e)
    scale = max(1.0, float(np.abs(P["tpos"]).max()))
    bp, brot = max(10 * rp.max(), 1e-5 * scale), max(10 * rr.max(), 1e-5)
    print(P["name"], "residual after %d iterations: |e_p| %.3g (reference in float32 %.3g, bound %.3g), |e_r| %.3g "
          "(reference %.3g, bound %.3g)" % (ITERATIONS, ep.max(), rp.max(), bp, er.max(), rr.max(), brot))
    PARITY[P["name"]]["convergence"] = {"pos": float(ep.max()), "pos_ref32": float(rp.max()), "pos_bound": bp,
                                        "rot": float(er.max()), "rot_ref32": float(rr.max()), "rot_bound": brot}
    assert ep.max() <= bp and er.max() <= brot
    # the err output against the independent residual, under the one-iteration tolerance
    envs = list(range(n))
    tol = _bounds(_ref(P, envs, np.float64, True, True, 1), _ref(P, envs, np.float32, True, True, 1))["err"]["bound"]
    assert np.abs(got.err.cpu().numpy() - e).max() <= tol, (np.abs(got.err.cpu().numpy() - e).max(), tol)


def test_limits_and_robustness(setup):
    P = setup
    m, A = P["m"], P["m"].arrays
    far = P["tpos"].copy()
    far[:, :, 0] += 10.0
    hinges = [d for d in range(m.nv) if A["jnt_type"][A["dof_jntid"][d]] == mjcf.JNT_HINGE]
    for tpos, dofs in ((P["tpos"], None), (far, hinges)):  # reachable; out of reach: the free joints may not move
        got = mjx.ik(P["sys"], P["d"], P["frames"], dev(tpos), dev(P["fquat"]), offset=P["off"], qpos_start=dev(P["start"]),
                     dofs=dofs, iterations=ITERATIONS, damping=DAMPING, limits=True)
        q = got.qpos.cpu().numpy()
        assert np.isfinite(q).all() and np.isfinite(got.err.cpu().numpy()).all()
        nlim = 0
        for j in range(m.njnt):
            a = int(A["jnt_qposadr"][j])
            if A["jnt_type"][j] == mjcf.JNT_FREE:
                assert np.abs(np.linalg.norm(np.float64(q[:, a + 3:a + 7]), axis=1) - 1).max() <= 1e-6
            elif A["jnt_limited"][j]:
                lo, hi = np.float32(A["jnt_range"][j])
                assert (q[:, a] >= lo).all() and (q[:, a] <= hi).all(), j
                nlim += int(((q[:, a] == lo) | (q[:, a] == hi)).any())
    assert float(got.err[:, :, :3].abs().max()) > 5.0
    assert nlim > 0 or not A["jnt_limited"].any()  # the far target did push hinges onto their limits
    free = mjx.ik(P["sys"], P["d"], P["frames"], dev(far), None, offset=P["off"], qpos_start=dev(P["start"]),
                  dofs=hinges, iterations=3, damping=DAMPING, limits=False).qpos.cpu().numpy()
    assert np.isfinite(free).all()


def test_dofs(setup):
    P = setup
    m = P["m"]
    start = dev(P["start"])
    if P["name"] == "two_trees":  # every dof may move; the task is on the chain: the ball is left alone
        got = _gpu(P, iterations=5)
        assert torch.equal(got.qpos[:, 10:], start[:, 10:]) and not torch.equal(got.qpos[:, :10], start[:, :10])
        return
    got = _gpu(P, iterations=5, dofs=list(range(6, m.nv)))
    assert torch.equal(got.qpos[:, :7], start[:, :7])  # the free root, bit for bit
    assert (got.qpos[:, 7:] != start[:, 7:]).any(dim=1).all()
    only = _gpu(P, iterations=5, dofs=[d < 6 for d in range(m.nv)])
    assert torch.equal(only.qpos[:, 7:], start[:, 7:]) and (only.qpos[:, :7] != start[:, :7]).any(dim=1).all()


def test_non_interference(setup):
    P = setup
    m, sys_, d = P["m"], P["sys"], _load(P["sys"], P["states"])
    n, nt = len(P["start"]), len(P["body"])
    start = dev(P["start"])
    mjx.forward(sys_, d)
    fields = ("qpos", "qvel", "qacc_warmstart", "xpos", "xquat", "qacc", "qfrc_bias", "qfrc_constraint")
    keep = {f: d.get(f).clone() for f in fields}
    args = (sys_, d, P["frames"], dev(P["tpos"]), dev(P["fquat"]))
    kw = dict(offset=P["off"], damping=DAMPING)
    zero = mjx.ik(*args, qpos_start=start, iterations=0, **kw)
    assert torch.equal(zero.qpos, start) and (zero.niter == 0).all()
    assert float(zero.err.abs().max()) > 1e-3
    # the batch's own qpos is the default start
    own = mjx.ik(*args, iterations=0, **kw)
    assert torch.equal(own.qpos, keep["qpos"])
    # a masked env keeps its rows
    mask = torch.tensor(([1, 0, 1, 1, 0])[:n], dtype=torch.float32, device="cuda")
    out = (torch.full((n, m.nq), SENTINEL, device="cuda"), torch.full((n, nt, 6), SENTINEL, device="cuda"),
           torch.full((n,), -7, dtype=torch.int32, device="cuda"))
    full = mjx.ik(*args, qpos_start=start, iterations=3, **kw)
    part = mjx.ik(*args, qpos_start=start, iterations=3, mask=mask, out=out, **kw)
    on, off = mask > 0.5, mask < 0.5
    assert (part.qpos[off] == SENTINEL).all() and (part.err[off] == SENTINEL).all() and (part.niter[off] == -7).all()
    assert torch.equal(part.qpos[on], full.qpos[on]) and torch.equal(part.err[on], full.err[on]) and (part.niter[on] == 3).all()
    for f, t in keep.items():
        assert torch.equal(d.get(f), t), f
    # per-env model parameters do not matter
    d.enable_model_params(True)
    rng = np.random.default_rng(9)
    mass = np.float32(np.tile(m.body_mass, (n, 1)) * rng.uniform(0.5, 1.5, (n, m.nbody)))
    d.set_model_params(None, body_mass=torch.tensor(mass, device="cuda"))
    rand = mjx.ik(*args, qpos_start=start, iterations=3, **kw)
    assert torch.equal(rand.qpos, full.qpos) and torch.equal(rand.err, full.err)


def test_early_exit(setup):
    P = setup
    tol = 1e-3
    got = _gpu(P, iterations=ITERATIONS, tol=tol)
    niter = got.niter.cpu().numpy()
    print(P["name"], "iterations taken with tol = %g:" % tol, niter.tolist())
    assert (niter < ITERATIONS).all() and (niter > 0).all()
    ep, er = residual_norms(got.err.cpu().numpy())
    assert max(ep.max(), er.max()) < tol
    for k in sorted(set(niter.tolist())):
        fixed = _gpu(P, iterations=int(k))
        rows = torch.tensor(niter == k, device="cuda")
        assert torch.equal(fixed.qpos[rows], got.qpos[rows]) and torch.equal(fixed.err[rows], got.err[rows])


def test_captured_with_an_env_step(setup):
    P = setup
    if P["name"] not in mjx_amd.BUILTIN_MODELS:
        return  # the env is the humanoid's
    m, sys_ = P["m"], P["sys"]
    B = 8
    frames = P["frames"]
    cfg = resolve_ids(m, dataclasses.replace(reference_ppo_config().env_config, max_episode_steps=1000))
    act = torch.tensor(np.random.default_rng(2).uniform(-1, 1, (B, m.nu)), dtype=torch.float32, device="cuda")
    tpos, tquat = dev(np.resize(P["tpos"], (B,) + P["tpos"].shape[1:])), dev(np.resize(P["fquat"], (B,) + P["fquat"].shape[1:]))
    kw = dict(offset=P["off"], iterations=4, damping=DAMPING, posture=0.01, max_step=0.2)

    def make():
        env = HumanoidEnv(sys_, cfg, B, seed=11)
        env.reset(counter=1)
        return env
    env = make()
    eager = []
    for i in range(2):
        env.step(act, auto_reset=False, counter=2 + i)
        eager.append([t.clone() for t in env.ik(frames, tpos, tquat, **kw)])
    warm = make()  # warm-up launches outside the capture, on another batch
    warm.step(act, auto_reset=False, counter=2)
    warm.ik(frames, tpos, tquat, **kw)
    env = make()
    bufs = list(env.ik(frames, tpos, tquat, **kw))  # the first, allocating call
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.step(act, auto_reset=False, counter=2)
        env.ik(frames, tpos, tquat, **kw)
    for i in range(2):
        g.replay()
        torch.cuda.synchronize()
        for k, want in enumerate(eager[i]):
            assert torch.equal(bufs[k], want), (i, k)
    assert not torch.equal(eager[0][0], eager[1][0])


def test_arguments(setup):
    P = setup
    m, d = P["m"], P["d"]
    n, nt = len(P["start"]), len(P["body"])
    L, err = lib(), HEADER.enums["MJL_ERR_ARG"]
    ptr = lambda t: C.c_void_p(t.data_ptr())
    body = dev(P["body"], torch.int32)
    tp, tq = dev(P["tpos"]), dev(P["tquat"])
    q, e = torch.full((n, m.nq), SENTINEL, device="cuda"), torch.full((n, nt, 6), SENTINEL, device="cuda")
    ni = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    h, st = d.handle, mjx._stream()

    def call(batch=h, ntask=nt, body=ptr(body), tpos=ptr(tp), tquat=ptr(tq), iterations=3, damping=1e-3, posture=0.0,
             max_step=0.0, tol=0.0, flags=0, qout=ptr(q)):
        return L.mjl_ik(batch, None, ntask, body, None, tpos, tquat, None, None, None, -1, iterations, damping, posture,
                        max_step, tol, flags, qout, ptr(e), ptr(ni), st)
    cases = [call(batch=None), call(body=None), call(qout=None), call(ntask=0), call(ntask=33),
             call(tpos=None, tquat=None), call(iterations=-1), call(iterations=1025), call(damping=0.0),
             call(damping=-1.0), call(posture=-0.1), call(max_step=-0.1), call(tol=-1e-3), call(flags=2)]
    for i, rc in enumerate(cases):
        assert rc == err, (i, rc)
    assert len(L.mjl_last_error()) > 10
    torch.cuda.synchronize()
    assert (q == SENTINEL).all() and (e == SENTINEL).all() and (ni == -7).all()
    assert call(iterations=0) == 0 and call(iterations=1024, tol=1e-2, flags=abi.IK_LIMITS) == 0
    torch.cuda.synchronize()
    assert not (q == SENTINEL).any() and torch.isfinite(q).all()
    # a body id outside the model: NaN rows for every env
    bad = body.clone()
    bad[-1] = m.nbody
    assert call(body=ptr(bad)) == 0
    torch.cuda.synchronize()
    assert torch.isnan(q).all() and torch.isnan(e).all() and (ni == 0).all()
    with pytest.raises(ValueError):
        mjx.ik(P["sys"], d, [("xbody", m.nbody)], tp[:, :1])
    with pytest.raises(mjx.MjlError):
        mjx.ik(P["sys"], d, P["frames"])


def test_zz_parity_table():
    """Runs last in this module: the table of every model the tests above covered."""
    assert set(PARITY) == set(MODELS)
    for name, rec in PARITY.items():
        for key, r in rec.items():
            print(name, key, r)
    path = os.environ.get("MJX_IK_PARITY")
    if path:
        with open(path, "w") as fh:
            json.dump(PARITY, fh, indent=1, sort_keys=True)
