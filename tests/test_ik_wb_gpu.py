"""Whole-body inverse kinematics (mjl_ik_wb / mjx.ik_wb / HumanoidEnv.ik_wb) on the GPU against tests/ik_wb_ref.py.

Problems: tests/test_ik_wb.py wb_problem() for both humanoids and generic_models.full() (nv = 32): three distinct
envs, tiled to nenv = 3 and 65 (one grid tail); every row of every env is compared, against its distinct env's
reference.

Tolerance (the rule of tests/test_ik_gpu.py): per output the yardstick is max |ik_wb_ref in float32 - in float64|
after the same number of iterations; bound = max(8 x yardstick, 1e-6 x max(1, scale)), scale = max |value|.
Active set: every parity case with pairs first asserts that the float64 reference keeps |dist - clear_min| >= 1e-3 m
at every iterate (the one-sided rows make the result discontinuous where dist crosses clear_min). The figures are
printed (pytest -s) and, with MJX_IK_WB_PARITY=<path> in the environment, written there as JSON
(profiles/ik/wb_parity.json is such a run)."""
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
import ik_wb_ref as wb
from test_ik import DAMPING
from test_ik_wb import CLEAR_MIN, CLEAR_TOL, KINDS, MARGIN, MODELS, NDISTINCT, TWO_PLANES, wb_problem

pytestmark = pytest.mark.gpu

SENTINEL = -77.25
PARITY = {}
FIELDS = ("qpos", "err", "com_err", "clearance")


def dev(x, dtype=torch.float32):
    return torch.tensor(np.asarray(x), dtype=dtype, device="cuda")


def tile(x, nenv):
    return np.asarray(x)[np.arange(nenv) % NDISTINCT]


@pytest.fixture(scope="module", params=MODELS)
def model(request):
    P = dict(wb_problem(request.param))
    P["sys"] = mjx.put_model(P["m"])
    P["data"] = {}
    PARITY.setdefault(P["name"], {})
    return P


@pytest.fixture(scope="module", params=[3, 65])
def setup(request, model):
    P, n = dict(model), request.param
    if n not in model["data"]:
        d = mjx.make_data(P["sys"], n)
        d.set("qpos", torch.tensor(tile([s[0] for s in P["states"][:NDISTINCT]], n), dtype=torch.float32))
        model["data"][n] = d
    P["nenv"], P["d"] = n, model["data"][n]
    return P


def _gpu(P, start, frames=False, pos=True, rot=True, com=None, com_weight=None, pairs=None, **kw):
    """mjx.ik_wb on the tiled problem. com: the root; pairs: dict(geom1, geom2, clear_min, clear_weight)."""
    n = P["nenv"]
    kw.setdefault("damping", DAMPING)
    args = (P["frames"], dev(tile(P["tpos"], n)) if pos else None, dev(tile(P["fquat"], n)) if rot else None) if frames else ()
    if frames:
        kw["offset"] = P["off"]
    if com is not None:
        kw.update(com_target=dev(tile(P["com"][com], n)), com_body=com, com_weight=com_weight)
    if pairs is not None:
        kw.update(clearance=(pairs["geom1"], pairs["geom2"]), clearance_min=pairs["clear_min"],
                  clearance_weight=pairs.get("clear_weight"))
    return mjx.ik_wb(P["sys"], P["d"], *args, qpos_start=dev(tile(start, n)), **kw)


_REF = {}


def _ref(P, key, start, dtype, frames=False, pos=True, rot=True, com=None, com_weight=None, pairs=None, mass=None, **kw):
    """The reference of the distinct envs, computed once per (model, case, dtype) and shared by both batch sizes."""
    k = (P["name"], key, dtype)
    if k not in _REF:
        out = []
        for e in range(NDISTINCT):
            a = dict(qpos_start=start[e], damping=DAMPING, dtype=dtype, **kw)
            if frames:
                a.update(body=P["body"], offset=P["local"], target_pos=P["tpos"][e] if pos else None,
                         target_quat=P["tquat"][e] if rot else None)
            if com is not None:
                a.update(com_body=com, com_target=P["com"][com][e], com_weight=com_weight)
            if pairs is not None:
                a.update(geom1=pairs["geom1"], geom2=pairs["geom2"], clear_min=pairs["clear_min"],
                         clear_weight=pairs.get("clear_weight"))
            if mass is not None:
                a["mass"] = mass[e]
            out.append(wb.solve(P["m"], **a))
        _REF[k] = {"qpos": np.float64([o[0] for o in out]), "err": np.float64([o[1] for o in out]),
                   "com_err": np.float64([o[3] for o in out]), "clearance": np.float64([o[4] for o in out]),
                   "niter": [o[2] for o in out], "margin": min([o[5].min() for o in out if o[5].size] + [np.inf])}
    return _REF[k]


def _check(P, key, got, r64, r32):
    """Every field against the float64 reference under the rule of the module docstring; the worst ratio is kept."""
    n, fails, rec = P["nenv"], [], {}
    for f in FIELDS:
        g = getattr(got, f)
        if g is None or r64[f].size == 0:
            continue
        yard, scale = float(np.abs(r64[f] - r32[f]).max()), max(1.0, float(np.abs(r64[f]).max()))
        bound = max(8 * yard, 1e-6 * scale)
        err = float(np.abs(g.cpu().numpy().astype(np.float64) - tile(r64[f], n)).max())
        rec[f] = {"yardstick": yard, "scale": scale, "bound": bound, "worst_gpu_error": err, "ratio": err / bound}
        print(P["name"], n, key, f, {k: float(f"{v:.3g}") for k, v in rec[f].items()})
        if not err <= bound:
            fails.append((f, err, bound))
    rec["worst_ratio"] = max(r["ratio"] for r in rec.values())
    old = PARITY[P["name"]].get(key)
    if old is None or old["worst_ratio"] < rec["worst_ratio"]:
        PARITY[P["name"]][key] = rec
    return fails


@pytest.mark.parametrize("iterations", [0, 3])
def test_no_added_tasks_is_mjl_ik(setup, iterations):
    P, n = setup, setup["nenv"]
    kw = dict(offset=P["off"], qpos_start=dev(tile(P["start"], n)), iterations=iterations, damping=DAMPING, posture=0.02, max_step=0.05)
    a = mjx.ik(P["sys"], P["d"], P["frames"], dev(tile(P["tpos"], n)), dev(tile(P["fquat"], n)), **kw)
    b = mjx.ik_wb(P["sys"], P["d"], P["frames"], dev(tile(P["tpos"], n)), dev(tile(P["fquat"], n)), **kw)
    assert torch.equal(a.qpos, b.qpos) and torch.equal(a.err, b.err) and torch.equal(a.niter, b.niter)
    assert (b.niter == iterations).all() and (b.com_err == 0).all() and b.clearance.shape == (n, 0)
    if iterations == 0:
        assert torch.equal(b.qpos, kw["qpos_start"])


@pytest.mark.parametrize("iterations", [1, 10])
@pytest.mark.parametrize("weights", [(1, 1, 1), (1, 1, 0)], ids=["xyz", "xy"])
@pytest.mark.parametrize("root", [0, 1], ids=["whole", "subtree"])
def test_com_alone(setup, iterations, weights, root):
    P = setup
    b = P["roots"][root]
    key = "com/%s/%s/%d" % ("whole" if root == 0 else "subtree", "".join("xyz"[i] for i in range(3) if weights[i]), iterations)
    case = dict(com=b, com_weight=list(weights), iterations=iterations)
    r64, r32 = _ref(P, key, P["start"], np.float64, **case), _ref(P, key, P["start"], np.float32, **case)
    got = _gpu(P, P["start"], **case)
    assert (got.niter == iterations).all() and got.err.shape == (P["nenv"], 0, 6)
    fails = _check(P, key, got, r64, r32)
    assert not fails, fails
    assert np.abs(r64["qpos"] - P["start"]).max() > 1e-3  # the CoM rows did move the state
    if not weights[2]:
        assert (got.com_err[:, 2] == 0).all()
    if iterations == 10:
        assert float(got.com_err.abs().max()) < 1e-4


@pytest.mark.parametrize("kind", list(KINDS))
def test_overlapping_pair_is_separated(setup, kind):
    P = setup
    O = P["overlap"][kind]
    assert (O["dist"] < 0).all()
    pairs = dict(geom1=[O["pair"][0]], geom2=[O["pair"][1]], clear_min=CLEAR_MIN)
    zero = _gpu(P, O["start"], pairs=pairs, iterations=0, limits=O["limits"])
    assert np.abs(zero.clearance[:NDISTINCT, 0].cpu().numpy() - O["dist"]).max() < 1e-5  # the start does overlap on the GPU too
    got = _gpu(P, O["start"], pairs=pairs, iterations=10, limits=O["limits"])
    c = got.clearance.cpu().numpy()
    print(P["name"], P["nenv"], kind, O["pair"], "start", O["dist"], "end", c[:NDISTINCT, 0])
    assert (c >= np.float32(CLEAR_MIN) - CLEAR_TOL).all(), c.min()
    assert torch.isfinite(got.qpos).all()


def test_inactive_pair_moves_nothing(setup):
    P = setup
    M = P["mixed"]
    pairs = dict(geom1=M["geom1"][1:2], geom2=M["geom2"][1:2], clear_min=0.01)
    assert _ref(P, "far", P["start"], np.float64, pairs=pairs, iterations=10)["margin"] >= MARGIN
    got = _gpu(P, P["start"], pairs=pairs, iterations=10, posture=0.0)
    assert torch.equal(got.qpos, dev(tile(P["start"], P["nenv"]))) and (got.niter == 10).all()
    assert (got.clearance > 0.5).all()


@pytest.mark.parametrize("posture", [0.0, 0.05])
def test_everything_together(setup, posture):
    P, m = setup, setup["m"]
    key = "all/posture%g" % posture
    dofs = list(range(6, m.nv))  # the free joint is frozen
    dm = sum(1 << d_ for d_ in dofs)
    case = dict(frames=True, com=0, com_weight=[1, 1, 0.5], pairs=P["mixed"], iterations=3, posture=posture, max_step=0.01, limits=True)
    r64 = _ref(P, key, P["start"], np.float64, dofmask=dm, **case)
    r32 = _ref(P, key, P["start"], np.float32, dofmask=dm, **case)
    print(P["name"], key, "smallest |dist - clear_min| over the iterates:", r64["margin"])
    assert r64["margin"] >= MARGIN
    on = P["mixed"]["start_dist"] < P["mixed"]["clear_min"]
    assert on[:, [0, 2]].all() and not on[:, [1, 3]].any()  # two active pairs, two inactive
    got = _gpu(P, P["start"], dofs=dofs, **case)
    fails = _check(P, key, got, r64, r32)
    assert not fails, fails
    start = dev(tile(P["start"], P["nenv"]))
    assert torch.equal(got.qpos[:, :7], start[:, :7]) and (got.qpos[:, 7:] != start[:, 7:]).any(dim=1).all()
    assert np.abs(r64["qpos"] - P["start"]).max() >= 0.0099  # max_step was active


def test_tol_counts_the_added_terms(setup):
    """tol > 0 with a frame task whose residual is below tol from the start and a CoM task whose residual is not:
    the solve goes on until the CoM term of res is below tol too. The reference's res is well off tol on both
    sides of its exit (asserted first), so niter is the same in both precisions."""
    P, m, n, tol = setup, setup["m"], setup["nenv"], 2.5e-4
    body, local = P["body"][:1], P["local"][:1]
    tpos = np.float32([ik.frame_pose(m, q, body, local)[0] for q in P["start"]]).astype(np.float64)
    kw = dict(body=body, offset=local, damping=DAMPING, com_body=0, iterations=10)
    refs = {dt: [wb.solve(m, target_pos=tpos[e], qpos_start=P["start"][e], com_target=P["com"][0][e], tol=tol, dtype=dt, **kw)
                 for e in range(NDISTINCT)] for dt in (np.float64, np.float32)}
    res = lambda r: max(np.linalg.norm(r[1][:, :3], axis=1).max(), np.abs(r[3]).max())
    for e, r in enumerate(refs[np.float64]):
        k = r[2]
        assert 0 < k < 10 and res(r) < tol / 2, (e, k, res(r))
        before = wb.solve(m, target_pos=tpos[e], qpos_start=P["start"][e], com_target=P["com"][0][e], **dict(kw, iterations=k - 1))
        assert res(before) > 2 * tol, (e, res(before))
        zero = wb.solve(m, target_pos=tpos[e], qpos_start=P["start"][e], com_target=P["com"][0][e], **dict(kw, iterations=0))
        assert np.linalg.norm(zero[1][:, :3], axis=1).max() < tol / 2  # the frame term alone would stop at k = 0
        assert refs[np.float32][e][2] == k
    got = mjx.ik_wb(P["sys"], P["d"], P["frames"][:1], dev(tile(tpos, n)), offset=P["off"][:1], com_target=dev(tile(P["com"][0], n)),
                    qpos_start=dev(tile(P["start"], n)), iterations=10, damping=DAMPING, tol=tol)
    want = tile([r[2] for r in refs[np.float64]], n)
    print(P["name"], n, "iterations taken with tol = %g:" % tol, want[:NDISTINCT].tolist())
    assert (got.niter.cpu().numpy() == want).all(), got.niter
    pack = lambda rs: {"qpos": np.float64([r[0] for r in rs]), "err": np.float64([r[1] for r in rs]),
                       "com_err": np.float64([r[3] for r in rs]), "clearance": np.zeros((NDISTINCT, 0))}
    fails = _check(P, "tol", got, pack(refs[np.float64]), pack(refs[np.float32]))
    assert not fails, fails
    assert float(got.com_err.abs().max()) < tol and float(got.err[:, :, :3].norm(dim=2).max()) < tol


def test_per_env_masses(model):
    P, m, n = dict(model), model["m"], NDISTINCT
    P["nenv"] = n
    P["d"] = d = mjx.make_data(P["sys"], n)
    mass = np.float32(np.tile(m.body_mass, (n, 1)))
    mass[1, 1] *= 3  # env 1: a torso three times as heavy
    case = dict(com=0, iterations=1)
    nominal = _gpu(P, P["start"], **case)
    d.enable_model_params(True)
    d.set_model_params(None, body_mass=torch.tensor(mass, device="cuda"))
    got = _gpu(P, P["start"], **case)
    r64 = _ref(P, "mass", P["start"], np.float64, mass=np.float64(mass), **case)
    r32 = _ref(P, "mass", P["start"], np.float32, mass=np.float64(mass), **case)
    fails = _check(P, "mass", got, r64, r32)
    assert not fails, fails
    assert torch.equal(got.qpos[0], nominal.qpos[0]) and torch.equal(got.qpos[2], nominal.qpos[2])
    assert float((got.qpos[1] - nominal.qpos[1]).abs().max()) > 1e-4


def test_plumbing(setup):
    P, m, n = setup, setup["m"], setup["nenv"]
    nt, M = len(P["body"]), P["mixed"]
    case = dict(frames=True, com=0, pairs=M, iterations=2, max_step=0.02)
    full = _gpu(P, P["start"], **case)
    mask = torch.tensor(np.arange(n) % 3 != 1, dtype=torch.float32, device="cuda")
    out = (torch.full((n, m.nq), SENTINEL, device="cuda"), torch.full((n, nt, 6), SENTINEL, device="cuda"),
           torch.full((n,), -7, dtype=torch.int32, device="cuda"), torch.full((n, 3), SENTINEL, device="cuda"),
           torch.full((n, 4), SENTINEL, device="cuda"))
    part = _gpu(P, P["start"], mask=mask, out=out, **case)
    on, off = mask > 0.5, mask < 0.5
    for f, a, b in zip(part._fields, part, full):
        assert (a[off] == (-7 if f == "niter" else SENTINEL)).all() and torch.equal(a[on], b[on]), f
    some = _gpu(P, P["start"], out=(torch.empty((n, m.nq), device="cuda"), None, None, None, torch.empty((n, 4), device="cuda")), **case)
    assert some.err is None and some.niter is None and some.com_err is None
    assert torch.equal(some.qpos, full.qpos) and torch.equal(some.clearance, full.clearance)
    # a bad body id: NaN rows, by mjl_ik's rule (raw call: mjx checks ids on the host)
    L, ptr = lib(), lambda t: C.c_void_p(t.data_ptr())
    body = dev(P["body"], torch.int32)
    body[-1] = m.nbody
    g1, g2 = (C.c_int32 * 4)(*M["geom1"]), (C.c_int32 * 4)(*M["geom2"])
    cmin = (C.c_float * 4)(*[float(x) for x in M["clear_min"]])
    tp, ct = dev(tile(P["tpos"], n)), dev(tile(P["com"][0], n))
    rc = L.mjl_ik_wb(P["d"].handle, None, nt, ptr(body), None, ptr(tp), None, None, None, None, -1, 2, 1e-3, 0.0, 0.0, 0.0, 0,
                     ptr(out[0]), ptr(out[1]), ptr(out[2]), 0, ptr(ct), None, 4, g1, g2, cmin, None, ptr(out[3]), ptr(out[4]),
                     mjx._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert all(torch.isnan(out[i]).all() for i in (0, 1, 3, 4)) and (out[2] == 0).all()


def test_captured_with_an_env_step(model):
    P = model
    if P["name"] not in mjx_amd.BUILTIN_MODELS:
        return  # the env is the humanoid's
    m, sys_, B, M = P["m"], P["sys"], 8, P["mixed"]
    cfg = resolve_ids(m, dataclasses.replace(reference_ppo_config().env_config, max_episode_steps=1000))
    act = torch.tensor(np.random.default_rng(2).uniform(-1, 1, (B, m.nu)), dtype=torch.float32, device="cuda")
    tpos, tquat, ct = dev(tile(P["tpos"], B)), dev(tile(P["fquat"], B)), dev(tile(P["com"][0], B))
    kw = dict(offset=P["off"], com_target=ct, com_weight=[1, 1, 0], clearance=(M["geom1"], M["geom2"]), clearance_min=M["clear_min"],
              iterations=4, damping=DAMPING, posture=0.01, max_step=0.2)

    def make():
        env = HumanoidEnv(sys_, cfg, B, seed=11)
        env.reset(counter=1)
        return env
    env = make()
    eager = []
    for i in range(2):
        env.step(act, auto_reset=False, counter=2 + i)
        eager.append([t.clone() for t in env.ik_wb(P["frames"], tpos, tquat, **kw)])
    warm = make()  # warm-up launches outside the capture, on another batch
    warm.step(act, auto_reset=False, counter=2)
    warm.ik_wb(P["frames"], tpos, tquat, **kw)
    env = make()
    bufs = list(env.ik_wb(P["frames"], tpos, tquat, **kw))  # the first, allocating call
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.step(act, auto_reset=False, counter=2)
        env.ik_wb(P["frames"], tpos, tquat, **kw)
    for i in range(2):
        g.replay()
        torch.cuda.synchronize()
        for k, want in enumerate(eager[i]):
            assert torch.equal(bufs[k], want), (i, k)
    assert not torch.equal(eager[0][0], eager[1][0])


def test_refusals(model):
    P, m = model, model["m"]
    n, nt, M = NDISTINCT, len(P["body"]), P["mixed"]
    d = mjx.make_data(P["sys"], n)
    L, err = lib(), HEADER.enums["MJL_ERR_ARG"]
    ptr = lambda t: C.c_void_p(t.data_ptr())
    body, tp, ct = dev(P["body"], torch.int32), dev(P["tpos"]), dev(P["com"][0])
    q, e = torch.full((n, m.nq), SENTINEL, device="cuda"), torch.full((n, nt, 6), SENTINEL, device="cuda")
    ce, cl = torch.full((n, 3), SENTINEL, device="cuda"), torch.full((n, 4), SENTINEL, device="cuda")
    fl = lambda xs: (C.c_float * len(xs))(*[float(x) for x in xs])
    il = lambda xs: (C.c_int32 * len(xs))(*[int(x) for x in xs])

    def call(batch=d.handle, ntask=nt, body=ptr(body), tpos=ptr(tp), iterations=2, damping=1e-3, flags=0, qout=ptr(q), com_body=0,
             com_target=ptr(ct), com_weight=None, npair=4, g1=M["geom1"], g2=M["geom2"], cmin=M["clear_min"], cw=None):
        return L.mjl_ik_wb(batch, None, ntask, body, None, tpos, None, None, None, None, -1, iterations, damping, 0.0, 0.0, 0.0,
                           flags, qout, ptr(e), None, com_body, com_target, None if com_weight is None else fl(com_weight), npair,
                           None if g1 is None else il(g1), None if g2 is None else il(g2), None if cmin is None else fl(cmin),
                           None if cw is None else fl(cw), ptr(ce), ptr(cl), mjx._stream())
    nan, inf = float("nan"), float("inf")
    cases = [call(batch=None), call(qout=None), call(ntask=-1), call(ntask=33), call(body=None), call(tpos=None),
             call(iterations=-1), call(damping=0.0), call(flags=2),
             call(npair=-1), call(npair=33), call(ntask=0, com_body=-1, npair=0),
             call(com_body=-2), call(com_body=m.nbody), call(com_target=None),
             call(com_weight=[1, -1, 1]), call(com_weight=[1, nan, 1]), call(com_weight=[inf, 1, 1]),
             call(cw=[1, 1, -0.5, 1]), call(cw=[1, 1, inf, 1]), call(cmin=[0.01, -0.01, 0.01, 0.01]), call(cmin=[0.01, nan, 0.01, 0.01]),
             call(g1=None), call(cmin=None),
             call(g1=[M["geom1"][0], -1, M["geom1"][2], M["geom1"][3]]), call(g2=[M["geom2"][0], m.ngeom, M["geom2"][2], M["geom2"][3]]),
             call(g1=M["geom2"][:1] + M["geom1"][1:])]                       # a geom paired with itself
    for i, rc in enumerate(cases):
        assert rc == err, (i, rc)
    assert len(L.mjl_last_error()) > 10
    torch.cuda.synchronize()
    assert all((t == SENTINEL).all() for t in (q, e, ce, cl))  # nothing touched the device
    assert call() == 0 and call(ntask=0, body=None, tpos=None) == 0 and call(com_body=-1, com_target=None, npair=0) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(q).all() and torch.isfinite(cl).all()
    with pytest.raises(ValueError, match="32"):
        mjx.ik_wb(P["sys"], d, clearance=mjx.collision_pairs(P["sys"]))
    # two different planes: mjl_geom_distance's plane - plane rule, refused on the host (the two-plane model)
    sys2 = mjx.put_model(mjcf.compile_xml_string(TWO_PLANES, "two_planes"))
    d2 = mjx.make_data(sys2, 2)
    q2 = torch.full((2, sys2.nq), SENTINEL, device="cuda")
    c2 = torch.full((2, 1), SENTINEL, device="cuda")

    def call2(g1, g2):
        return L.mjl_ik_wb(d2.handle, None, 0, None, None, None, None, None, None, None, -1, 2, 1e-3, 0.0, 0.0, 0.0, 0, ptr(q2),
                           None, None, -1, None, None, 1, il([g1]), il([g2]), fl([0.01]), None, None, ptr(c2), mjx._stream())
    assert call2(0, 1) == err and "both planes" in L.mjl_last_error().decode() and call2(1, 0) == err
    torch.cuda.synchronize()
    assert (q2 == SENTINEL).all() and (c2 == SENTINEL).all()
    assert call2(0, 2) == 0 and call2(2, 1) == 0  # a plane against the sphere, either order
    torch.cuda.synchronize()
    assert torch.isfinite(q2).all() and torch.isfinite(c2).all()
    with pytest.raises(ValueError, match="both planes"):
        mjx.ik_wb(sys2, d2, clearance=("a", "b"))
    with pytest.raises(ValueError):
        mjx.ik_wb(P["sys"], d, clearance=("no_such_geom", 0))
    with pytest.raises(mjx.MjlError):
        mjx.ik_wb(P["sys"], d)


def test_zz_parity_table():
    """Runs last in this module: the worst ratio of every parity case of every model."""
    assert set(PARITY) == set(MODELS)
    for name, rec in PARITY.items():
        for key, r in rec.items():
            print(name, key, "worst ratio", float(f"{r['worst_ratio']:.3g}"))
    path = os.environ.get("MJX_IK_WB_PARITY")
    if path:
        with open(path, "w") as fh:
            json.dump(PARITY, fh, indent=1, sort_keys=True)
