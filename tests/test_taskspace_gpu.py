"""Task-space dynamics readout (mjl_jac_dot / mjl_centroidal, mjx.jac_dot / jac_dot_local / centroidal /
jac_subtree_com / angmom_mat, HumanoidEnv.jac_dot / centroidal) on the GPU against tests/taskspace_ref.py in fp64.

Batches: the 5 envs of tests/test_bodydata.py build_states for both humanoids, 4 random states for the two-tree
model (nv = 15: the dof masks keep the trees apart, one body chain of hinges) and for generic_models.full()
(nv = 32 fills every dof lane). Points as tests/test_dyn_gpu.py _points: every body origin, every site, three
bodies with an offset (an odd and an even count occur; npoint = 1 and 3 are run as well: the odd tail of the
two-points-per-pass loop). Subtree roots: the whole model, body 1, a mid body and a leaf.

Tolerances (the rule of tests/test_dyn_gpu.py tolerances): per field the yardstick is max |taskspace_ref in
float32 - in float64| over the states; the kernel gets bound = max(8 x yardstick, 1e-6 x max(1, scale)), scale =
max |value|. The figures are printed (pytest -s) and, with MJX_TASKSPACE_PARITY=<path> in the environment, written
there as JSON (profiles/taskspace/parity.json is such a run)."""
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
from oracle import Oracle, state_arrays

import dyn_ref as dr
import generic_models as gm
import taskspace_ref as tr
from test_bodydata import build_states
from test_dyn import generic_states

pytestmark = pytest.mark.gpu

SENTINEL = -77.25
JD_FIELDS = ("jacp_dot", "jacr_dot", "jdotv")
CE_FIELDS = ("jac_com", "angmom_mat", "bias")
FIELDS = JD_FIELDS + CE_FIELDS
PARITY = {}
MODELS = list(mjx_amd.BUILTIN_MODELS) + ["two_trees", "full"]


def _load(sys_, states):
    d = mjx.make_data(sys_, len(states))
    for i, f in enumerate(("qpos", "qvel", "qacc_warmstart", "ctrl")):
        d.set(f, torch.tensor(np.array([s[i] for s in states]), dtype=torch.float32))
    return d


def _model(name):
    if name == "two_trees":
        m = mjcf.compile_xml_string(tr.TWO_TREES, name)
        return m, generic_states(m, 4)
    if name == "full":
        m = gm.full()
        return m, generic_states(m, 4)
    m = mjx_amd.load_model(name)
    return m, build_states(m)


def _points(m):
    """tests/test_dyn_gpu.py _points: (frames for jac_dot_local, offsets [npoint, 3], (body, body-frame offset))."""
    rng = np.random.default_rng(4)
    frames = [("xbody", b) for b in range(m.nbody)] + [("site", s) for s in range(m.nsite)]
    off = np.zeros((len(frames) + 3, 3))
    frames += [("xbody", b) for b in (1, m.nbody // 2, m.nbody - 1)]
    off[-3:] = rng.uniform(-0.3, 0.3, (3, 3))
    pts = []
    for f, o in zip(frames, off):
        pts.append((f[1], o) if f[0] == "xbody" else
                   (int(m.arrays["site_bodyid"][f[1]]), np.asarray(m.arrays["site_pos"][f[1]], np.float64)))
    return frames, off, pts


def _roots(m):
    return [0, 1, m.nbody // 2, m.nbody - 1]


def _reference(m, outs, states, pts, roots, dtype, mass=None, inertia=None):
    pick = lambda a, e: None if a is None else a[e]
    ref = {f: [] for f in FIELDS}
    for e, (o, st) in enumerate(zip(outs, states)):
        qvel = st[1]
        axes = dr.dof_axes(m, o, dtype)
        rates = tr.dof_rates(m, o, qvel, dtype, axes)
        js = [tr.jac_dot(m, o, b, dr.local_point(o, b, off, dtype), qvel, dtype, axes, rates) for b, off in pts]
        cs = [tr.centroidal(m, o, qvel, b, pick(mass, e), pick(inertia, e), dtype, axes, rates) for b in roots]
        for k, f in enumerate(JD_FIELDS):
            ref[f].append(np.array([j[k] for j in js]))
        for k, f in enumerate(CE_FIELDS):
            ref[f].append(np.array([c[k] for c in cs]))
    return {f: np.array(v) for f, v in ref.items()}


def tolerances(r64, r32):
    tol = {}
    for f in FIELDS:
        yard = float(np.abs(np.float64(r32[f]) - r64[f]).max())
        scale = max(1.0, float(np.abs(r64[f]).max()))
        tol[f] = {"yardstick": yard, "scale": scale, "bound": max(8 * yard, 1e-6 * scale)}
    return tol


@pytest.fixture(scope="module", params=MODELS)
def setup(request):
    name = request.param
    m, states = _model(name)
    orc = Oracle(m)
    outs = [state_arrays(m, orc.forward(orc.new_state(*st))) for st in states]
    frames, off, pts = _points(m)
    roots = _roots(m)
    r64 = _reference(m, outs, states, pts, roots, np.float64)
    r32 = _reference(m, outs, states, pts, roots, np.float32)
    tol = tolerances(r64, r32)
    PARITY[name] = {f: dict(t, worst_gpu_error=0.0) for f, t in tol.items()}
    print(name, "tolerances:", {f: {k: float(f"{v:.3g}") for k, v in t.items()} for f, t in tol.items()})
    return dict(name=name, m=m, sys=mjx.put_model(m), states=states, outs=outs, frames=frames, off=off, pts=pts,
                roots=roots, r64=r64, r32=r32, tol=tol, qvel1=float(max(np.abs(st[1]).sum() for st in states)))


def _err(S, field, got, want):
    """worst |got - want|, recorded for the parity table; returns (err, bound)."""
    got = got.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(got) else got
    err = float(np.abs(got - want).max())
    rec = PARITY[S["name"]][field]
    rec["worst_gpu_error"] = max(rec["worst_gpu_error"], err)
    print(S["name"], field, "yardstick %.3g bound %.3g worst GPU error %.3g" % (rec["yardstick"], rec["bound"], err))
    return err, S["tol"][field]["bound"]


def _bits_zero(t):
    return bool((t.contiguous().view(torch.int32) == 0).all())


def test_jac_dot_parity(setup):
    S = setup
    m, sys_ = S["m"], S["sys"]
    d = _load(sys_, S["states"])
    out = mjx.jac_dot_local(sys_, d, S["frames"], S["off"])
    fails = []
    for f, got in zip(JD_FIELDS, out):
        err, bound = _err(S, f, got, S["r64"][f])
        if err > bound:
            fails.append((f, err, bound))
    # the world frame, fed the points the local Jacobian call reports, reproduces it
    xp = mjx.jac_local(sys_, d, S["frames"], S["off"])[2]
    for f, got in zip(JD_FIELDS, mjx.jac_dot(sys_, d, xp, [b for b, _ in S["pts"]])):
        err, bound = _err(S, f, got, S["r64"][f])
        if err > bound:
            fails.append((f + " (world)", err, bound))
    # npoint = 1 and 3: the odd tail of the two-points-per-pass loop; the same bits as in the full call
    for sel in ([len(S["frames"]) - 1], [2, len(S["frames"]) - 2, 1]):
        sub = mjx.jac_dot_local(sys_, d, [S["frames"][k] for k in sel], S["off"][sel])
        for f, got, full in zip(JD_FIELDS, sub, out):
            assert torch.equal(got, full[:, sel]), (f, sel)
    # jdotv is the matrix product: within its own bound plus the matrices' bound carried through the product
    qvel = d.get("qvel")
    prod = torch.cat([torch.einsum("epiv,ev->epi", out[0], qvel), torch.einsum("epiv,ev->epi", out[1], qvel)], dim=2)
    err = float((prod - out[2]).abs().max())
    bound = S["tol"]["jdotv"]["bound"] + max(S["tol"]["jacp_dot"]["bound"], S["tol"]["jacr_dot"]["bound"]) * S["qvel1"]
    print(S["name"], "jdotv against the matrix products: err %.3g bound %.3g" % (err, bound))
    if err > bound:
        fails.append(("jdotv product", err, bound))
    assert not fails, fails
    assert all(_bits_zero(t[:, 0]) for t in out)  # body 0: zero rows
    if S["name"] == "two_trees":  # the chain's columns are zero for the ball and the other way round
        ball = m.name2id("body", "ball")
        assert (out[0][:, ball, :, :9] == 0).all() and (out[1][:, 1:ball, :, 9:] == 0).all()
        assert float(out[0][:, ball - 1].abs().max()) > 0.1


def test_centroidal_parity(setup):
    S = setup
    m, sys_ = S["m"], S["sys"]
    d = _load(sys_, S["states"])
    out = mjx.centroidal(sys_, d, S["roots"])
    fails = []
    for f, got in zip(CE_FIELDS, out):
        err, bound = _err(S, f, got, S["r64"][f])
        if err > bound:
            fails.append((f, err, bound))
    assert torch.equal(mjx.jac_subtree_com(sys_, d, S["roots"]), out[0])
    assert torch.equal(mjx.angmom_mat(sys_, d, S["roots"]), out[1])
    one = mjx.centroidal(sys_, d)  # the default: the whole model, nsub = 1
    for got, full in zip(one, out):
        assert torch.equal(got[:, 0], full[:, 0])
    # J qvel against body_data's momenta, both on the GPU. Bound: the matrix's bound carried through the product
    # plus the project's bound for a float32 evaluation of the momentum itself (the reference in both precisions)
    qvel = d.get("qvel")
    bd = mjx.body_data(sys_, d, ("subtree_linvel", "subtree_angmom"))
    q64 = np.array([st[1] for st in S["states"]])
    for f, want in (("jac_com", bd.subtree_linvel), ("angmom_mat", bd.subtree_angmom)):
        k = CE_FIELDS.index(f)
        v64 = np.einsum("esiv,ev->esi", S["r64"][f], q64)
        v32 = np.einsum("esiv,ev->esi", S["r32"][f], np.float32(q64))
        bound = S["tol"][f]["bound"] * S["qvel1"] + max(8 * float(np.abs(v32 - v64).max()), 1e-6 * max(1.0, float(np.abs(v64).max())))
        err = float((torch.einsum("esiv,ev->esi", out[k], qvel) - want[:, S["roots"]]).abs().max())
        print(S["name"], f, "qvel against body_data: err %.3g bound %.3g" % (err, bound))
        if err > bound:
            fails.append((f + " qvel", err, bound))
    assert not fails, fails


def test_accelerometer_identity():
    """At a site with an accelerometer, jacp qacc + jdotv[:3] is the site's classical acceleration: R accelerometer
    + gravity of mjl_sensors after a forward, all on the GPU with the qacc that forward stored. Bound: 8 x the
    float32-against-float64 difference of jacp qacc + jdotv[:3] in the numpy references (the oracle's qacc)."""
    m = gm.tail_sensors()
    sys_ = mjx.put_model(m)
    states = build_states(m)
    orc = Oracle(m)
    outs = [state_arrays(m, orc.forward(orc.new_state(*st))) for st in states]
    d = _load(sys_, states)
    sens = mjx.sensors(sys_, d)  # every stage: runs the forward pass
    qacc, xquat = d.get("qacc"), d.get("xquat")
    site = m.name2id("site", "imu_tail")
    body = int(m.arrays["site_bodyid"][site])
    jp = mjx.jac_local(sys_, d, ("site", site))[0][:, 0]
    jdv = mjx.jac_dot_local(sys_, d, ("site", site), out=(None, None, torch.empty(len(states), 1, 6, device="cuda")))[2][:, 0]
    got = torch.einsum("eiv,ev->ei", jp, qacc) + jdv[:, :3]
    Rs = np.asarray(mjcf.quat2mat(np.asarray(m.arrays["site_quat"][site], np.float64))).reshape(3, 3)
    xq = xquat.cpu().numpy().astype(np.float64)
    acc = sens[:, sys_.sensor_slice("accel_tail")].cpu().numpy().astype(np.float64)
    want = np.array([dr._q2m(xq[e, body]) @ Rs @ acc[e] for e in range(len(states))]) + np.asarray(m.gravity, np.float64)
    yard = 0.0
    for st, o in zip(states, outs):
        v = []
        for dt in (np.float32, np.float64):
            x = dr.local_point(o, body, m.arrays["site_pos"][site], dt)
            v.append(np.float64(dr.jac(m, o, body, x, dt)[0] @ np.asarray(o["qacc"], np.float64).astype(dt)
                                + tr.jac_dot(m, o, body, x, st[1], dt)[2][:3]))
        yard = max(yard, float(np.abs(v[0] - v[1]).max()))
    err = float(np.abs(got.cpu().numpy() - want).max())
    print("tail_sensors accelerometer identity: err %.3g bound %.3g scale %.3g" % (err, 8 * yard, np.abs(want).max()))
    assert err <= 8 * yard, (err, 8 * yard)


def test_exact_behaviour(setup):
    S = setup
    m, sys_ = S["m"], S["sys"]
    n, nv, npt, ns = len(S["states"]), m.nv, len(S["frames"]), len(S["roots"])
    d = _load(sys_, S["states"])
    mjx.forward(sys_, d)
    keep = {f: d.get(f).clone() for f in ("qpos", "qvel", "xpos", "xquat", "qacc", "qacc_warmstart", "qfrc_bias")}
    full = lambda *s: torch.full(s, SENTINEL, device="cuda")
    mask = torch.tensor(([1, 0, 1, 1, 0])[:n], dtype=torch.float32, device="cuda")
    jd = mjx.jac_dot_local(sys_, d, S["frames"], S["off"])
    ce = mjx.centroidal(sys_, d, S["roots"])
    # masked envs keep a sentinel
    jm = mjx.jac_dot_local(sys_, d, S["frames"], S["off"], mask=mask, out=(full(n, npt, 3, nv), full(n, npt, 3, nv), full(n, npt, 6)))
    cm = mjx.centroidal(sys_, d, S["roots"], mask=mask, out=(full(n, ns, 3, nv), full(n, ns, 3, nv), full(n, ns, 6)))
    for t, ref in zip(jm + cm, jd + ce):
        assert (t[mask < 0.5] == SENTINEL).all() and torch.equal(t[mask > 0.5], ref[mask > 0.5])
    # every NULL-output combination: the same bits for the remaining outputs
    for pick in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)):
        oj = mjx.jac_dot_local(sys_, d, S["frames"], S["off"], out=tuple(torch.empty_like(t) if p else None for t, p in zip(jd, pick)))
        oc = mjx.centroidal(sys_, d, S["roots"], out=tuple(torch.empty_like(t) if p else None for t, p in zip(ce, pick)))
        for got, ref, p in zip(oj + oc, jd + ce, pick + pick):
            assert (got is None) if not p else torch.equal(got, ref), pick
    # an out-of-range id: NaN rows for that point only (the Python surface refuses it on the host: the C entry)
    L = lib()
    P = lambda t: C.c_void_p(t.data_ptr())
    ids = torch.tensor([1, m.nbody, 2, -1, 0], dtype=torch.int32, device="cuda")
    a, b, c = torch.zeros(n, 5, 3, nv, device="cuda"), torch.zeros(n, 5, 3, nv, device="cuda"), torch.zeros(n, 5, 6, device="cuda")
    assert L.mjl_jac_dot(d.handle, None, 5, P(ids), abi.JAC_FRAME["local"], None, P(a), P(b), P(c), mjx._stream()) == 0
    good = mjx.jac_dot_local(sys_, d, [("xbody", 1), ("xbody", 2), ("xbody", 0)])
    for t, g in zip((a, b, c), good):
        assert torch.isnan(t[:, [1, 3]]).all() and torch.equal(t[:, [0, 2, 4]], g)
    ids = torch.tensor([0, m.nbody + 3, 1], dtype=torch.int32, device="cuda")
    a, b, c = torch.zeros(n, 3, 3, nv, device="cuda"), torch.zeros(n, 3, 3, nv, device="cuda"), torch.zeros(n, 3, 6, device="cuda")
    assert L.mjl_centroidal(d.handle, None, 3, P(ids), P(a), P(b), P(c), mjx._stream()) == 0
    for t, g in zip((a, b, c), ce):
        assert torch.isnan(t[:, 1]).all() and torch.equal(t[:, [0, 2]], g[:, :2])
    # refused calls write nothing
    err = HEADER.enums["MJL_ERR_ARG"]
    s1, s2 = full(n, 3, 3, nv), full(n, 3, 6)
    assert L.mjl_jac_dot(d.handle, None, 3, P(ids), 2, None, P(s1), None, P(s2), mjx._stream()) == err
    assert L.mjl_jac_dot(d.handle, None, 3, P(ids), 0, None, P(s1), None, P(s2), mjx._stream()) == err
    assert L.mjl_centroidal(d.handle, None, 33, P(ids), P(s1), None, P(s2), mjx._stream()) == err
    torch.cuda.synchronize()
    assert (s1 == SENTINEL).all() and (s2 == SENTINEL).all()
    for bad in (-1, m.nbody, "no_such_body"):
        with pytest.raises(ValueError):
            mjx.centroidal(sys_, d, bad)
        with pytest.raises(ValueError):
            mjx.jac_dot(sys_, d, torch.ones(n, 1, 3, device="cuda"), bad)
    # the batch's state and stored derived fields are bit-identical
    for f, t in keep.items():
        assert torch.equal(d.get(f), t), f
    # qvel = 0: every output is +0 bit for bit
    d.set("qvel", torch.zeros(n, nv))
    for t in mjx.jac_dot_local(sys_, d, S["frames"], S["off"]) + mjx.centroidal(sys_, d, S["roots"])[2:]:
        assert _bits_zero(t)
    z = mjx.jac_dot(sys_, d, torch.ones(n, 2, 3, device="cuda"), [1, m.nbody - 1])
    assert all(_bits_zero(t) for t in z)


def test_per_env_parameters(setup):
    S = setup
    m, sys_ = S["m"], S["sys"]
    n = len(S["states"])
    d = _load(sys_, S["states"])
    j0 = mjx.jac_dot_local(sys_, d, S["frames"], S["off"])
    c0 = mjx.centroidal(sys_, d, S["roots"])
    d.enable_model_params(True)
    mass = np.tile(np.float32(m.body_mass), (n, 1))
    inertia = np.tile(np.float32(np.reshape(m.arrays["body_inertia"], (m.nbody, 6))), (n, 1, 1))
    rng = np.random.default_rng(8)
    for e in (1, 2):  # per body, so that centres of mass move
        k = np.float32(rng.uniform(0.5, 1.5, m.nbody))
        mass[e] *= k
        inertia[e] *= k[:, None]
    d.set_model_params(None, body_mass=torch.tensor(mass, device="cuda"), body_inertia=torch.tensor(inertia, device="cuda"))
    j1 = mjx.jac_dot_local(sys_, d, S["frames"], S["off"])
    c1 = mjx.centroidal(sys_, d, S["roots"])
    for a, b in zip(j0, j1):
        assert torch.equal(a, b)  # no geometric field is per-env
    for a, b in zip(c0, c1):
        assert torch.equal(a[0], b[0]) and torch.equal(a[3], b[3])  # nominal envs: bit-identical
    mass64 = [None if e not in (1, 2) else np.float64(mass[e]) for e in range(n)]
    in64 = [None if e not in (1, 2) else np.float64(inertia[e]) for e in range(n)]
    ref = _reference(m, S["outs"], S["states"], S["pts"][:1], S["roots"], np.float64, mass64, in64)
    moved = False
    for k, f in enumerate(CE_FIELDS):
        for e in (1, 2):
            err = float(np.abs(c1[k][e].cpu().numpy() - ref[f][e]).max())
            assert err <= 1.5 * S["tol"][f]["bound"], (f, e, err)  # (the scaled values' magnitudes: at most 1.5 x)
            moved = moved or np.abs(ref[f][e] - S["r64"][f][e]).max() > 10 * S["tol"][f]["bound"]
    assert moved  # the values did move


def test_captured_with_an_env_step(setup):
    S = setup
    if S["name"] not in mjx_amd.BUILTIN_MODELS:
        return  # the env is the humanoid's
    m, sys_ = S["m"], S["sys"]
    B, frames, roots = 8, ["pelvis", ("site", 0), ("xbody", m.nbody - 1)], [0, 2]
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
        eager.append([t.clone() for t in env.jac_dot(frames) + env.centroidal(roots)])
    warm = make()  # warm-up launches outside the capture, on another batch
    warm.step(act, auto_reset=False, counter=2)
    warm.jac_dot(frames)
    warm.centroidal(roots)
    env = make()
    bufs = list(env.jac_dot(frames) + env.centroidal(roots))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.step(act, auto_reset=False, counter=2)
        env.jac_dot(frames)
        env.centroidal(roots)
    for i in range(2):
        g.replay()
        torch.cuda.synchronize()
        for k, want in enumerate(eager[i]):
            assert torch.equal(bufs[k], want), (i, k)
    # a single captured launch replays the eager call bit for bit
    d = env.data
    want = mjx.jac_dot_local(sys_, d, frames)
    out = tuple(torch.zeros_like(t) for t in want)
    tabs = (torch.tensor(mjx.jac_frames(sys_, frames)[0], dtype=torch.int32, device="cuda"),
            torch.tensor(mjx.jac_frames(sys_, frames)[1], device="cuda"))
    torch.cuda.synchronize()
    g1 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g1):
        mjx.jac_dot_local(sys_, d, frames, out=out, _dev=tabs)
    g1.replay()
    torch.cuda.synchronize()
    for a, b in zip(out, want):
        assert torch.equal(a, b)


def test_zz_parity_table():
    """Runs last in this module: the table of every model the tests above covered."""
    assert set(PARITY) == set(MODELS)
    for name, rec in PARITY.items():
        for f, r in rec.items():
            print(name, f, {k: float(f"{v:.3g}") for k, v in r.items()})
    path = os.environ.get("MJX_TASKSPACE_PARITY")
    if path:
        with open(path, "w") as fh:
            json.dump(PARITY, fh, indent=1, sort_keys=True)
