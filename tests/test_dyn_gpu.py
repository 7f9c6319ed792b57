"""Jacobian and mass-matrix readout (mjl_jac / mjl_mass_matrix, mjx.jac / jac_local / full_m / mul_m / solve_m) on
the GPU against tests/dyn_ref.py in fp64.

Batches: the 5 envs of tests/test_bodydata.py build_states for both humanoids, 4 random states for the two-tree
model below (a free 3-link hinge chain and a second free sphere: the dof masks keep the trees apart) and for
generic_models.full() (nv = 32 fills every dof lane).

Tolerances (the rule of tests/test_bodydata_gpu.py tolerances): per field the yardstick is max |dyn_ref in float32 -
in float64| over the states; the kernel gets bound = max(8 x yardstick, 1e-6 x max(1, scale)), scale = max |value|.
The figures are printed (pytest -s) and, with MJX_DYN_PARITY=<path> in the environment, written there as JSON
(profiles/dyn/parity.json is such a run)."""
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
from test_bodydata import build_states
from test_dyn import generic_states

pytestmark = pytest.mark.gpu

SENTINEL = -77.25
FIELDS = ("jacp", "jacr", "xpnt", "full_m", "mul_m", "solve_m")
PARITY = {}

TWO_TREES = """
<mujoco model="two_trees">
  <option timestep="0.004"/>
  <worldbody>
    <geom name="floor" type="plane" size="0 0 1"/>
    <body name="a0" pos="0 0 1"><freejoint/>
      <geom type="capsule" fromto="0 0 0 0.2 0 0" size="0.03"/>
      <body name="a1" pos="0.2 0 0">
        <joint name="h1" type="hinge" axis="0 1 0" pos="0.01 0 0" armature="0.02"/>
        <geom type="capsule" fromto="0 0 0 0.2 0 0.05" size="0.03"/>
        <body name="a2" pos="0.2 0 0.05" quat="0.9 0.1 0.3 -0.2">
          <joint name="h2" type="hinge" axis="1 0 0.3"/>
          <geom type="capsule" fromto="0 0 0 0.15 0.05 0" size="0.025"/>
          <body name="a3" pos="0.15 0.05 0">
            <joint name="h3" type="hinge" axis="0 0 1" pos="0 0.01 0"/>
            <geom type="capsule" fromto="0 0 0 0.1 0.1 0.1" size="0.02"/>
            <site name="tip" pos="0.1 0.1 0.1" quat="0.7 0.1 -0.5 0.5" size="0.01"/>
          </body>
        </body>
      </body>
    </body>
    <body name="ball" pos="0.5 0.5 1"><freejoint/><geom type="sphere" size="0.1"/></body>
  </worldbody>
  <actuator><motor name="m1" joint="h1" gear="5"/></actuator>
</mujoco>
"""


def _load(sys_, states):
    d = mjx.make_data(sys_, len(states))
    for i, f in enumerate(("qpos", "qvel", "qacc_warmstart", "ctrl")):
        d.set(f, torch.tensor(np.array([s[i] for s in states]), dtype=torch.float32))
    return d


def _model(name):
    if name == "two_trees":
        m = mjcf.compile_xml_string(TWO_TREES, name)
        return m, generic_states(m, 4)
    if name == "full":
        m = gm.full()
        return m, generic_states(m, 4)
    m = mjx_amd.load_model(name)
    return m, build_states(m)


def _points(m):
    """(frames for jac_local, offsets [npoint, 3], (body, body-frame offset) per point): every body origin, every
    site, three bodies with an offset."""
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


def _reference(m, outs, pts, vecs, dtype, mass=None, inertia=None, armature=None):
    pick = lambda a, e: None if a is None else a[e]
    ref = {f: [] for f in FIELDS}
    for e, o in enumerate(outs):
        axes = dr.dof_axes(m, o, dtype)
        xs = [dr.local_point(o, b, off, dtype) for b, off in pts]
        js = [dr.jac(m, o, b, x, dtype, axes) for (b, _), x in zip(pts, xs)]
        M = dr.mass_matrix(m, o, pick(mass, e), pick(inertia, e), pick(armature, e), dtype)
        v = np.asarray(vecs[e], np.float64).astype(dtype)
        ref["jacp"].append(np.array([j[0] for j in js]))
        ref["jacr"].append(np.array([j[1] for j in js]))
        ref["xpnt"].append(np.array(xs))
        ref["full_m"].append(M)
        ref["mul_m"].append(v @ M.T)
        ref["solve_m"].append(dr.solve(M, v, dtype))
    return {f: np.array(v) for f, v in ref.items()}


def tolerances(r64, r32):
    tol = {}
    for f in FIELDS:
        yard = float(np.abs(np.float64(r32[f]) - r64[f]).max())
        scale = max(1.0, float(np.abs(r64[f]).max()))
        tol[f] = {"yardstick": yard, "scale": scale, "bound": max(8 * yard, 1e-6 * scale)}
    return tol


MODELS = list(mjx_amd.BUILTIN_MODELS) + ["two_trees", "full"]


@pytest.fixture(scope="module", params=MODELS)
def setup(request):
    name = request.param
    m, states = _model(name)
    orc = Oracle(m)
    outs = [state_arrays(m, orc.forward(orc.new_state(*st))) for st in states]
    frames, off, pts = _points(m)
    vecs = np.float32(np.random.default_rng(6).uniform(-1, 1, (len(states), 5, m.nv))).astype(np.float64)
    r64 = _reference(m, outs, pts, vecs, np.float64)
    tol = tolerances(r64, _reference(m, outs, pts, vecs, np.float32))
    PARITY[name] = {f: dict(t, worst_gpu_error=0.0) for f, t in tol.items()}
    print(name, "tolerances:", {f: {k: float(f"{v:.3g}") for k, v in t.items()} for f, t in tol.items()})
    return dict(name=name, m=m, sys=mjx.put_model(m), states=states, outs=outs, frames=frames, off=off, pts=pts,
                vecs=vecs, r64=r64, tol=tol)


def _err(S, field, got, want, envs=None):
    """worst |got - want| over `envs`, recorded for the parity table; returns (err, bound)."""
    got = got.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(got) else got
    e = slice(None) if envs is None else envs
    err = float(np.abs(got[e] - want[e]).max())
    rec = PARITY[S["name"]][field]
    rec["worst_gpu_error"] = max(rec["worst_gpu_error"], err)
    print(S["name"], field, "yardstick %.3g bound %.3g worst GPU error %.3g" % (rec["yardstick"], rec["bound"], err))
    return err, S["tol"][field]["bound"]


def test_jacobian_parity(setup):
    S = setup
    m, sys_ = S["m"], S["sys"]
    d = _load(sys_, S["states"])
    jp, jr, xp = mjx.jac_local(sys_, d, S["frames"], S["off"])
    fails = []
    for f, got in (("jacp", jp), ("jacr", jr), ("xpnt", xp)):
        err, bound = _err(S, f, got, S["r64"][f])
        if err > bound:
            fails.append((f, err, bound))
    # the world frame, fed the points the local call reported, reproduces it
    bodies = [b for b, _ in S["pts"]]
    wp, wr = mjx.jac(sys_, d, xp, bodies)
    for f, got in (("jacp", wp), ("jacr", wr)):
        err, bound = _err(S, f, got, S["r64"][f])
        if err > bound:
            fails.append((f + " (world)", err, bound))
    assert not fails, fails
    assert (jp[:, 0] == 0).all() and (jr[:, 0] == 0).all()  # body 0: zero rows
    if S["name"] == "two_trees":  # the chain's columns are zero for the ball and the other way round
        ball = m.name2id("body", "ball")
        assert (jp[:, ball, :, :9] == 0).all() and (jr[:, ball, :, :9] == 0).all()
        assert (jp[:, 1:ball, :, 9:] == 0).all() and (jr[:, 1:ball, :, 9:] == 0).all()
        assert float(jp[:, ball, :, 9:].abs().max()) == 1.0 and float(jr[:, ball - 1, :, :9].abs().max()) > 0.5


def test_velocity_consistency():
    """jacp qvel / jacr qvel against the sensors' framelinvel / frameangvel (site and body frames) and against
    body_data's cvel moved to the point, all on the GPU. Tolerance: the sum of the two readouts' bounds, each the
    project's bound for a float32 evaluation of that velocity: for the Jacobian bound(jac) |qvel|_1, for the other
    readout max(8 x |v32 - v64|, 1e-6 max(1, |v|)) with v = J qvel from dyn_ref in both precisions."""
    m = gm.tail_sensors()
    sys_ = mjx.put_model(m)
    states = build_states(m)
    orc = Oracle(m)
    outs = [state_arrays(m, orc.forward(orc.new_state(*st))) for st in states]
    d = _load(sys_, states)
    qvel = d.get("qvel")
    sens = mjx.sensors(sys_, d, stages=abi.SENSOR_STAGE["pos"] | abi.SENSOR_STAGE["vel"])
    frames = ["imu_tail", "tail3"] + [("xbody", b) for b in range(1, m.nbody)]
    jp, jr, xp = mjx.jac_local(sys_, d, frames)
    vp, vr = torch.einsum("epiv,ev->epi", jp, qvel), torch.einsum("epiv,ev->epi", jr, qvel)
    bodies, local = mjx.jac_frames(sys_, frames)

    def bound(k, rot):
        worst = 0.0
        for e, o in enumerate(outs):
            v = []
            for dt in (np.float32, np.float64):
                x = dr.local_point(o, bodies[k], local[k], dt)
                j = dr.jac(m, o, bodies[k], x, dt)[rot]
                v.append(np.float64(j @ np.asarray(states[e][1]).astype(dt)))
            jb = max(8 * np.abs(dr.jac(m, o, bodies[k], x, np.float32)[rot] - dr.jac(m, o, bodies[k], x)[rot]).max(), 1e-6)
            worst = max(worst, jb * np.abs(states[e][1]).sum() + max(8 * np.abs(v[0] - v[1]).max(), 1e-6 * max(1.0, np.abs(v[1]).max())))
        return worst
    for k, (got, name, rot) in enumerate(((vr[:, 0], "fa_site", 1), (vp[:, 1], "fl_tail3", 0))):
        err = float((got - sens[:, sys_.sensor_slice(name)]).abs().max())
        print("tail_sensors", name, "err", err, "bound", bound(k, rot))
        assert err <= bound(k, rot), (name, err)
    bd = mjx.body_data(sys_, d, ("subtree_com", "cvel"))
    root = torch.tensor([int(r) for r in m.arrays["body_rootid"]], device="cuda")
    for k, b in enumerate(range(1, m.nbody), start=2):
        c0 = bd.subtree_com[:, root[b]]
        lin = bd.cvel[:, b, 3:] + torch.linalg.cross(bd.cvel[:, b, :3], xp[:, k] - c0)
        e_lin, e_ang = float((vp[:, k] - lin).abs().max()), float((vr[:, k] - bd.cvel[:, b, :3]).abs().max())
        assert e_lin <= bound(k, 0) and e_ang <= bound(k, 1), (b, e_lin, e_ang, bound(k, 0), bound(k, 1))


@pytest.mark.parametrize("nvec", [1, 5])
def test_mass_matrix(setup, nvec):
    S = setup
    m, sys_ = S["m"], S["sys"]
    d = _load(sys_, S["states"])
    M = mjx.full_m(sys_, d)
    assert torch.equal(M, M.transpose(1, 2))  # symmetric bit for bit
    v = torch.tensor(S["vecs"][:, :nvec], dtype=torch.float32, device="cuda")
    arg = v[:, 0] if nvec == 1 else v
    y, x = mjx.mul_m(sys_, d, arg), mjx.solve_m(sys_, d, arg)
    assert y.shape == arg.shape and x.shape == arg.shape
    M64 = np.array([o["M"] for o in S["outs"]])
    fails = []
    for f, got, want in (("full_m", M, M64), ("mul_m", y.view(len(M64), nvec, -1), S["r64"]["mul_m"][:, :nvec]),
                         ("solve_m", x.view(len(M64), nvec, -1), S["r64"]["solve_m"][:, :nvec])):
        err, bound = _err(S, f, got, want)
        if err > bound:
            fails.append((f, err, bound))
    x64 = x.view(len(M64), nvec, -1).cpu().numpy().astype(np.float64)
    res = np.linalg.norm(np.einsum("eij,ekj->eki", M64, x64) - S["vecs"][:, :nvec], axis=-1) / np.linalg.norm(S["vecs"][:, :nvec], axis=-1)
    PARITY[S["name"]]["solve_m"]["relative_residual"] = max(PARITY[S["name"]]["solve_m"].get("relative_residual", 0.0), float(res.max()))
    print(S["name"], "solve_m relative residual |M64 x - v| / |v|:", float(res.max()))
    assert not fails, fails
    if S["name"] == "two_trees":
        assert (M[:, :9, 9:] == 0).all()


def test_per_env_parameters(setup):
    S = setup
    m, sys_ = S["m"], S["sys"]
    n = len(S["states"])
    d = _load(sys_, S["states"])
    M0 = mjx.full_m(sys_, d)
    j0 = mjx.jac_local(sys_, d, S["frames"], S["off"])
    d.enable_model_params(True)
    mass = np.tile(np.float32(m.body_mass), (n, 1))
    inertia = np.tile(np.float32(np.reshape(m.arrays["body_inertia"], (m.nbody, 6))), (n, 1, 1))
    arm = np.tile(np.float32(m.arrays["dof_armature"]), (n, 1))
    for e, k in ((1, 1.5), (2, 0.75)):
        mass[e] *= np.float32(k)
        inertia[e] *= np.float32(k)
        arm[e] = arm[e] * np.float32(k) + np.float32(0.01)
    d.set_model_params(None, body_mass=torch.tensor(mass, device="cuda"), body_inertia=torch.tensor(inertia, device="cuda"),
                       dof_armature=torch.tensor(arm, device="cuda"))
    M1 = mjx.full_m(sys_, d)
    j1 = mjx.jac_local(sys_, d, S["frames"], S["off"])
    assert torch.equal(M1[0], M0[0]) and torch.equal(M1[3], M0[3])  # nominal envs: bit-identical
    for a, b in zip(j0, j1):
        assert torch.equal(a, b)
    for e in (1, 2):
        want = dr.mass_matrix(m, S["outs"][e], np.float64(mass[e]), np.float64(inertia[e]), np.float64(arm[e]))
        err = float(np.abs(M1[e].cpu().numpy() - want).max())
        assert err <= 1.5 * S["tol"]["full_m"]["bound"], (e, err)  # (the scaled values' magnitudes: at most 1.5 x)
        assert np.abs(want - S["r64"]["full_m"][e]).max() > 10 * S["tol"]["full_m"]["bound"]  # the values did move


def test_mask_null_outputs_untouched_state(setup):
    S = setup
    m, sys_ = S["m"], S["sys"]
    n = len(S["states"])
    d = _load(sys_, S["states"])
    mjx.forward(sys_, d)
    keep = {f: d.get(f).clone() for f in ("qpos", "qvel", "xpos", "xquat", "qacc")}
    mask = torch.tensor(([1, 0, 1, 1, 0])[:n], dtype=torch.float32, device="cuda")
    npt, nv = len(S["frames"]), m.nv
    full = lambda *s: torch.full(s, SENTINEL, device="cuda")
    out = (full(n, npt, 3, nv), full(n, npt, 3, nv), full(n, npt, 3))
    mjx.jac_local(sys_, d, S["frames"], S["off"], mask=mask, out=out)
    v = torch.tensor(S["vecs"], dtype=torch.float32, device="cuda")
    mo = (mjx.full_m(sys_, d, mask, full(n, nv, nv)), mjx.mul_m(sys_, d, v, mask, full(n, 5, nv)),
          mjx.solve_m(sys_, d, v, mask, full(n, 5, nv)))
    for t in out + mo:
        assert (t[mask < 0.5] == SENTINEL).all() and not (t[mask > 0.5] == SENTINEL).any()
    # each output alone equals the same output requested with the others
    both = mjx.jac_local(sys_, d, S["frames"], S["off"])
    onlyp = mjx.jac_local(sys_, d, S["frames"], S["off"], out=(torch.empty_like(both[0]), None, None))
    onlyr = mjx.jac_local(sys_, d, S["frames"], S["off"], out=(None, torch.empty_like(both[1]), None))
    assert onlyp[1] is None and onlyp[2] is None and torch.equal(onlyp[0], both[0]) and torch.equal(onlyr[1], both[1])
    M, y, x = (torch.empty(n, nv, nv, device="cuda"), torch.empty(n, 5, nv, device="cuda"), torch.empty(n, 5, nv, device="cuda"))
    mjx._mass_matrix(sys_, d, None, M, v, y, x)
    assert torch.equal(M, mjx.full_m(sys_, d)) and torch.equal(y, mjx.mul_m(sys_, d, v)) and torch.equal(x, mjx.solve_m(sys_, d, v))
    for f, t in keep.items():
        assert torch.equal(d.get(f), t), f
    # straight after a step, without a forward: the Jacobian of the post-step qpos
    mjx.step(sys_, d)
    jp, jr, xp = mjx.jac_local(sys_, d, S["frames"], S["off"])
    q = d.get("qpos").cpu().numpy().astype(np.float64)
    orc = Oracle(m)
    outs = [state_arrays(m, orc.forward(orc.new_state(q[e]))) for e in range(n)]
    ref = _reference(m, outs, S["pts"], S["vecs"], np.float64)
    for f, got in (("jacp", jp), ("jacr", jr), ("xpnt", xp)):
        err = float(np.abs(got.cpu().numpy() - ref[f]).max())
        assert err <= S["tol"][f]["bound"], (f, err)
    assert np.abs(ref["xpnt"] - S["r64"]["xpnt"]).max() > 100 * S["tol"]["xpnt"]["bound"]  # the state did move


def test_world_body_and_bad_arguments(setup):
    S = setup
    m, sys_ = S["m"], S["sys"]
    n, nv = len(S["states"]), m.nv
    d = _load(sys_, S["states"])
    jp, jr = mjx.jac(sys_, d, torch.ones(n, 1, 3, device="cuda"), 0)
    assert (jp == 0).all() and (jr == 0).all()
    for bad in (-1, m.nbody, "no_such_body"):
        with pytest.raises(ValueError):
            mjx.jac(sys_, d, torch.ones(n, 1, 3, device="cuda"), bad)
    with pytest.raises(ValueError):
        mjx.jac_local(sys_, d, [("xbody", m.nbody)])
    L, err = lib(), HEADER.enums["MJL_ERR_ARG"]
    P = lambda t: C.c_void_p(t.data_ptr())
    body = torch.zeros(2, dtype=torch.int32, device="cuda")
    pnt = torch.zeros(n, 2, 3, device="cuda")
    a, b, x = (torch.full((n, 2, 3, nv), SENTINEL, device="cuda"), torch.full((n, 2, 3, nv), SENTINEL, device="cuda"),
               torch.full((n, 2, 3), SENTINEL, device="cuda"))
    h, st = d.handle, mjx._stream()
    cases = [L.mjl_jac(None, None, 2, P(body), 0, P(pnt), P(a), P(b), P(x), st),
             L.mjl_jac(h, None, 2, None, 0, P(pnt), P(a), P(b), P(x), st),
             L.mjl_jac(h, None, 2, P(body), 0, P(pnt), None, None, P(x), st),
             L.mjl_jac(h, None, 0, P(body), 0, P(pnt), P(a), P(b), P(x), st),
             L.mjl_jac(h, None, 257, P(body), 0, P(pnt), P(a), P(b), P(x), st),
             L.mjl_jac(h, None, 2, P(body), 2, P(pnt), P(a), P(b), P(x), st),
             L.mjl_jac(h, None, 2, P(body), 0, None, P(a), P(b), P(x), st)]
    M, v, y = (torch.full((n, nv, nv), SENTINEL, device="cuda"), torch.zeros(n, 1, nv, device="cuda"),
               torch.full((n, 1, nv), SENTINEL, device="cuda"))
    cases += [L.mjl_mass_matrix(None, None, P(M), 0, None, None, None, st),
              L.mjl_mass_matrix(h, None, None, 1, P(v), None, None, st),
              L.mjl_mass_matrix(h, None, P(M), 65, P(v), P(y), None, st),
              L.mjl_mass_matrix(h, None, P(M), -1, None, None, None, st),
              L.mjl_mass_matrix(h, None, P(M), 1, None, P(y), None, st),
              L.mjl_mass_matrix(h, None, P(M), 0, P(v), None, P(y), st)]
    for i, rc in enumerate(cases):
        assert rc == err, (i, rc)
    assert L.mjl_jac(h, None, 2, P(body), 2, P(pnt), P(a), P(b), P(x), st) == err and len(L.mjl_last_error()) > 10
    torch.cuda.synchronize()
    for t in (a, b, x, M, y):
        assert (t == SENTINEL).all()


def test_captured_with_an_env_step(setup):
    S = setup
    if S["name"] not in mjx_amd.BUILTIN_MODELS:
        return  # the env is the humanoid's
    m, sys_ = S["m"], S["sys"]
    B, frames = 8, ["pelvis", ("site", 0), ("xbody", m.nbody - 1)]
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
        eager.append([t.clone() for t in env.jac(frames)] + [env.full_m().clone()])
    warm = make()  # warm-up launches outside the capture, on another batch
    warm.step(act, auto_reset=False, counter=2)
    warm.jac(frames)
    warm.full_m()
    env = make()
    bufs = list(env.jac(frames)) + [env.full_m()]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.step(act, auto_reset=False, counter=2)
        env.jac(frames)
        env.full_m()
    for i in range(2):
        g.replay()
        torch.cuda.synchronize()
        for k, want in enumerate(eager[i]):
            assert torch.equal(bufs[k], want), (i, k)


def test_zz_parity_table():
    """Runs last in this module: the table of every model the tests above covered."""
    assert set(PARITY) == set(MODELS)
    for name, rec in PARITY.items():
        for f, r in rec.items():
            print(name, f, {k: float(f"{v:.3g}") for k, v in r.items()})
    path = os.environ.get("MJX_DYN_PARITY")
    if path:
        with open(path, "w") as fh:
            json.dump(PARITY, fh, indent=1, sort_keys=True)
