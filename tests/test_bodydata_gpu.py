"""Body-level readout (mjl_body_data / mjx.body_data) on the GPU against tests/bodydata_ref.py in fp64.

Batch: 5 envs (tests/test_bodydata.py build_states: falls with foot and body contacts, states in the air), mask
[1,0,1,1,0]. Models: both humanoids and the fixed-base chain of tests/test_bodydata.py (a body whose centre of
mass is off its origin and whose principal axes are not the body's).

Tolerances: per field the yardstick is max |bodydata_ref in float32 - in float64| over the states; the kernel gets
8 x that (summation order, fused multiply-adds, quaternions instead of matrices), at least 1e-6 x the field's scale
(max |value| over the states, at least 1). cfrc_ext / cfrc_int also inherit the forward pass's error when compared
with the reference fed by the ORACLE's qacc and contacts, at the existing parity tolerances (tests/test_gpu_parity.py:
2e-3 (1 + max |ref|) for qacc and for efc_force-derived values): with te / tq those two figures, L the largest
distance of a load's point from c0 (at least 1), per body cfrc_ext <= ncon 3 te 2 L (three frame rows per
component, the lever arm for the torque) and cfrc_int <= sum over the model of that + M nv tq L^2 (every dof
moves every body's centre by at most L per unit qacc). Those bounds are loose, so, as test_sensors_gpu does for the
accelerometer, both fields are also compared with the reference fed by what the call's own forward pass stored
(qacc read back, contacts from forward_contacts of the same state) at the 8 x yardstick bound alone: the forward's
error is out and the readout's own arithmetic is checked at float32 resolution. ximat: bodydata_ref.check_ximat.
The table this prints (pytest -s) is in DESIGN.md "Body data"."""
import dataclasses

import numpy as np
import pytest
import torch

import mjx_amd
from mjx_amd import abi, mjcf, mjx
from mjx_amd.config import reference_ppo_config
from mjx_amd.envs import HumanoidEnv, gym_humanoid_obs, resolve_ids
from oracle import Oracle, state_arrays

import bodydata_ref as br
from test_bodydata import BALANCE_BOUND, CHAIN, NENV, build_states, chain_states

pytestmark = pytest.mark.gpu

MASK = np.array([1, 0, 1, 1, 0], np.float32)
SENTINEL = -77.25
ALL = tuple(mjx.BODY_FIELDS)
POSVEL = ALL[:7]


def _load(sys_, states):
    d = mjx.make_data(sys_, len(states))
    for i, f in enumerate(("qpos", "qvel", "qacc_warmstart", "ctrl")):
        d.set(f, torch.tensor(np.array([s[i] for s in states]), dtype=torch.float32))
    return d


def _np(bd):
    return {f: getattr(bd, f).cpu().numpy().astype(np.float64) for f in ALL if getattr(bd, f) is not None}


def _refs(m, states, xfrc=None, mass=None, inertia=None):
    orc = Oracle(m)
    outs = [state_arrays(m, orc.forward(orc.new_state(*st))) for st in states]
    pick = lambda a, e: None if a is None else a[e]
    r64 = [br.body_data(m, o, None if xfrc is None else xfrc[e], pick(mass, e), pick(inertia, e)) for e, o in enumerate(outs)]
    r32 = [br.body_data(m, o, None if xfrc is None else xfrc[e], pick(mass, e), pick(inertia, e), np.float32)
           for e, o in enumerate(outs)]
    return outs, r64, r32


def tolerances(r64, r32):
    tol = {}
    for f in br.FIELDS:
        yard = max(float(np.abs(np.float64(a[f]) - b[f]).max()) for a, b in zip(r32, r64))
        scale = max(1.0, max(float(np.abs(b[f]).max()) for b in r64))
        tol[f] = {"yardstick": yard, "scale": scale, "bound": max(8 * yard, 1e-6 * scale)}
    return tol


def inherited(m, o, ref):
    """(cfrc_ext, cfrc_int) terms of one state: the forward pass's error at the parity tolerances (docstring)."""
    te = 2e-3 * (1 + (np.abs(o["efc_force"]).max() if len(o["efc_force"]) else 0.0))
    tq = 2e-3 * (1 + np.abs(o["qacc"]).max())
    c0 = ref["subtree_com"][[int(r) for r in m.arrays["body_rootid"]]]
    L = max(1.0, float(np.abs(ref["xipos"] - c0).max()),
            max((float(np.abs(p - c0[1:]).max()) for p in o["con_pos"]), default=0.0))
    ext = int(o["ncon"]) * 3 * te * 2 * L
    return ext, m.nbody * ext + float(np.sum(m.arrays["body_mass"])) * m.nv * tq * L * L


def stored_forward(sys_, d, states):
    """(contacts, qacc) of the forward pass the readout ran: a forward pass leaves its solution in qacc_warmstart,
    so the state's own warm start is put back first and the same pass runs again, bit for bit."""
    d.set("qacc_warmstart", torch.tensor(np.array([s[2] for s in states]), dtype=torch.float32))
    c = mjx.forward_contacts(sys_, d)
    return c, d.get("qacc").cpu().numpy().astype(np.float64)


def stored_inputs(m, c, qacc, o, e):
    """The oracle-shaped forward outputs of env e as the GPU's own forward pass left them."""
    n = int(c.ncon[e])
    fw = c.force[e, :n].cpu().numpy().astype(np.float64)
    rows, typ = [], []
    mu = {(int(a), int(b)): m.pair_friction[p][0] for p, (a, b) in enumerate(zip(m.pair_geom1, m.pair_geom2))}
    for j in range(n):  # rows whose contact-frame force is the stored one
        if int(c.dim[e, j]) == 1:
            rows += [fw[j, 0]]
            typ += [2]
        else:
            k = mu[tuple(int(x) for x in c.geom[e, j])]
            typ += [3] * 4
            # the normal force is the four rows' sum: split it so that the sum and both differences hold
            rows += [0.0] * 4
            rows[-4:] = [fw[j, 0] / 4 + fw[j, 1] / (2 * k), fw[j, 0] / 4 - fw[j, 1] / (2 * k),
                         fw[j, 0] / 4 + fw[j, 2] / (2 * k), fw[j, 0] / 4 - fw[j, 2] / (2 * k)]
    return dict(o, qacc=qacc[e], ncon=n,
                con_pos=c.pos[e, :n].cpu().numpy().astype(np.float64),
                con_frame=c.frame[e, :n].reshape(n, 9).cpu().numpy().astype(np.float64),
                con_geom=c.geom[e, :n].cpu().numpy(), efc_force=np.array(rows), efc_type=np.array(typ, np.int32))


MODELS = list(mjx_amd.BUILTIN_MODELS) + ["bd_chain"]


@pytest.fixture(scope="module", params=MODELS)
def setup(request):
    name = request.param
    if name == "bd_chain":
        m = mjcf.compile_xml_string(CHAIN, name)
        states = chain_states(m)
    else:
        m = mjx_amd.load_model(name)
        states = build_states(m)
    outs, r64, r32 = _refs(m, states)
    tol = tolerances(r64, r32)
    print(name, "tolerances:", {f: {k: float(f"{v:.3g}") for k, v in t.items()} for f, t in tol.items()})
    return name, m, mjx.put_model(m), states, outs, r64, tol


def _check(name, m, sys_, d, states, got, outs, r64, tol, envs, what):
    worst = {}
    c, qacc = stored_forward(sys_, d, states)
    geoms = c.geom.cpu().numpy()
    differ = [e for e in range(NENV) if sorted(map(tuple, geoms[e][geoms[e, :, 0] >= 0])) !=
              sorted(tuple(int(x) for x in g) for g in outs[e]["con_geom"])]
    assert len(differ) <= 1, differ
    for e in envs:
        for f in br.FIELDS:
            bound = tol[f]["bound"]
            if f in ("cfrc_ext", "cfrc_int"):
                if e in differ:
                    continue
                bound += inherited(m, outs[e], r64[e])[f == "cfrc_int"]
            err = float(np.abs(got[f][e] - r64[e][f]).max())
            worst[f] = max(worst.get(f, 0.0), err / bound)
            assert err <= bound, f"{what} env {e} {f}: err {err:.3e} > {bound:.3e}"
        so = stored_inputs(m, c, qacc, outs[e], e)
        ref = br.body_data(m, so)
        for f in ("cfrc_ext", "cfrc_int"):
            err = float(np.abs(got[f][e] - ref[f]).max())
            worst[f + "@stored"] = max(worst.get(f + "@stored", 0.0), err / tol[f]["bound"])
            assert err <= tol[f]["bound"], f"{what} env {e} {f} on the stored forward: err {err:.3e} > {tol[f]['bound']:.3e}"
        wx = br.check_ximat(m, outs[e], got["ximat"][e], 2e-6)
        worst["ximat"] = max(worst.get("ximat", 0.0), wx / 2e-6)
    print(what, "worst err / bound:", {k: round(v, 3) for k, v in worst.items()})


def test_parity_masked_and_unmasked(setup):
    name, m, sys_, states, outs, r64, tol = setup
    d = _load(sys_, states)
    out = mjx.BodyData(**{f: torch.full((NENV, m.nbody) + s, SENTINEL, device="cuda") for f, s in mjx.BODY_FIELDS.items()})
    mjx.body_data(sys_, d, ALL, mask=torch.tensor(MASK), out=out)
    for f in ALL:
        assert (getattr(out, f)[MASK < 0.5] == SENTINEL).all(), f
    fresh = mjx.body_data(sys_, _load(sys_, states), ("subtree_com",), mask=torch.tensor(MASK))
    assert (fresh.subtree_com[MASK < 0.5] == 0).all() and fresh.cvel is None
    _check(name, m, sys_, d, states, _np(out), outs, r64, tol, np.flatnonzero(MASK > 0.5), f"{name} masked")
    d = _load(sys_, states)
    got = _np(mjx.body_data(sys_, d, ALL))
    _check(name, m, sys_, d, states, got, outs, r64, tol, range(NENV), name)
    for f in ("cinert", "cvel", "cfrc_ext", "cfrc_int"):
        assert (got[f][:, 0] == 0).all(), f


def test_direct_oracle_pins(setup):
    """xipos, subtree_com, cinert, cvel against the oracle's own fp64 arrays (not through bodydata_ref)."""
    name, m, sys_, states, outs, r64, tol = setup
    got = _np(mjx.body_data(sys_, _load(sys_, states), ("xipos", "subtree_com", "cinert", "cvel")))
    orc = Oracle(m)
    for e, st in enumerate(states):
        s = orc.forward(orc.new_state(*st))
        a = state_arrays(m, s)
        for f, want in (("xipos", a["xipos"]), ("subtree_com", a["subtree_com"]), ("cinert", np.array(s.cinert)[:m.nbody]),
                        ("cvel", a["cvel"])):
            err = float(np.abs(got[f][e] - want).max())
            assert err <= tol[f]["bound"], f"{name} env {e} {f}: err {err:.3e} > {tol[f]['bound']:.3e}"


@pytest.mark.parametrize("applied", [False, True])
def test_momentum_balance_on_the_kernel(setup, applied):
    """cfrc_int of the free root is ~0 against sum |cfrc_ext| + M |g|: the CPU test's bound plus the float32 term
    (cfrc_int's 8 x yardstick bound over the scale); `applied`: 200 N on a hand, attached."""
    name, m, sys_, states, outs, r64, tol = setup
    if name == "bd_chain":
        return  # the balance is a free root's
    d = _load(sys_, states)
    if applied:
        hand = max(b for b, n in enumerate(m.names["body"]) if "hand" in n or "lower_arm" in n)
        xfrc = torch.zeros((NENV, m.nbody, 6), device="cuda")
        xfrc[:, hand, :3] = torch.tensor([120.0, -100.0, 124.9], device="cuda")  # 200 N
        assert abs(float(xfrc[0, hand, :3].norm()) - 200.0) < 0.1 and int(m.arrays["body_rootid"][hand]) == 1 and hand > 1
        d.attach_applied(None, xfrc)
    bd = _np(mjx.body_data(sys_, d, ("cfrc_ext", "cfrc_int")))
    ncon = d.get("stats")[:, 0].cpu().numpy()
    assert (ncon > 0).sum() >= 3
    if applied:
        assert np.abs(bd["cfrc_ext"][:, hand, 3:] ).max() >= 100.0
    for e in range(NENV):
        scale = np.abs(bd["cfrc_ext"][e]).sum() + float(np.sum(m.body_mass)) * np.linalg.norm(m.gravity)
        res = np.abs(bd["cfrc_int"][e, 1]).max() / scale
        bound = BALANCE_BOUND + tol["cfrc_int"]["bound"] / scale
        print(name, "applied" if applied else "plain", "env", e, "residual / scale", res, "bound", bound)
        assert res <= bound, (e, res, bound)


def test_static_chain():
    """qvel = 0: the world-attached link's cfrc_int force is sum_k m_k (a_k - g), recomputed from the reference
    kinematics on the qacc the forward stored; nothing external acts, so cfrc_ext is zero."""
    m = mjcf.compile_xml_string(CHAIN, "bd_chain")
    sys_ = mjx.put_model(m)
    states = [(q, 0 * v, w, c) for q, v, w, c in chain_states(m)]
    outs, r64, r32 = _refs(m, states)
    tol = tolerances(r64, r32)
    d = _load(sys_, states)
    bd = _np(mjx.body_data(sys_, d, ("cfrc_ext", "cfrc_int")))
    qacc = d.get("qacc").cpu().numpy().astype(np.float64)
    import sensors_ref as sr
    for e, (q, v, w, c) in enumerate(states):
        assert outs[e]["ncon"] == 0
        k = sr.kinematics(m, q, v, qacc[e])
        want = np.zeros(3)
        for b in range(1, m.nbody):
            dd = k["R"][b] @ np.asarray(m.arrays["body_ipos"][b])
            a = k["a"][b] + np.cross(k["dw"][b], dd) + np.cross(k["w"][b], np.cross(k["w"][b], dd))
            want += m.body_mass[b] * (a - np.asarray(m.gravity))
        assert np.abs(want).max() > 1.0
        assert np.abs(bd["cfrc_int"][e, 1, 3:] - want).max() <= tol["cfrc_int"]["bound"]
        assert (bd["cfrc_ext"][e] == 0).all()


def test_per_env_parameters(setup):
    name, m, sys_, states, outs, r64, tol = setup
    fields = ("subtree_com", "cinert", "subtree_angmom")
    d = _load(sys_, states)
    before = mjx.body_data(sys_, d, fields)
    d.enable_model_params(True)
    bodies = [1, m.nbody // 2, m.nbody - 1]
    mass = np.tile(np.float32(m.body_mass), (NENV, 1))
    inertia = np.tile(np.float32(np.reshape(m.body_inertia, (m.nbody, 6))), (NENV, 1, 1))
    mass[2, bodies] *= np.float32(1.5)
    inertia[2, bodies] *= np.float32(1.5)
    d.set_model_params(None, body_mass=torch.tensor(mass, device="cuda"), body_inertia=torch.tensor(inertia, device="cuda"))
    after = mjx.body_data(sys_, d, fields)
    ref = br.body_data(m, outs[2], None, np.float64(mass[2]), np.float64(inertia[2]))
    base = r64[2]
    for f in fields:
        assert torch.equal(getattr(after, f)[0], getattr(before, f)[0]), f  # env 0: bit-identical
        got = getattr(after, f)[2].cpu().numpy().astype(np.float64)
        assert np.abs(got - ref[f]).max() <= 1.5 * tol[f]["bound"], f  # (the scaled values' magnitudes: at most 1.5 x)
    assert np.abs(ref["cinert"] - base["cinert"]).max() > 10 * tol["cinert"]["bound"]  # the values did move


def test_null_outputs_and_untouched_fields(setup):
    name, m, sys_, states, outs, r64, tol = setup
    d = _load(sys_, states)
    mjx.forward(sys_, d)
    fields = {f: d.get(f).clone() for f in abi.FIELD}
    every = mjx.body_data(sys_, d, POSVEL)
    only = mjx.body_data(sys_, d, ("subtree_com",))
    assert torch.equal(only.subtree_com, every.subtree_com) and only.xipos is None
    for f in abi.FIELD:
        assert torch.equal(d.get(f), fields[f]), f
    full = mjx.body_data(sys_, d, ALL)
    for f in POSVEL:
        assert torch.equal(getattr(full, f), getattr(every, f)), f
    with pytest.raises(mjx_amd._lib.MjlError):
        mjx.body_data(sys_, d, ())


def test_captured_with_an_env_step(setup):
    name, m, sys_, states, *_ = setup
    if name == "bd_chain":
        return  # the env is the humanoid's
    B, fields = 8, ("subtree_com", "cvel", "subtree_linvel")
    cfg = resolve_ids(m, dataclasses.replace(reference_ppo_config().env_config, max_episode_steps=1000))
    act = torch.tensor(np.random.default_rng(2).uniform(-1, 1, (B, m.nu)), dtype=torch.float32, device="cuda")

    def make():
        env = HumanoidEnv(sys_, cfg, B, seed=11)
        env.reset(counter=1)
        return env
    env = make()
    eager = []
    for i in range(3):
        env.step(act, auto_reset=False, counter=2 + i)
        eager.append([getattr(env.body_data(fields), f).clone() for f in fields])
    warm = make()  # warm-up launches outside the capture, on another batch
    warm.step(act, auto_reset=False, counter=2)
    warm.body_data(fields)
    env = make()
    bd = env.body_data(fields)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.step(act, auto_reset=False, counter=2)
        env.body_data(fields)
    for i in range(3):
        g.replay()
        torch.cuda.synchronize()
        for f, want in zip(fields, eager[i]):
            assert torch.equal(getattr(bd, f), want), (i, f)


def test_gym_humanoid_obs(setup):
    name, m, sys_, states, *_ = setup
    d = _load(sys_, states)
    bd = mjx.body_data(sys_, d, ("cinert", "cvel", "cfrc_ext"))
    obs = gym_humanoid_obs(sys_, d, bd)
    nb = m.nbody - 1
    parts = [d.get("qpos")[:, 2:], d.get("qvel"), bd.cinert[:, 1:].reshape(NENV, -1), bd.cvel[:, 1:].reshape(NENV, -1),
             d.get("qfrc_actuator"), bd.cfrc_ext[:, 1:].reshape(NENV, -1)]
    assert tuple(obs.shape) == (NENV, m.nq - 2 + m.nv + 10 * nb + 6 * nb + m.nv + 6 * nb)
    o = 0
    for p in parts:
        assert torch.equal(obs[:, o:o + p.shape[1]], p)
        o += p.shape[1]
    assert o == obs.shape[1]
