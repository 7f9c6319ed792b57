"""Sensor readout (mjl_sensors / mjx.sensors) on the GPU against tests/sensors_ref.py evaluated on the fp64
oracle's forward pass of the same state.

Model: each humanoid with, through MJCF text, an IMU site on the torso (rotated, off the body origin), one on
the left foot, jointpos / jointvel / jointlimitfrc / jointactuatorfrc on every hinge, actuatorfrc on every
actuator, frame sensors on one xbody and one site, and the two touch sensors among them (127 sensors, so adr
differs from the sensor id). Batch: 5 envs (rest state, two falls with random controls, two states with a knee
and an elbow past their range), one call with a mask that leaves out 2 envs, one without a mask.

Tolerances (recorded in profiles/sensors/tolerances.json, computed here again from the same inputs): per sensor
type the yardstick is max |formulas in numpy float32 - float64| over the test states; the kernel gets 8 x that
(summation order, fused multiply-adds), at least 1e-6 x the type's scale. Acc-stage values also inherit the
forward pass's error, with the existing parity tests' tolerances (tests/test_gpu_parity.py: qacc, efc_force-
derived values 2e-3 * (1 + max|ref|), qfrc_actuator 2e-5 * (1 + max|ref|)): touch and jointlimitfrc through
efc_force, jointactuatorfrc through qfrc_actuator, the accelerometer through qacc. The accelerometer is also
compared with the reference evaluated on the qacc the call's forward pass stored, at the 8 x yardstick bound
alone (about 9e-4 m/s^2): that takes the forward's error out and checks gravity and the centripetal / Coriolis
terms, which the test asserts are more than 100 x that bound in every moving state. framequat is compared up to sign (q and -q
are one rotation). The generic (non-humanoid) kernel instantiation runs in tests/test_generic_gpu.py, this
readout included (test_sensors_readout_on_tail); the CPU tests' small chain model (a free root with a rotated body, joint pos offsets, two joints on one body,
a site quaternion) fits the humanoid instantiation the existing small-model GPU tests run, so it is run here
too, with every sensor type once."""
import ctypes as C
import dataclasses
import os
import re

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

import actuators_ref as ar
import sensors_ref as sr

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
POS, VEL, ACC = (abi.SENSOR_STAGE[k] for k in ("pos", "vel", "acc"))
ALL = POS | VEL | ACC
T = mjcf.SENSOR_TYPES
SENTINEL = -77.25
NENV = 5
MASK = np.array([1, 0, 1, 1, 0], np.float32)
FORCED = {3: ("knee_left", "elbow_left"), 4: ("knee_left", "elbow_right")}  # joints set past their range, by env
FRAME7 = ("framepos", "framequat", "framexaxis", "frameyaxis", "framezaxis", "framelinvel", "frameangvel")


def sensor_xml(name):
    """The golden humanoid's MJCF with the two IMU sites and the full sensor set."""
    text = open(os.path.join(GOLDEN, name + ".xml")).read()
    base = mjx_amd.load_model(name)
    hinges, acts = base.names["joint"][1:], base.names["actuator"]
    text, n1 = re.subn(r'(<body name="torso"[^>]*>)',
                       r'\1\n<site name="imu_torso" pos="0.05 -0.02 0.1" quat="0.7 0.1 -0.5 0.5" size="0.01"/>', text)
    text, n2 = re.subn(r'(<body name="foot_left"[^>]*>)',
                       r'\1\n<site name="imu_foot" pos="0.02 0.01 -0.01" quat="0.5 -0.5 0.5 0.5" size="0.01"/>', text)
    assert n1 == 1 and n2 == 1
    s = [f'<jointpos name="jp_{j}" joint="{j}"/>' for j in hinges]
    s += ['<gyro name="gyro" site="imu_torso" noise="0.01"/>', '<touch name="touch_foot_right" site="site_foot_right"/>']
    s += [f'<jointvel name="jv_{j}" joint="{j}"/>' for j in hinges]
    s += ['<accelerometer name="accel" site="imu_torso"/>', '<velocimeter name="velo" site="imu_torso"/>',
          '<touch name="touch_foot_left" site="site_foot_left"/>']
    s += [f'<jointlimitfrc name="jl_{j}" joint="{j}"/>' for j in hinges]
    s += [f'<gyro name="gyro_foot" site="imu_foot"/>', '<accelerometer name="accel_foot" site="imu_foot"/>',
          '<velocimeter name="velo_foot" site="imu_foot"/>']
    s += [f'<jointactuatorfrc name="ja_{j}" joint="{j}"/>' for j in hinges]
    s += [f'<{t} name="{t}_pelvis" objtype="xbody" objname="pelvis"/>' for t in FRAME7]
    s += [f'<actuatorfrc name="af_{a}" actuator="{a}"/>' for a in acts]
    s += [f'<{t} name="{t}_site" objtype="site" objname="imu_torso"/>' for t in FRAME7]
    text, n3 = re.subn(r"<sensor>.*?</sensor>", "<sensor>\n" + "\n".join(s) + "\n</sensor>", text, flags=re.S)
    assert n3 == 1
    return text


def build_states(m, seed=3):
    """(qpos, qvel, qacc_warmstart, ctrl) x 5, rounded to float32: rest, two falls, two past-range states."""
    rng = np.random.default_rng(seed)
    od = Oracle(m)
    jn = m.names["joint"]
    qa = lambda n: int(m.jnt_qposadr[jn.index(n)])
    rng_of = lambda n: m.jnt_range[jn.index(n)]
    out = [(m.qpos0.copy(), np.zeros(m.nv), np.zeros(m.nv), np.zeros(m.nu))]
    for drop, nst in ((0.25, 25), (0.1, 45)):
        q = m.qpos0.copy()
        q[7:] += rng.uniform(-0.3, 0.3, m.nq - 7)
        q[2] -= drop
        s = od.new_state(q, rng.uniform(-1, 1, m.nv), ctrl=rng.uniform(-1, 1, m.nu))
        od.rollout(s, rng.uniform(-1, 1, (nst, m.nu)))
        a = state_arrays(m, s)
        out.append((a["qpos"], a["qvel"], a["qacc_warmstart"], rng.uniform(-1.5, 1.5, m.nu)))
    for k, (knee, elbow) in enumerate(FORCED[3 + i] for i in range(2)):
        q, v, w, _ = (x.copy() for x in out[1 + k])
        v, c = 0.5 * v, rng.uniform(-1.5, 1.5, m.nu)
        q[qa(knee)] = rng_of(knee)[0] - 0.05
        q[qa(elbow)] = rng_of(elbow)[1] + 0.04
        # the forced joints at rest with their motors pushing further past the limit: the limit rows carry force
        for jname, push in ((knee, -1.0), (elbow, 1.0)):
            v[int(m.jnt_dofadr[jn.index(jname)])] = 0.0
            c[m.names["actuator"].index(jname)] = push
        out.append((q, v, w, c))
    return [tuple(np.float32(x).astype(np.float64) for x in st) for st in out]


def reference(m, states, gear=None):
    """Per state: the oracle's forward outputs (motor-equivalent model for general actuators, as
    tests/test_actuators_gpu.py) and the reference rows in float64 and float32."""
    general = "actuator_kind" in m.arrays
    orc = Oracle(ar.motor_model(m, False) if general else m)
    outs, r64, r32 = [], [], []
    for i, (q, v, w, c) in enumerate(states):
        mi = m if gear is None else ar.with_arrays(m, actuator_gear=np.float64(gear[i]))
        if gear is not None:
            orc = Oracle(ar.motor_model(mi, False))
        oc = ar.motor_ctrl(mi, q, v, c, False) if general else c
        o = state_arrays(m, orc.forward(orc.new_state(q, v, w, oc)))
        outs.append(o)
        g = None if gear is None else np.float64(gear[i])
        r64.append(sr.sensordata(m, o, c, g, np.float64))
        r32.append(sr.sensordata(m, o, c, g, np.float32))
    return outs, np.array(r64), np.array(r32, np.float64)


def _slots(m):
    """Per sensor: (name, type, slice)."""
    A = m.arrays
    return [(m.names["sensor"][s], int(A["rsensor_type"][s]),
             slice(int(A["rsensor_adr"][s]), int(A["rsensor_adr"][s] + A["rsensor_dim"][s]))) for s in range(m.nrsensor)]


def tolerances(m, states, outs, r64, r32):
    """{type: {"yardstick", "scale", "bound"}} and the per-state inherited terms [state][sensor index]."""
    yard, scale = {}, sr.scales(m, r64)
    for _, t, sl in _slots(m):
        yard[t] = max(yard.get(t, 0.0), float(np.max(np.abs(r32[:, sl] - r64[:, sl]))))
    tol = {t: {"yardstick": yard[t], "scale": scale[t], "bound": max(8 * yard[t], 1e-6 * scale[t])} for t in yard}
    inherited = []
    for (q, v, w, c), o in zip(states, outs):
        tq = 2e-3 * (1 + np.abs(o["qacc"]).max())
        te = 2e-3 * (1 + (np.abs(o["efc_force"]).max() if len(o["efc_force"]) else 0.0))
        ta = 2e-5 * (1 + np.abs(o["qfrc_actuator"]).max())
        row = []
        for s, (_, t, sl) in enumerate(_slots(m)):
            if t in (T["touch"], T["jointlimitfrc"]):
                row.append(te)
            elif t == T["jointactuatorfrc"]:
                row.append(ta)
            elif t == T["accelerometer"]:  # against the oracle's qacc; accel_on_stored_qacc takes this term out
                row.append(tq)
            else:
                row.append(0.0)
        inherited.append(row)
    return tol, inherited


def accel_on_stored_qacc(m, states, outs, got, qacc, tol, what, gear=None):
    """The accelerometers against the reference evaluated with the qacc the forward pass of the call stored
    (float32, read back): the forward's own error is out of the comparison, so the bound is the kernel's alone,
    8 x yardstick, and the velocity-dependent terms and gravity are checked at that resolution."""
    worst = 0.0
    for e, ((q, v, w, c), o) in enumerate(zip(states, outs)):
        ref = sr.sensordata(m, dict(o, qacc=np.asarray(qacc[e], np.float64)), c, None if gear is None else np.float64(gear[e]))
        for name, t, sl in _slots(m):
            if t != T["accelerometer"]:
                continue
            err = np.abs(np.asarray(got[e, sl], np.float64) - ref[sl]).max()
            worst = max(worst, err / tol[t]["bound"])
            assert err <= tol[t]["bound"], f"{what} env {e} {name} on the stored qacc: err {err:.3e} > {tol[t]['bound']:.3e}"
    print(what, "accelerometer on the stored qacc, worst err / bound:", round(worst, 3))


def tolerance_table():
    """What profiles/sensors/tolerances.json holds (tools/sensor_tolerances.py writes it, tests/test_sensors.py
    compares): per model and sensor type the yardstick, scale and bound, and the largest inherited term."""
    from test_sensors import CHAIN
    inv = {v: k for k, v in T.items()}
    models = {name: mjcf.compile_xml_string(sensor_xml(name), name) for name in mjx_amd.BUILTIN_MODELS}
    models["chain"] = mjcf.compile_xml_string(CHAIN, "chain")
    table = {}
    for name, m in models.items():
        states = chain_states(m) if name == "chain" else build_states(m)
        outs, r64, r32 = reference(m, states)
        tol, inh = tolerances(m, states, outs, r64, r32)
        types = [t for _, t, _ in _slots(m)]
        table[name] = {inv[t]: dict(v, inherited_max=max(row[s] for row in inh for s, tt in enumerate(types) if tt == t))
                       for t, v in sorted(tol.items())}
    return table


def _load(sys_, states):
    d = mjx.make_data(sys_, len(states))
    t = lambda i: torch.tensor(np.array([s[i] for s in states]), dtype=torch.float32)
    for i, f in enumerate(("qpos", "qvel", "qacc_warmstart", "ctrl")):
        d.set(f, t(i))
    return d


def _check_rows(m, got, r64, tol, inherited, envs, what):
    worst = {}
    for e in envs:
        for s, (name, t, sl) in enumerate(_slots(m)):
            g, r = np.asarray(got[e, sl], np.float64), r64[e, sl]
            err = np.abs(g - r).max()
            if t == T["framequat"]:
                err = min(err, np.abs(g + r).max())
            bound = tol[t]["bound"] + inherited[e][s]
            worst[t] = max(worst.get(t, 0.0), err / bound)
            assert err <= bound, f"{what} env {e} sensor {name}: err {err:.3e} > {bound:.3e}"
    print(what, "worst err / bound per type:", {k: round(v, 3) for k, v in sorted(worst.items())})


@pytest.fixture(scope="module", params=mjx_amd.BUILTIN_MODELS)
def setup(request):
    m = mjcf.compile_xml_string(sensor_xml(request.param), request.param)
    states = build_states(m)
    outs, r64, r32 = reference(m, states)
    tol, inh = tolerances(m, states, outs, r64, r32)
    return request.param, m, mjx.put_model(m), states, outs, r64, tol, inh


def test_input_conditions(setup):
    """Asserted on the reference alone: the inputs exercise limits, touch and (PD variant) the force clamp."""
    name, m, sys_, states, outs, r64, tol, inh = setup
    sl = {t: [s for _, tt, s in _slots(m) if tt == t] for t in T.values()}
    lim = [any(np.any(r64[e, s] != 0) for s in sl[T["jointlimitfrc"]]) for e in range(NENV)]
    touch = [any(np.any(r64[e, s] != 0) for s in sl[T["touch"]]) for e in range(NENV)]
    assert sum(lim) >= 2 and sum(touch) >= 1, (lim, touch)
    for e, joints in FORCED.items():  # the limits the states force carry force, in masked-in env 3 too
        assert all(r64[e, m.sensor_slice("jl_" + j)][0] > 1.0 for j in joints), (e, joints)
    assert MASK[3] > 0.5
    # the moving states' velocity-dependent acceleration is far above the accelerometer's own bound
    for e in range(1, NENV):
        q, v = states[e][0], states[e][1]
        k1, k0 = sr.kinematics(m, q, v, outs[e]["qacc"]), sr.kinematics(m, q, None, outs[e]["qacc"])
        site = m.names["site"].index("imu_foot")
        dv = np.abs(sr.frame(m, k1, mjcf.OBJ_SITE, site)[4] - sr.frame(m, k0, mjcf.OBJ_SITE, site)[4]).max()
        assert dv > 100 * tol[T["accelerometer"]]["bound"], (e, dv)
    assert m.nrsensor == 127 and len(states) == NENV
    assert [s.start for _, _, s in _slots(m)] != list(range(m.nrsensor))  # adr differs from the sensor id
    g = ar.general_model(m, 20.0, 1.5, seed=4, forcerange=0.35)
    clamped = [sr.actuator_force(g, u, q, v, c)[1] for q, v, _, c in states for u in range(g.nu)]
    assert any(clamped) and not all(clamped)


def test_parity_masked_and_unmasked(setup):
    name, m, sys_, states, outs, r64, tol, inh = setup
    d = _load(sys_, states)
    out = torch.full((NENV, sys_.nrsensordata), SENTINEL, device="cuda")
    mjx.sensors(sys_, d, mask=torch.tensor(MASK), out=out)
    got = out.cpu().numpy()
    assert (got[MASK < 0.5] == SENTINEL).all()  # masked-out rows keep the sentinel
    _check_rows(m, got, r64, tol, inh, np.flatnonzero(MASK > 0.5), f"{name} masked")
    d = _load(sys_, states)
    got = mjx.sensors(sys_, d).cpu().numpy()
    _check_rows(m, got, r64, tol, inh, range(NENV), name)
    accel_on_stored_qacc(m, states, outs, got, d.get("qacc").cpu().numpy(), tol, name)
    # bit equality where the kernel copies
    qpos, qvel = d.get("qpos").cpu().numpy(), d.get("qvel").cpu().numpy()
    touch, qfa = d.get("sensordata").cpu().numpy(), d.get("qfrc_actuator").cpu().numpy()
    A = m.arrays
    for s, (sname, t, sl) in enumerate(_slots(m)):
        j = int(A["rsensor_objid"][s])
        if t == T["jointpos"]:
            np.testing.assert_array_equal(got[:, sl.start], qpos[:, A["jnt_qposadr"][j]], err_msg=sname)
        elif t == T["jointvel"]:
            np.testing.assert_array_equal(got[:, sl.start], qvel[:, A["jnt_dofadr"][j]], err_msg=sname)
        elif t == T["jointactuatorfrc"]:
            np.testing.assert_array_equal(got[:, sl.start], qfa[:, A["jnt_dofadr"][j]], err_msg=sname)
        elif t == T["touch"]:
            np.testing.assert_array_equal(got[:, sl.start], touch[:, A["sensor_adr"][j]], err_msg=sname)
    assert sys_.sensor_slice("accel") == _slots(m)[[n for n, _, _ in _slots(m)].index("accel")][2]


@pytest.mark.parametrize("variant", ["pd_forcerange", "per_env_gear"])
def test_actuator_variants(setup, variant):
    """actuatorfrc (and everything else) with PD actuators and a force range, then with per-env gear."""
    name, m, _, states, _, _, _, _ = setup
    g = ar.general_model(m, 20.0, 1.5, seed=4, forcerange=0.35)
    sys_ = mjx.put_model(g)
    d = _load(sys_, states)
    gear = None
    if variant == "per_env_gear":
        gear = np.float32(np.asarray(g.actuator_gear) * np.random.default_rng(8).uniform(0.5, 1.5, (NENV, g.nu)))
        d.enable_model_params(True)
        d.set_model_params(None, actuator_gear=torch.tensor(gear, device="cuda"))
    outs, r64, r32 = reference(g, states, gear)
    tol, inh = tolerances(g, states, outs, r64, r32)
    got = mjx.sensors(sys_, d).cpu().numpy()
    _check_rows(g, got, r64, tol, inh, range(NENV), f"{name} {variant}")
    accel_on_stored_qacc(g, states, outs, got, d.get("qacc").cpu().numpy(), tol, f"{name} {variant}", gear)


def test_argument_errors_and_a_model_without_sensors(setup):
    name, m, sys_, states, *_ = setup
    L, err = lib(), HEADER.enums["MJL_ERR_ARG"]
    d = _load(sys_, states)
    out = torch.full((NENV, sys_.nrsensordata), SENTINEL, device="cuda")
    ptr, stream = C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.mjl_sensors(d.handle, None, ALL, None, stream) == err and b"out" in L.mjl_last_error()
    for stages in (0, 8, ALL | 16, -1):
        assert L.mjl_sensors(d.handle, None, stages, ptr, stream) == err and b"stages" in L.mjl_last_error(), stages
    assert L.mjl_sensors(None, None, ALL, ptr, stream) == err
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
    # a model without sensors: OK, nothing launched, the buffer untouched
    text = re.sub(r"<sensor>.*?</sensor>", "", open(os.path.join(GOLDEN, name + ".xml")).read(), flags=re.S)
    bare = mjcf.compile_xml_string(text, name)
    assert (bare.nrsensor, bare.nsensor) == (0, 0)
    sysb = mjx.put_model(bare)
    db = mjx.make_data(sysb, 2)
    assert sysb.nrsensordata == 0 and L.mjl_sensors(db.handle, None, ALL, ptr, stream) == 0
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and tuple(mjx.sensors(sysb, db).shape) == (2, 0)


def chain_states(m):
    """Four states of the CPU tests' chain (a free root with a rotated body, joints with pos offsets, two joints on
    one body, a site quaternion): rest, tumbling in the air, lying on the floor, j1 pushed past its range."""
    rng = np.random.default_rng(12)
    out = [(m.qpos0.copy(), np.zeros(m.nv), np.zeros(m.nv), np.zeros(m.nu))]
    for z, past in ((1.0, False), (0.045, False), (1.0, True)):
        q = m.qpos0.copy()
        q[2] = z
        q[3:7] = rng.normal(size=4) if z == 1.0 else [1.0, 0.0, 0.02, 0.0]
        q[3:7] /= np.linalg.norm(q[3:7])
        q[7:] += rng.uniform(-0.4, 0.4, m.nq - 7)
        v, c = rng.uniform(-2, 2, m.nv) * (0.1 if z < 1 else 1.0), rng.uniform(-1, 1, m.nu)
        if past:
            q[7], v[6], c[0] = m.jnt_range[1][1] + 0.05, 0.0, 1.0
        out.append((q, v, np.zeros(m.nv), c))
    return [tuple(np.float32(x).astype(np.float64) for x in st) for st in out]


def test_chain_model():
    """A non-humanoid tree through the same kernel: every sensor type once (tests/test_sensors.py CHAIN)."""
    from test_sensors import CHAIN
    m = mjcf.compile_xml_string(CHAIN, "chain")
    states = chain_states(m)
    outs, r64, r32 = reference(m, states)
    tol, inh = tolerances(m, states, outs, r64, r32)
    assert r64[3, m.sensor_slice("lf")][0] > 1.0 and outs[2]["ncon"] > 0  # a loaded limit; a state in contact
    sys_ = mjx.put_model(m)
    d = _load(sys_, states)
    got = mjx.sensors(sys_, d).cpu().numpy()
    _check_rows(m, got, r64, tol, inh, range(len(states)), "chain")
    accel_on_stored_qacc(m, states, outs, got, d.get("qacc").cpu().numpy(), tol, "chain")


def test_no_forward_path_after_a_step(setup):
    """POS | VEL alone after mjl_step: the post-step state's values, the acc slots and every field untouched."""
    name, m, sys_, states, *_ = setup
    d = _load(sys_, states)
    mjx.step(sys_, d)
    fields = {f: d.get(f).clone() for f in abi.FIELD}
    out = torch.full((NENV, sys_.nrsensordata), SENTINEL, device="cuda")
    mjx.sensors(sys_, d, stages=POS | VEL, out=out)
    for f in abi.FIELD:
        assert torch.equal(d.get(f), fields[f]), f
    fresh = mjx.make_data(sys_, NENV)
    fresh.set("qpos", fields["qpos"])
    fresh.set("qvel", fields["qvel"])
    want = mjx.sensors(sys_, fresh, stages=POS | VEL)
    got, want = out.cpu().numpy(), want.cpu().numpy()
    for sname, t, sl in _slots(m):
        if mjcf.sensor_stage(t) == ACC:
            assert (got[:, sl] == SENTINEL).all(), sname
        else:
            np.testing.assert_array_equal(got[:, sl], want[:, sl], err_msg=sname)
    # the stages one at a time fill the same slots
    out2 = torch.full_like(out, SENTINEL)
    mjx.sensors(sys_, d, stages=POS, out=out2)
    mjx.sensors(sys_, d, stages=VEL, out=out2)
    assert torch.equal(out2, out)


def test_captured_with_an_env_step(setup):
    name, m, sys_, states, *_ = setup
    B = 8
    cfg = resolve_ids(m, dataclasses.replace(reference_ppo_config().env_config, max_episode_steps=1000))
    act = torch.tensor(np.random.default_rng(2).uniform(-1, 1, (B, m.nu)), dtype=torch.float32, device="cuda")

    def make():
        env = HumanoidEnv(sys_, cfg, B, seed=11)
        env.reset(counter=1)
        return env
    env = make()
    env.step(act, auto_reset=False, counter=2)
    eager = env.sensors(stages=POS | VEL).cpu().numpy()
    env = make()
    buf = torch.zeros((B, sys_.nrsensordata), device="cuda")
    warm = HumanoidEnv(sys_, cfg, B, seed=11)  # warm-up launches outside the capture, on another batch
    warm.reset(counter=1)
    warm.step(act, auto_reset=False, counter=2)
    warm.sensors(stages=POS | VEL)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.step(act, auto_reset=False, counter=2)
        env.sensors(stages=POS | VEL, out=buf)
    g.replay()
    torch.cuda.synchronize()
    # the capture did not run the step; the replay is the first (and only) step of this env
    np.testing.assert_array_equal(buf.cpu().numpy(), eager)
