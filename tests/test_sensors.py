"""Sensor readout, host side (no GPU): the MJCF compiler's two sensor tables, the descriptor validation of
mjl_model_create (also alone, under the host sanitizers, through tools/model_host_check.cpp), the binding and
argument errors of mjl_sensors / mjl_model_nrsensordata, and the validation of tests/sensors_ref.py against
finite differences and the oracle's kinematics, independently of any GPU code."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mjx_amd
from mjx_amd import _lib, abi, mjcf
from mjx_amd._header import HEADER
from oracle import Oracle, state_arrays

import sensors_ref as sr
from test_model_host import _compiler, _create, _set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
OK, ARG, UNSUPPORTED = 0, 1, 2
T = mjcf.SENSOR_TYPES

# a hinge chain on a free body with a rotated root, joint pos offsets, two joints on one body and a site
# quaternion: small enough to read, every sensor type once; tests/test_sensors_gpu.py runs it on the GPU too
CHAIN = """<mujoco model="chain"><option timestep="0.002"/>
<worldbody><geom name="floor" type="plane" size="5 5 .1"/>
 <body name="base" pos="0 0 1" quat="0.9 0.1 0.3 0.3"><freejoint name="root"/>
  <geom type="capsule" size=".05" fromto="0 0 0 .3 0 0"/>
  <site name="imu" pos=".1 .02 .03" quat="0.5 0.5 -0.5 0.5" size=".01"/>
  <body name="link1" pos=".3 0 0" quat="0.8 0 0.6 0"><joint name="j1" axis="0 1 0" pos=".02 0 .01" range="-30 40"/>
   <geom type="capsule" size=".04" fromto="0 0 0 .25 0 0"/>
   <body name="link2" pos=".25 0 0"><joint name="j2" axis="0 0 1" range="-50 50"/><joint name="j3" axis="1 0 0" pos="0 .01 0"/>
    <geom type="capsule" size=".03" fromto="0 0 0 .2 0 0"/>
    <site name="tip" pos=".2 0 .01" size=".02 .02 .02" type="box"/>
   </body></body></body></worldbody>
<actuator><motor name="m1" joint="j1" gear="10" ctrlrange="-1 1"/><motor name="m2" joint="j2" gear="5"/></actuator>
<sensor>
 <framepos name="fp" objtype="site" objname="tip"/><jointpos name="p1" joint="j1"/><gyro name="g" site="imu" noise="0.1"/>
 <touch name="t" site="tip"/><framequat name="fq" objtype="xbody" objname="link2"/><jointvel name="v2" joint="j2"/>
 <accelerometer name="acc" site="imu"/><velocimeter name="vel" site="tip"/><actuatorfrc name="af" actuator="m2"/>
 <jointlimitfrc name="lf" joint="j1"/><jointactuatorfrc name="jf" joint="j2"/><framexaxis name="fx" objtype="site" objname="imu"/>
 <frameyaxis name="fy" objtype="xbody" objname="base"/><framezaxis name="fz" objtype="site" objname="tip"/>
 <framelinvel name="lv" objtype="site" objname="tip"/><frameangvel name="av" objtype="xbody" objname="link1"/>
</sensor></mujoco>"""


@pytest.fixture(scope="module")
def chain():
    return mjcf.compile_xml_string(CHAIN, "chain")


def test_constants_are_the_headers():
    E = HEADER.enums
    assert {k: E["MJL_SENS_" + k.upper()] for k in T} == T and len(T) == E["MJL_NSENSTYPE"] == 16 and T["touch"] == 0
    assert (mjcf.OBJ_XBODY, mjcf.OBJ_SITE, mjcf.OBJ_JOINT, mjcf.OBJ_ACTUATOR, mjcf.OBJ_TOUCH) == tuple(
        E["MJL_OBJ_" + k] for k in ("XBODY", "SITE", "JOINT", "ACTUATOR", "TOUCH"))
    assert (mjcf.STAGE_POS, mjcf.STAGE_VEL, mjcf.STAGE_ACC) == (1, 2, 4) == tuple(abi.SENSOR_STAGE[k] for k in ("pos", "vel", "acc"))
    assert (mjcf.MAXRSENSOR, mjcf.MAXRSENSORDATA) == (abi.MAXRSENSOR, abi.MAXRSENSORDATA) == (128, 256)
    stage = {"pos": ("jointpos", "framepos", "framequat", "framexaxis", "frameyaxis", "framezaxis"),
             "vel": ("jointvel", "gyro", "velocimeter", "framelinvel", "frameangvel"),
             "acc": ("touch", "accelerometer", "actuatorfrc", "jointactuatorfrc", "jointlimitfrc")}
    for st, names in stage.items():
        assert all(mjcf.sensor_stage(T[n]) == abi.SENSOR_STAGE[st] for n in names)
    assert [mjcf.sensor_dim(T[n]) for n in ("touch", "jointpos", "framequat", "gyro", "actuatorfrc", "framezaxis")] == [1, 1, 4, 3, 1, 3]


def test_every_element_compiles_into_both_tables(chain):
    m, A = chain, chain.arrays
    names = ["fp", "p1", "g", "t", "fq", "v2", "acc", "vel", "af", "lf", "jf", "fx", "fy", "fz", "lv", "av"]
    assert m.names["sensor"] == names and m.nrsensor == 16
    want_t = [T[k] for k in ("framepos", "jointpos", "gyro", "touch", "framequat", "jointvel", "accelerometer", "velocimeter",
                             "actuatorfrc", "jointlimitfrc", "jointactuatorfrc", "framexaxis", "frameyaxis", "framezaxis",
                             "framelinvel", "frameangvel")]
    dims = [3, 1, 3, 1, 4, 1, 3, 3, 1, 1, 1, 3, 3, 3, 3, 3]
    S, X, J, U, TT = mjcf.OBJ_SITE, mjcf.OBJ_XBODY, mjcf.OBJ_JOINT, mjcf.OBJ_ACTUATOR, mjcf.OBJ_TOUCH
    assert list(A["rsensor_type"]) == want_t and list(A["rsensor_dim"]) == dims
    assert list(A["rsensor_adr"]) == list(np.cumsum([0] + dims[:-1])) and m.nrsensordata == sum(dims) == 37
    assert list(A["rsensor_objtype"]) == [S, J, S, TT, X, J, S, S, U, J, J, S, X, S, S, X]
    assert list(A["rsensor_objid"]) == [1, 1, 0, 0, 3, 2, 0, 1, 1, 1, 2, 0, 1, 1, 1, 2]
    # the touch list is what it was: one touch sensor on site 1, at address 0
    assert (m.nsensor, m.nsensordata) == (1, 1)
    assert list(A["sensor_type"]) == [0] and list(A["sensor_objid"]) == [1] and list(A["sensor_adr"]) == [0]
    assert m.sensor_slice("acc") == slice(13, 16) and m.sensor_slice("fq") == slice(8, 12)
    with pytest.raises(KeyError):
        m.sensor_slice("nope")
    d = abi.model_desc(m)
    assert (d.nrsensor, d.nrsensordata, d.nsensor, d.nsensordata) == (16, 37, 1, 1)
    assert _create(_lib.lib(), d)[0] == OK


@pytest.mark.parametrize("element,fragment", [
    ('<framepos name="bad" objtype="body" objname="link1"/>', "objtype='body'"),
    ('<framequat name="bad" objtype="geom" objname="floor"/>', "objtype='geom'"),
    ('<framepos name="bad" objtype="site" objname="tip" reftype="xbody" refname="base"/>', "reftype"),
    ('<gyro name="bad" site="imu" cutoff="2"/>', "cutoff"),
    ('<magnetometer name="bad" site="imu"/>', "<magnetometer> 'bad' not supported"),
    ('<jointpos name="bad" joint="root"/>', "free joint"),
    ('<jointvel name="bad" joint="root"/>', "free joint"),
    ('<touch name="bad" site="imu"/>', "box site"),
    ('<gyro name="bad" site="nosuch"/>', "unknown site"),
])
def test_rejected_forms_name_the_sensor(element, fragment):
    with pytest.raises(mjcf.MJCFError) as e:
        mjcf.compile_xml_string(CHAIN.replace("<sensor>", "<sensor>" + element), "chain")
    assert "bad" in str(e.value) and fragment in str(e.value)


def test_touch_only_models_keep_their_arrays_byte_for_byte():
    for name in mjx_amd.BUILTIN_MODELS:
        fresh, asset = mjcf.compile_xml(os.path.join(GOLDEN, name + ".xml")), mjx_amd.load_model(name)
        old = [k for k in fresh.arrays if k not in mjcf.READOUT_ARRAYS]
        assert set(mjcf.READOUT_ARRAYS) <= set(fresh.arrays) and len(old) == len(fresh.arrays) - 5
        for k in old:
            a, b = np.asarray(fresh.arrays[k]), np.asarray(asset.arrays[k])
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
        assert fresh.names["sensor"] == ["touch_foot_right", "touch_foot_left"] == asset.names["sensor"]
        for m in (fresh, asset):  # the readout table of a touch-only model is the touch list
            assert (m.nrsensor, m.nrsensordata) == (2, 2)
            assert [list(m.arrays[k]) for k in mjcf.READOUT_ARRAYS] == [[0, 0], [mjcf.OBJ_TOUCH] * 2, [0, 1], [0, 1], [1, 1]]


def test_env_touch_ids_index_the_touch_list():
    """With other sensors declared before them the touch sensors' ids move; the env config keeps the touch list's."""
    from mjx_amd.config import reference_ppo_config
    from mjx_amd.envs import resolve_ids
    text = open(os.path.join(GOLDEN, "humanoid_mjx.xml")).read()
    text = text.replace('<touch name="touch_foot_right"', '<jointpos name="kp" joint="knee_left"/>\n<touch name="touch_foot_right"')
    text = text.replace('<touch name="touch_foot_left"', '<jointvel name="kv" joint="knee_left"/>\n<touch name="touch_foot_left"')
    m = mjcf.compile_xml_string(text, "humanoid_mjx")
    assert m.names["sensor"] == ["kp", "touch_foot_right", "kv", "touch_foot_left"] and m.nsensor == 2
    cfg = resolve_ids(m, reference_ppo_config().env_config)
    assert (cfg.touch_sensor_right_id, cfg.touch_sensor_left_id) == (0, 1)
    base = resolve_ids(mjx_amd.load_model("humanoid_mjx"), reference_ppo_config().env_config)
    assert (base.touch_sensor_right_id, base.touch_sensor_left_id) == (0, 1)


# descriptor validation: (case, mutation of the chain's descriptor, code, message fragment)
REJECTED = [
    ("nrsensor_over", _set("nrsensor", abi.MAXRSENSOR + 1), UNSUPPORTED, "readout table exceeds"),
    ("nrsensordata_over", _set("nrsensordata", abi.MAXRSENSORDATA + 1), UNSUPPORTED, "readout table exceeds"),
    ("nrsensor_neg", _set("nrsensor", -1), ARG, "negative"),
    ("type_unknown", _set("rsensor_type", 16, 2), UNSUPPORTED, "rsensor_type[2] = 16"),
    ("type_neg", _set("rsensor_type", -1, 2), UNSUPPORTED, "rsensor_type[2] = -1"),
    ("objtype_gyro_xbody", _set("rsensor_objtype", 0, 2), UNSUPPORTED, "rsensor_objtype[2] = 0"),
    ("objtype_touch_site", _set("rsensor_objtype", 1, 3), UNSUPPORTED, "rsensor_objtype[3] = 1"),
    ("objtype_joint_site", _set("rsensor_objtype", 1, 1), UNSUPPORTED, "rsensor_objtype[1] = 1"),
    ("objtype_frame_joint", _set("rsensor_objtype", 2, 0), UNSUPPORTED, "rsensor_objtype[0] = 2"),
    ("site_past", _set("rsensor_objid", 2, 2), ARG, "rsensor_objid[2] = 2"),
    ("site_neg", _set("rsensor_objid", -1, 0), ARG, "rsensor_objid[0] = -1"),
    ("body_past", _set("rsensor_objid", 4, 4), ARG, "rsensor_objid[4] = 4"),
    ("joint_past", _set("rsensor_objid", 4, 1), ARG, "rsensor_objid[1] = 4"),
    ("joint_huge", _set("rsensor_objid", 2**31 - 1, 9), ARG, "rsensor_objid[9]"),
    ("joint_free", _set("rsensor_objid", 0, 5), UNSUPPORTED, "free joint"),
    ("actuator_past", _set("rsensor_objid", 2, 8), ARG, "rsensor_objid[8] = 2"),
    ("touch_past", _set("rsensor_objid", 1, 3), ARG, "rsensor_objid[3] = 1"),
    ("dim_wrong", _set("rsensor_dim", 3, 4), ARG, "rsensor_dim[4] = 3"),
    ("adr_neg", _set("rsensor_adr", -1, 1), ARG, "rsensor_adr[1] = -1"),
    ("adr_past", _set("rsensor_adr", 35, 15), ARG, "rsensor_adr[15] = 35"),
    ("adr_overlap", _set("rsensor_adr", 2, 1), ARG, "overlaps"),
    ("ndata_short", _set("nrsensordata", 36), ARG, "rsensor_adr[15] = 34"),
]


@pytest.fixture(scope="module")
def host_results(chain, tmp_path_factory):
    """Per case: (code, message) of model_build alone under ASan + UBSan, and of mjl_model_create."""
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("sensor_host")
    exe = tmp / "model_host_check"
    cc = subprocess.run([cxx, "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                         os.path.join(ROOT, "tools", "model_host_check.cpp")], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    base = bytes(abi.model_desc(chain))
    cases = {"chain": abi.ModelDesc.from_buffer_copy(base)}
    for case, mutate, _, _ in REJECTED:
        cases[case] = abi.ModelDesc.from_buffer_copy(base)
        mutate(cases[case])
    files = []
    for case, d in cases.items():
        files.append(str(tmp / (case + ".desc")))
        with open(files[-1], "wb") as fh:
            fh.write(bytes(d))
    run = subprocess.run([str(exe)] + files, capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-4000:]
    tab = subprocess.run([str(exe), "--sensors", files[0]], capture_output=True, text=True)
    assert tab.returncode == 0 and tab.stderr == "", tab.stderr[-4000:]
    L = _lib.lib()
    out = {"--sensors": tab.stdout}
    for (case, d), line in zip(cases.items(), run.stdout.splitlines()):
        col = line.split("\t")
        out[case] = {"alone": (int(col[1].split("=")[1]), col[5].split("=", 1)[1]), "lib": _create(L, d)[:2]}
    return out


def test_accepted_alone_and_its_table(host_results, chain):
    assert host_results["chain"]["alone"] == (OK, "") == host_results["chain"]["lib"]
    line = host_results["--sensors"].splitlines()[0].split("\t")
    assert line[1:4] == ["rc=0", "n=16", "ndata=37"] and line[4] == "stages=7"
    stages = [mjcf.sensor_stage(int(t)) for t in chain.arrays["rsensor_type"]]
    assert line[5] == "stage=" + ",".join(str(s) for s in stages)
    assert line[6].startswith("site_quat0=0.5,0.5,-0.5,0.5")


@pytest.mark.parametrize("case,code,fragment", [(c, code, frag) for c, _, code, frag in REJECTED])
def test_descriptor_rejections(host_results, case, code, fragment):
    r = host_results[case]
    assert r["alone"][0] == code and fragment in r["alone"][1], r["alone"]
    assert r["lib"] == r["alone"]


def test_entry_points_and_argument_errors_without_gpu(chain):
    L = _lib.lib()
    vp, i32 = C.c_void_p, C.c_int
    assert "mjl_sensors" in _lib.EXPORTS and "mjl_model_nrsensordata" in _lib.EXPORTS
    assert L.mjl_sensors.argtypes == [vp, vp, i32, vp, vp] and L.mjl_sensors.restype is i32
    assert L.mjl_model_nrsensordata.argtypes == [vp] and L.mjl_model_nrsensordata.restype is i32
    by_name = {n: a for _, n, a in HEADER.protos}
    assert by_name["mjl_sensors"] == ["mjlBatch*", "float*", "int", "float*", "void*"]
    assert L.mjl_model_nrsensordata(None) == -1
    h = C.c_void_p()
    assert L.mjl_model_create(C.byref(abi.model_desc(chain)), C.byref(h)) == 0
    assert L.mjl_model_nrsensordata(h) == 37
    L.mjl_model_destroy(h)
    err = HEADER.enums["MJL_ERR_ARG"]
    assert L.mjl_sensors(None, None, 7, None, None) == err and b"null batch" in L.mjl_last_error()
    assert HEADER.enums["MJL_NFIELD"] == 16 and abi.desc_size() > 0  # no field was added
    from mjx_amd import mjx
    sys_ = mjx.put_model(chain)
    assert sys_.nrsensordata == 37 and sys_.sensor_slice("g") == slice(4, 7)
    assert mjx_amd.sensors is mjx.sensors
    from mjx_amd.envs import HumanoidEnv
    assert callable(HumanoidEnv.sensors)
    for name in mjx_amd.BUILTIN_MODELS:
        assert mjx.put_model(mjx_amd.load_model(name)).nrsensordata == 2


def test_recorded_tolerances_are_what_the_gpu_test_computes():
    """profiles/sensors/tolerances.json (tools/sensor_tolerances.py) against the GPU test's own computation, which
    needs no GPU: yardsticks, scales, bounds and inherited terms, per model and sensor type."""
    import json
    import test_sensors_gpu as tg
    with open(os.path.join(ROOT, "profiles", "sensors", "tolerances.json")) as f:
        rec = json.load(f)["models"]
    now = tg.tolerance_table()
    assert set(rec) == set(now) == {"humanoid_mjx", "humanoid", "chain"}
    for name in now:
        assert set(rec[name]) == set(now[name]), name
        for t, v in now[name].items():
            for k in ("yardstick", "scale", "bound", "inherited_max"):
                assert rec[name][t][k] == pytest.approx(v[k], rel=1e-6, abs=1e-12), (name, t, k)
            assert v["bound"] == max(8 * v["yardstick"], 1e-6 * v["scale"])


# ---- the reference, validated on the CPU -------------------------------------------------------------------------
def _advance(m, q, v, eps):
    """q + eps * v on the configuration manifold (free joint: world translation, local rotation)."""
    A, out = m.arrays, np.array(q, np.float64)
    for j in range(m.njnt):
        qa, d = int(A["jnt_qposadr"][j]), int(A["jnt_dofadr"][j])
        if A["jnt_type"][j] == mjcf.JNT_FREE:
            out[qa:qa + 3] += eps * v[d:d + 3]
            w = eps * v[d + 3:d + 6]
            ang = np.linalg.norm(w)
            dq = np.array([1.0, 0, 0, 0]) if ang == 0 else np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * w / ang])
            out[qa + 3:qa + 7] = mjcf.quat_mul(q[qa + 3:qa + 7] / np.linalg.norm(q[qa + 3:qa + 7]), dq)
        else:
            out[qa] += eps * v[d]
    return out


def _frames(m):
    return [(mjcf.OBJ_XBODY, b) for b in range(1, m.nbody)] + [(mjcf.OBJ_SITE, s) for s in range(m.nsite)]


def _ref_models():
    return [mjcf.compile_xml_string(CHAIN, "chain"), mjx_amd.load_model("humanoid_mjx")]


@pytest.mark.parametrize("m", _ref_models(), ids=["chain", "humanoid_mjx"])
def test_reference_velocities_and_accelerations_against_finite_differences(m):
    rng = np.random.default_rng(5)
    q = np.array(m.qpos0, np.float64)
    q[7:] += rng.uniform(-0.4, 0.4, m.nq - 7)
    q[3:7] = rng.normal(size=4)
    q[3:7] /= np.linalg.norm(q[3:7])
    v, a = rng.uniform(-2, 2, m.nv), rng.uniform(-5, 5, m.nv)
    eps = 1e-6
    k0 = sr.kinematics(m, q, v, a)
    kp, km = sr.kinematics(m, _advance(m, q, v, eps), v), sr.kinematics(m, _advance(m, q, v, -eps), v)
    ka = sr.kinematics(m, q, a)  # J(q) qacc: the velocities qacc would give
    for ot, oid in _frames(m):
        p0, R0, w0, v0, a0 = sr.frame(m, k0, ot, oid)
        pp, Rp, _, vp_, _ = sr.frame(m, kp, ot, oid)
        pm, Rm, _, vm_, _ = sr.frame(m, km, ot, oid)
        np.testing.assert_allclose(v0, (pp - pm) / (2 * eps), atol=2e-8, err_msg=f"linvel {ot} {oid}")
        W = (Rp - Rm) / (2 * eps) @ R0.T  # skew(w)
        np.testing.assert_allclose(w0, [W[2, 1], W[0, 2], W[1, 0]], atol=2e-8, err_msg=f"angvel {ot} {oid}")
        np.testing.assert_allclose(a0, sr.frame(m, ka, ot, oid)[3] + (vp_ - vm_) / (2 * eps), atol=2e-7,
                                   err_msg=f"acceleration {ot} {oid}")
        # velocimeter and gyro are these in the frame: nothing else to check but the rotation
        np.testing.assert_allclose(R0 @ R0.T, np.eye(3), atol=1e-12)


@pytest.mark.parametrize("name", mjx_amd.BUILTIN_MODELS)
def test_reference_frames_and_velocities_against_the_oracle(name):
    m = mjx_amd.load_model(name)
    rng = np.random.default_rng(6)
    orc = Oracle(m)
    q = np.array(m.qpos0, np.float64)
    q[7:] += rng.uniform(-0.3, 0.3, m.nq - 7)
    s = orc.new_state(q, rng.uniform(-1, 1, m.nv), ctrl=rng.uniform(-1, 1, m.nu))
    orc.rollout(s, rng.uniform(-1, 1, (20, m.nu)))
    o = state_arrays(m, orc.forward(s))
    k = sr.kinematics(m, o["qpos"], o["qvel"], o["qacc"])
    np.testing.assert_allclose(k["x"], o["xpos"], atol=1e-12)
    for b in range(1, m.nbody):
        qr = sr.mat2quat(k["R"][b])
        assert min(np.abs(qr - o["xquat"][b]).max(), np.abs(qr + o["xquat"][b]).max()) < 1e-12
        # cvel: [angular; linear at the root's subtree com]
        np.testing.assert_allclose(k["w"][b], o["cvel"][b][:3], atol=1e-10)
        com = o["subtree_com"][int(m.body_rootid[b])]
        np.testing.assert_allclose(k["v"][b], o["cvel"][b][3:] + np.cross(o["cvel"][b][:3], o["xpos"][b] - com), atol=1e-10)
    # at rest on the floor the accelerometer reads -gravity in the site frame: zero velocity and acceleration
    k = sr.kinematics(m, m.qpos0)
    _, R, _, _, a = sr.frame(m, k, mjcf.OBJ_SITE, 0)
    np.testing.assert_allclose(R.T @ (a - m.gravity), R.T @ -np.asarray(m.gravity), atol=1e-14)
