"""General actuators off the GPU: the MJCF compiler (<position>, <velocity>, <general>), the MjModel filler,
pd_actuators, and the host model build (mjl_model_create and tools/model_host_check.cpp alone under the host
sanitizers): accepted and refused descriptors, and the motor block left as it was."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import mjx_amd
from mjx_amd import _lib, abi, actuators, mjcf
from mjx_amd.mjmodel import compile_mjmodel

from test_mjmodel import _fake_mujoco, _mjmodel_view
from test_model_host import ARG, OK, ROOT, UNSUPPORTED, _compiler, _create

NEW = ("actuator_kind", "actuator_gain", "actuator_biasprm", "actuator_forcelimited", "actuator_forcerange")

BODY = """<worldbody><body pos="0 0 1">
  <joint name="a" type="hinge" axis="0 1 0" range="-30 60"/>
  <geom type="capsule" fromto="0 0 0 .4 0 0" size=".03"/>
  <body pos=".4 0 0"><joint name="b" type="hinge" axis="0 1 0" range="-90 10"/>
    <geom type="capsule" fromto="0 0 0 .3 0 0" size=".03"/>
    <body pos=".3 0 0"><joint name="c" type="hinge" axis="0 0 1"/>
      <geom type="capsule" fromto="0 0 0 .2 0 0" size=".02"/></body></body></body></worldbody>"""

XML = f"""<mujoco>
  <default>
    <position kp="40" kv="3" forcerange="-20 20"/>
    <default class="soft"><position kp="10" kv="0"/><general gear="2"/></default>
  </default>{BODY}
  <actuator>
    <position name="pa" joint="a" inheritrange="0.5"/>
    <velocity name="va" joint="a" kv="5" gear="3" ctrlrange="-1 1"/>
    <position name="pb" joint="b" class="soft" ctrlrange="-2 2" ctrllimited="false" forcelimited="false"/>
    <general name="gc" joint="c" class="soft" gainprm="7" biastype="affine" biasprm="1.5 -7 -0.25" forcerange="-4 9"/>
    <general name="gn" joint="c" gainprm="2" biasprm="1 2 3"/>
    <motor name="mc" joint="c" gear="11" ctrlrange="-.4 .4"/>
  </actuator></mujoco>"""


def _one(actuator):
    return f"<mujoco>{BODY}<actuator>{actuator}</actuator></mujoco>"


def test_mjcf_compiles_position_velocity_general():
    m = mjcf.compile_xml_string(XML)
    assert m.nu == 6 and m.names["actuator"] == ["pa", "va", "pb", "gc", "gn", "mc"]
    np.testing.assert_array_equal(m.actuator_trnid, [0, 0, 1, 2, 2, 2])  # two actuators on joint a, three on c
    np.testing.assert_array_equal(m.actuator_kind, [1, 1, 1, 1, 1, 0])
    np.testing.assert_array_equal(m.actuator_gear, [1, 3, 1, 2, 1, 11])
    np.testing.assert_array_equal(m.actuator_gain, [40, 5, 10, 7, 2, 1])
    # position: (0, -kp, -kv); velocity: (0, 0, -kv); general: biasprm when affine, none otherwise; motor: none
    np.testing.assert_array_equal(m.actuator_biasprm, [[0, -40, -3], [0, 0, -5], [0, -10, 0], [1.5, -7, -0.25],
                                                       [0, 0, 0], [0, 0, 0]])
    # inheritrange 0.5 of the joint's (-30, 60) degrees: mean 15, half-width 45 * 0.5
    lo, hi = np.deg2rad(15 - 22.5), np.deg2rad(15 + 22.5)
    np.testing.assert_allclose(m.actuator_ctrlrange, [[lo, hi], [-1, 1], [-2, 2], [0, 0], [0, 0], [-.4, .4]], atol=1e-15)
    np.testing.assert_array_equal(m.actuator_ctrllimited, [1, 1, 0, 0, 0, 1])
    # forcerange from the <default> block's <position>, off where the element says so, auto elsewhere
    np.testing.assert_array_equal(m.actuator_forcelimited, [1, 0, 0, 1, 0, 0])
    np.testing.assert_array_equal(m.actuator_forcerange, [[-20, 20], [0, 0], [-20, 20], [-4, 9], [0, 0], [0, 0]])
    d = abi.model_desc(m)
    assert list(d.actuator_kind[:6]) == [1, 1, 1, 1, 1, 0] and d.actuator_biasprm[3][2] == -0.25
    assert d.actuator_forcerange[3][1] == 9 and d.actuator_gain[1] == 5 and d.actuator_forcelimited[0] == 1


def test_motor_only_models_carry_no_new_arrays():
    m = mjcf.compile_xml_string(_one('<motor joint="a" gear="5" ctrlrange="-1 1"/>'))
    assert not set(NEW) & set(m.arrays)
    for name in ("humanoid", "humanoid_mjx"):
        assert not set(NEW) & set(mjx_amd.load_model(name).arrays)


@pytest.mark.parametrize("actuator,fragment", [
    ('<position joint="a" kp="1" dampratio="1"/>', "dampratio"),
    ('<position joint="a" kp="1" timeconst="0.1"/>', "timeconst"),
    ('<general joint="a" dyntype="integrator"/>', "dyntype"),
    ('<general joint="a" dyntype="filter"/>', "dyntype"),
    ('<general joint="a" gaintype="affine"/>', "gaintype"),
    ('<general joint="a" gaintype="muscle"/>', "gaintype"),
    ('<general joint="a" biastype="muscle"/>', "biastype"),
    ('<general joint="a" biastype="user"/>', "biastype"),
    ('<intvelocity joint="a"/>', "intvelocity"), ('<damper joint="a"/>', "damper"), ('<muscle joint="a"/>', "muscle"),
    ('<cylinder joint="a"/>', "cylinder"), ('<adhesion body="x"/>', "adhesion"),
    ('<position tendon="t"/>', "tendon"), ('<velocity site="s"/>', "site"), ('<general body="x"/>', "body"),
    ('<general jointinparent="a"/>', "jointinparent"),
])
def test_mjcf_rejections_name_the_attribute(actuator, fragment):
    with pytest.raises(mjcf.MJCFError, match=fragment):
        mjcf.compile_xml_string(_one(actuator))


def test_pd_actuators_fields():
    m = mjx_amd.load_model("humanoid_mjx")
    before = {k: v.copy() for k, v in m.arrays.items()}
    nu = m.nu
    q0 = m.qpos0[m.jnt_qposadr[m.actuator_trnid]]
    lim = np.abs(m.actuator_gear) * np.abs(m.actuator_ctrlrange).max(1)
    p = actuators.pd_actuators(m, 30.0, 2.0, 0.5)
    np.testing.assert_array_equal(p.actuator_kind, np.ones(nu))
    np.testing.assert_array_equal(p.actuator_gain, np.full(nu, 15.0))
    np.testing.assert_array_equal(p.actuator_biasprm, np.stack([30.0 * q0, np.full(nu, -30.0), np.full(nu, -2.0)], 1))
    np.testing.assert_array_equal(p.actuator_gear, np.ones(nu))
    np.testing.assert_array_equal(p.actuator_ctrlrange, m.actuator_ctrlrange)
    np.testing.assert_array_equal(p.actuator_ctrllimited, m.actuator_ctrllimited)
    np.testing.assert_array_equal(p.actuator_forcerange, np.stack([-lim, lim], 1))
    np.testing.assert_array_equal(p.actuator_forcelimited, m.actuator_ctrllimited)
    assert lim.min() > 0 and p.nu == nu and p.names == m.names
    rng = np.random.default_rng(0)
    kp, kv, sc = rng.uniform(5, 50, nu), rng.uniform(0, 3, nu), rng.uniform(0.2, 1, nu)
    p = actuators.pd_actuators(m, kp, kv, sc)
    np.testing.assert_array_equal(p.actuator_gain, kp * sc)
    np.testing.assert_array_equal(p.actuator_biasprm, np.stack([kp * q0, -kp, -kv], 1))
    p1 = actuators.pd_actuators(m, kp, 1.0)  # action_scale defaults to 1
    np.testing.assert_array_equal(p1.actuator_gain, kp)
    for k, v in before.items():  # the source model is untouched
        np.testing.assert_array_equal(m.arrays[k], v, err_msg=k)
    assert set(m.arrays) == set(before) and actuators.has_general_actuators(p) and not actuators.has_general_actuators(m)
    with pytest.raises(ValueError, match="kp"):
        actuators.pd_actuators(m, np.ones(nu + 1), 1.0)
    with pytest.raises(mjcf.MJCFError, match="already"):
        actuators.pd_actuators(p, 1.0, 1.0)


def test_train_ppo_pd_control_flag():
    import importlib.util
    spec = importlib.util.spec_from_file_location("train_ppo_cli", os.path.join(ROOT, "mujoco-mjx-lab_amd", "train_ppo.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    m = mjx_amd.load_model("humanoid_mjx")
    assert cli.control_model(cli.parse_args([]), m) is m  # off by default
    p = cli.control_model(cli.parse_args(["--pd-control", "30", "2", "--action-scale", "0.5"]), m)
    np.testing.assert_array_equal(p.actuator_gain, np.full(m.nu, 15.0))
    np.testing.assert_array_equal(p.actuator_biasprm[:, 2], np.full(m.nu, -2.0))
    with pytest.raises(SystemExit):
        cli.parse_args(["--action-scale", "0.5"])


# ------------------------------------------------------------------------------------------------ mjmodel.py
def _general_view(m):
    """test_mjmodel's MjModel-shaped view, with MuJoCo's actuator arrays for the general fields."""
    v, mod = _mjmodel_view(m), _fake_mujoco(m)
    mod.mjtBias.mjBIAS_AFFINE, mod.mjtBias.mjBIAS_MUSCLE = 1, 2
    nu = m.nu
    A = m.arrays
    v.actuator_gainprm = np.zeros((nu, 10))
    v.actuator_gainprm[:, 0] = A["actuator_gain"]
    v.actuator_biasprm = np.zeros((nu, 10))
    v.actuator_biasprm[:, :3] = A["actuator_biasprm"]
    v.actuator_biastype = np.where(np.any(A["actuator_biasprm"] != 0, 1), 1, 0).astype(np.int32)
    v.actuator_forcelimited, v.actuator_forcerange = A["actuator_forcelimited"], A["actuator_forcerange"]
    return v, mod


def test_mjmodel_accepts_affine_bias_gain_and_forcerange():
    m = actuators.pd_actuators(mjx_amd.load_model("humanoid_mjx"), 30.0, 2.0, 0.5)
    m.arrays["actuator_kind"][3] = 0  # one motor among them: gain 1, no bias, no force limit
    m.arrays["actuator_gain"][3], m.arrays["actuator_biasprm"][3], m.arrays["actuator_forcelimited"][3] = 1.0, 0.0, 0
    m.arrays["actuator_forcerange"][3] = 0.0
    m.arrays["actuator_biasprm"][5] = 0.0  # and a pure gain (bias none, gain 15)
    v, mod = _general_view(m)
    got = compile_mjmodel(v, mod)
    for k in NEW + ("actuator_gear", "actuator_trnid", "actuator_ctrlrange", "actuator_ctrllimited"):
        np.testing.assert_array_equal(got.arrays[k], m.arrays[k], err_msg=k)
    assert bytes(abi.model_desc(got))[abi.ModelDesc.actuator_kind.offset:abi.ModelDesc.tendon_num.offset] == \
        bytes(abi.model_desc(m))[abi.ModelDesc.actuator_kind.offset:abi.ModelDesc.tendon_num.offset]
    v.actuator_biastype = v.actuator_biastype.copy()
    v.actuator_biastype[0] = 2
    with pytest.raises(mjcf.MJCFError, match="biastype"):
        compile_mjmodel(v, mod)
    v, mod = _general_view(m)
    v.actuator_gaintype = np.ones(m.nu, np.int32)
    with pytest.raises(mjcf.MJCFError, match="gaintype"):
        compile_mjmodel(v, mod)
    v, mod = _general_view(m)
    v.actuator_dyntype = np.ones(m.nu, np.int32)
    with pytest.raises(mjcf.MJCFError, match="dyntype"):
        compile_mjmodel(v, mod)


# ------------------------------------------------------------------------------------------------ host model build
# sha256 of the model block mjl_model_create built of each humanoid before general actuators existed (45936 bytes)
MOTOR_BLOCK = {"humanoid": "f7201c37ac57ebcb526fb4d0a6c6b274143afddeb27524b139633125a75b7314",
               "humanoid_mjx": "5d573821f99918e0131b0735de1cc47ec7bc656cf4f60f116612450631defbab"}
MOTOR_BLOCK_BYTES = 45936


def _pd_desc(name="humanoid_mjx"):
    return abi.model_desc(actuators.pd_actuators(mjx_amd.load_model(name), 30.0, 2.0, 0.5))


def _mut(field, value, *idx):
    def mutate(d):
        a = getattr(d, field)
        for i in idx[:-1]:
            a = a[i]
        a[idx[-1]] = value
    return mutate


def _empty_range(d):
    d.actuator_forcerange[4][0], d.actuator_forcerange[4][1] = 3.0, -3.0


def _empty_range_unlimited(d):
    _empty_range(d)
    d.actuator_forcelimited[4] = 0


BAD = [
    ("gain_nan", _mut("actuator_gain", float("nan"), 2), ARG, "actuator 2: gain, biasprm and forcerange must be finite"),
    ("bias_inf", _mut("actuator_biasprm", float("inf"), 7, 1), ARG, "actuator 7: gain"),
    ("range_nan", _mut("actuator_forcerange", float("nan"), 0, 1), ARG, "actuator 0: gain"),
    ("range_empty", _empty_range, ARG, "actuator 4: forcerange [3, -3] is empty"),
    ("kind_2", _mut("actuator_kind", 2, 5), UNSUPPORTED, "actuator 5: kind 2 not supported"),
    ("kind_neg", _mut("actuator_kind", -1, 5), UNSUPPORTED, "actuator 5: kind -1 not supported"),
]
GOOD = [("range_empty_unlimited", _empty_range_unlimited)]  # an unused range is not looked at


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("actuators_host")
    exe = tmp / "model_host_check"
    cc = subprocess.run([cxx, "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o",
                         str(exe), os.path.join(ROOT, "tools", "model_host_check.cpp")], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    cases = {n: abi.model_desc(mjx_amd.load_model(n)) for n in ("humanoid", "humanoid_mjx")}
    cases["pd"], cases["pd_humanoid"] = _pd_desc(), _pd_desc("humanoid")
    cases["mixed"] = abi.model_desc(mjcf.compile_xml_string(XML))
    pure = _pd_desc()
    for u in range(pure.nu):
        pure.actuator_biasprm[u][2] = 0.0
    cases["stiffness_only"] = pure
    for case, mutate, *_ in BAD + GOOD:
        cases[case] = _pd_desc()
        mutate(cases[case])
    files = {}
    for case, d in cases.items():
        files[case] = str(tmp / (case + ".desc"))
        with open(files[case], "wb") as fh:
            fh.write(bytes(d))

    def run(*args):
        r = subprocess.run([str(exe), *args], capture_output=True, text=True)
        assert r.stderr == "", r.stderr[-4000:]  # a clean sanitizer exit
        return r
    return cases, files, run


def test_model_create_accepts_and_refuses_alike_alone_and_in_the_library(host):
    cases, files, run = host
    L = _lib.lib()
    r = run(*files.values())
    assert r.returncode == 0
    for (case, d), line in zip(cases.items(), r.stdout.splitlines()):
        col = line.split("\t")
        alone = (int(col[1].split("=")[1]), col[5].split("=", 1)[1], int(col[2].split("=")[1]), int(col[3].split("=")[1]))
        assert _create(L, d) == alone, case
        want = {c: (code, frag) for c, _, code, frag in BAD}.get(case, (OK, ""))
        assert alone[0] == want[0] and want[1] in alone[1], (case, alone)
    # the row and contact capacities do not depend on the actuators
    assert _create(L, cases["pd"])[2:] == _create(L, cases["humanoid_mjx"])[2:]


def test_motor_block_is_byte_identical_and_general_flags(host):
    cases, files, run = host
    names = ("humanoid", "humanoid_mjx", "pd", "pd_humanoid", "mixed", "stiffness_only")
    r = run("--block", *(files[n] for n in names))
    assert r.returncode == 0
    info = {}
    for n, line in zip(names, r.stdout.splitlines()):
        info[n] = dict(c.split("=") for c in line.split("\t")[1:])
        assert info[n]["rc"] == "0" and int(info[n]["motor_bytes"]) == MOTOR_BLOCK_BYTES
    for n in ("humanoid", "humanoid_mjx"):  # descriptors that do not know the new fields: all zero there
        d = cases[n]
        assert not any(d.actuator_kind) and not any(d.actuator_gain) and not any(d.actuator_forcelimited)
        block = open(files[n] + ".block", "rb").read()
        assert len(block) == int(info[n]["sizeof_ModelF"])
        assert hashlib.sha256(block[:MOTOR_BLOCK_BYTES]).hexdigest() == MOTOR_BLOCK[n]
        assert not any(block[MOTOR_BLOCK_BYTES:])  # and nothing after it
        assert (info[n]["act_general"], info[n]["act_b2"]) == ("0", "0")
    assert (info["pd"]["act_general"], info["pd"]["act_b2"]) == ("1", "1")
    assert (info["mixed"]["act_general"], info["mixed"]["act_b2"]) == ("1", "1")
    assert (info["stiffness_only"]["act_general"], info["stiffness_only"]["act_b2"]) == ("1", "0")
    # everything a motor model has is the same in the PD model's block but the gear (1 instead of the motor's)
    a = open(files["humanoid_mjx"] + ".block", "rb").read()[:MOTOR_BLOCK_BYTES]
    b = open(files["pd"] + ".block", "rb").read()[:MOTOR_BLOCK_BYTES]
    diff = np.flatnonzero(np.frombuffer(a, np.uint8) != np.frombuffer(b, np.uint8))
    assert 0 < len(diff) and diff.max() - diff.min() < 4 * abi.MAXU


def test_per_env_parameters_host_side_on_general_descriptors(host):
    """tools/model_host_check --params on general descriptors: a substituted gear or damping leaves no stale
    derived value anywhere in the block (the kernels derive length, velocity, moment and gear^2 b2 from the
    block's one gear)."""
    cases, files, run = host
    r = run("--params", files["pd"], files["pd_humanoid"], files["mixed"])
    assert r.returncode == 0, r.stdout
    assert [line.split("\t")[1] for line in r.stdout.splitlines()] == ["params=ok"] * 3
