"""Per-env model parameters without a GPU: the binding, the argument checks that need no device, the draw
(mjx_amd/randomize.py), the host side of the block builder under the sanitizers (tools/model_host_check.cpp
--params), and the precondition of the GPU physics check (tests/test_model_params_gpu.py, test 4): on the
tests' own draw the oracle's float32 instantiation stays within the parity tolerances of its float64 one."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import mjx_amd
from mjx_amd import _lib, abi, mjcf
from mjx_amd._header import HEADER
from mjx_amd.randomize import draw_model_params, pair_friction_from_geoms
from oracle import Oracle, state_arrays

from model_params_ref import MODELS, draw, substituted

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = HEADER.enums["MJL_ERR_ARG"]


def test_entry_points_are_bound_from_the_header():
    by_name = {n: (r, a) for r, n, a in HEADER.protos}
    assert by_name["mjl_model_param_dim"] == ("int", ["mjlModel*", "int"])
    assert by_name["mjl_batch_set_model_params"] == ("int", ["mjlBatch*", "float**", "float*", "void*"])
    assert by_name["mjl_batch_get_model_params"] == ("int", ["mjlBatch*", "int", "float*", "void*"])
    assert all(n in _lib.EXPORTS for n in by_name if "model_param" in n)
    assert abi.NMP == 6 and abi.OPT_PER_ENV_MODEL == 5
    assert abi.MODEL_PARAM == {"body_mass": 0, "body_inertia": 1, "dof_damping": 2, "dof_armature": 3,
                               "actuator_gear": 4, "pair_friction": 5}
    L = _lib.lib()
    vp = C.c_void_p
    assert L.mjl_batch_set_model_params.argtypes == [vp, vp, vp, vp]
    assert L.mjl_batch_get_model_params.argtypes == [vp, C.c_int, vp, vp]


def test_null_batch_is_an_argument_error():
    L = _lib.lib()
    table = (C.c_void_p * abi.NMP)()
    assert L.mjl_batch_set_model_params(None, table, None, None) == ARG
    assert L.mjl_batch_get_model_params(None, 0, None, None) == ARG
    assert L.mjl_batch_set_option(None, abi.OPT_PER_ENV_MODEL, 1) == ARG
    assert L.mjl_model_param_dim(None, 0) == -1


@pytest.mark.parametrize("name", MODELS)
def test_param_dims(name):
    m = mjx_amd.load_model(name)
    L, h = _lib.lib(), C.c_void_p()
    d = abi.model_desc(m)
    assert L.mjl_model_create(C.byref(d), C.byref(h)) == 0
    want = {"body_mass": m.nbody, "body_inertia": m.nbody * 6, "dof_damping": m.nv, "dof_armature": m.nv,
            "actuator_gear": m.nu, "pair_friction": m.npair}
    for k, dim in want.items():
        assert L.mjl_model_param_dim(h, abi.MODEL_PARAM[k]) == dim, k
    for bad in (-1, abi.NMP, 99):
        assert L.mjl_model_param_dim(h, bad) == -1
    L.mjl_model_destroy(h)


@pytest.mark.parametrize("name", MODELS)
def test_draw_shapes_and_unit_scales(name):
    m = mjx_amd.load_model(name)
    n = 5
    p = draw_model_params(m, n, {"mass": (0.5, 1.5), "friction": (0.3, 1.5), "damping": (0.5, 2), "armature": (0.5, 2),
                                 "gear": (0.7, 1.3)}, seed=3)
    shapes = {"body_mass": (n, m.nbody), "body_inertia": (n, m.nbody, 6), "dof_damping": (n, m.nv),
              "dof_armature": (n, m.nv), "actuator_gear": (n, m.nu), "pair_friction": (n, m.npair)}
    assert {k: tuple(v.shape) for k, v in p.items()} == shapes
    assert all(v.dtype == torch.float32 and v.is_contiguous() and v.device.type == "cpu" for v in p.values())
    assert len({tuple(r.tolist()) for r in p["body_mass"]}) == n  # a draw of its own per env
    # scales of 1, given as ranges or left out: the compiled model's fields, exactly
    for ranges in ({k: (1.0, 1.0) for k in ("mass", "friction", "damping", "armature", "gear")}, {}):
        one = draw_model_params(m, n, ranges, seed=1)
        ref = {"body_mass": m.body_mass, "body_inertia": np.reshape(m.body_inertia, (m.nbody, 6)),
               "dof_damping": m.dof_damping, "dof_armature": m.dof_armature, "actuator_gear": m.actuator_gear,
               "pair_friction": np.reshape(m.pair_friction, (-1, 5))[:, 0]}
        for k, v in one.items():
            for e in range(n):
                np.testing.assert_array_equal(v[e].numpy(), np.float32(ref[k]), err_msg=k)
    # the inertia scales with the mass, per body
    with np.errstate(invalid="ignore", divide="ignore"):
        sm = p["body_mass"].numpy().astype(np.float64) / np.asarray(m.body_mass)[None]
        si = p["body_inertia"].numpy().astype(np.float64) / np.reshape(m.body_inertia, (1, m.nbody, 6))
    for b in range(1, m.nbody):
        assert 0.5 <= sm[:, b].min() and sm[:, b].max() <= 1.5
        ok = np.isfinite(si[:, b])
        np.testing.assert_allclose(si[:, b][ok], np.broadcast_to(sm[:, b, None], si[:, b].shape)[ok], rtol=1e-6)
    assert draw_model_params(m, n, {"mass": (0.5, 1.5)}, seed=3)["body_mass"].equal(p["body_mass"])  # reproducible
    with pytest.raises(ValueError):
        draw_model_params(m, n, {"masses": (0.5, 1.5)})


def test_pair_friction_takes_the_larger_scaled_geom():
    """Two geoms, by hand: floor 1.0 against ball 0.6. Scales (0.5, 1.5) -> max(0.5, 0.9) = 0.9; scales
    (1.2, 0.5) -> max(1.2, 0.3) = 1.2; scales of 1 -> the compiled pair value max(1.0, 0.6) = 1.0."""
    m = mjcf.compile_xml_string("""<mujoco><worldbody>
        <geom name="floor" type="plane" size="5 5 .1" friction="1.0 0.005 0.0001"/>
        <body pos="0 0 1"><freejoint/><geom name="ball" type="sphere" size=".1" friction="0.6 0.005 0.0001"/></body>
        </worldbody></mujoco>""")
    assert m.npair == 1 and m.pair_friction[0][0] == 1.0
    floor, ball = m.names["geom"].index("floor"), m.names["geom"].index("ball")
    s = np.ones((3, m.ngeom))
    s[0, floor], s[0, ball] = 0.5, 1.5
    s[1, floor], s[1, ball] = 1.2, 0.5
    np.testing.assert_allclose(pair_friction_from_geoms(m, s)[:, 0], [0.9, 1.2, 1.0], rtol=0, atol=1e-15)


def test_host_side_under_the_sanitizers(tmp_path):
    """tools/model_host_check.cpp --params: model_build on substituted descriptors and model_param_stage, as a
    stand-alone program built with the host compiler's address and undefined-behaviour sanitizers."""
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "model_host_check"
    cc = subprocess.run([cxx, "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                         os.path.join(ROOT, "tools", "model_host_check.cpp")], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    files = []
    for name in MODELS:
        files.append(str(tmp_path / (name + ".desc")))
        with open(files[-1], "wb") as fh:
            fh.write(bytes(abi.model_desc(mjx_amd.load_model(name))))
    run = subprocess.run([str(exe), "--params"] + files, capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.stdout, run.stderr[-4000:])
    assert run.stdout.splitlines() == [f + "\tparams=ok" for f in files]


def _rel(got, ref):
    return np.abs(np.asarray(got, np.float64) - ref).max() / (1.0 + np.abs(ref).max())


@pytest.mark.parametrize("name", MODELS)
def test_float32_oracle_within_the_parity_tolerances_on_the_draw(name):
    """The GPU physics check compares a float32 kernel with the float64 oracle on randomised models at
    tests/test_gpu_parity.py's tolerances. That is a fair demand only if float32 arithmetic as such stays within
    them on these models: the oracle's own float32 instantiation against its float64 one, every env of the
    draw, forward and one step."""
    from test_gpu_parity import _states
    m = mjx_amd.load_model(name)
    states = _states(m)
    p = draw(m, len(states))
    worst = {}
    for i, (q, v, w, c) in enumerate(states):
        sub = substituted(name, p, i)
        o64, o32 = Oracle(sub), Oracle(sub, use_float=True)
        a, b = (state_arrays(sub, o.forward(o.new_state(q, v, w, c))) for o in (o64, o32))
        assert (a["ncon"], a["nefc"]) == (b["ncon"], b["nefc"]), f"env {i}: counts"
        for f, tol in (("qfrc_bias", 2e-5), ("qfrc_passive", 2e-5), ("qfrc_actuator", 2e-5), ("qacc", 2e-3),
                       ("qfrc_constraint", 2e-3)):
            worst[f] = max(worst.get(f, 0), _rel(b[f], a[f]) / tol)
        a, b = (state_arrays(sub, o.step(o.new_state(q, v, w, c))) for o in (o64, o32))
        worst["qpos"] = max(worst.get("qpos", 0), np.abs(b["qpos"] - a["qpos"]).max() / 2e-5)
        for f in ("qvel", "qacc_warmstart"):
            worst[f] = max(worst.get(f, 0), _rel(b[f], a[f]) / 2e-3)
    print({k: round(float(v), 4) for k, v in worst.items()})  # fraction of each tolerance used
    assert max(worst.values()) <= 1.0, worst


def test_train_ppo_flags():
    """--rand-* are off by default (PPOTrainer gets randomize=None: no option set, no new kernel) and map to
    the draw's range names."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("train_ppo_cli", os.path.join(ROOT, "mujoco-mjx-lab_amd", "train_ppo.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    assert cli.randomize_config(cli.parse_args([])) is None
    a = cli.parse_args(["--rand-mass", "0.5", "1.5", "--rand-friction", "0.3", "1.5", "--rand-gear", "0.7", "1.3"])
    assert cli.randomize_config(a) == {"mass": (0.5, 1.5), "friction": (0.3, 1.5), "gear": (0.7, 1.3)}
    a = cli.parse_args(["--rand-damping", "0.5", "2", "--rand-armature", "0.5", "2"])
    r = cli.randomize_config(a)
    assert r == {"damping": (0.5, 2.0), "armature": (0.5, 2.0)}
    m = mjx_amd.load_model("humanoid_mjx")
    assert draw_model_params(m, 2, r, 0)["dof_damping"].shape == (2, m.nv)
