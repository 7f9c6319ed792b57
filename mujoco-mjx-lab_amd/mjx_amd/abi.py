"""The C ABI's constants and structs as ctypes, and conversion from compiled models.

Nothing here is declared twice: the capacities, `AUX_DIM`, the `OPT_*` and `FIELD` numbers and the
fields of `ModelDesc` / `EnvConfigC` / `VisualDesc` are read from include/mjx355.h (`_header.py`), the header the
library is built from and stamped with. `tests/test_abi.py` checks the layouts against a C compiler.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._header import HEADER, SCALARS

_D, _E = HEADER.defines, HEADER.enums
# MAXBODY ... MAXOBS and AUX_DIM (#define MJL_*); OPT_STORE_DERIVED ... OPT_VJP_TAPE (enum MJL_OPT_*)
globals().update({k[4:]: v for k, v in _D.items()})
globals().update({k[4:]: v for k, v in _E.items() if k.startswith("MJL_OPT_")})
# per-env fields of mjl_get / mjl_set by lower-case name ("qpos": MJL_FIELD_QPOS, ...)
FIELD = {k[10:].lower(): v for k, v in _E.items() if k.startswith("MJL_FIELD_")}

# per-env model parameters of mjl_batch_set_model_params by field name ("body_mass": MJL_MP_BODY_MASS, ...)
MODEL_PARAM = {k[7:].lower(): v for k, v in _E.items() if k.startswith("MJL_MP_")}

# exponent-carried cotangents (mjl_vjp_scale_attach): log2 of the output magnitude from which an env's
# cotangents are rescaled, and the range the library accepts
VJP_SCALE_THRESHOLD_LOG2 = 40
VJP_SCALE_THRESHOLD_RANGE = (0, 96)


def _fields(struct: str):
    out = []
    for name, t, dims in HEADER.structs[struct]:
        ct = SCALARS[t]
        for d in reversed(dims):
            ct = ct * d
        out.append((name, ct))
    return out


class ModelDesc(C.Structure):
    _fields_ = _fields("mjlModelDesc")


class EnvConfigC(C.Structure):
    _fields_ = _fields("mjlEnvConfig")


class VisualDesc(C.Structure):
    _fields_ = _fields("mjlVisualDesc")


CAM_MODE = {k[8:].lower(): v for k, v in _E.items() if k.startswith("MJL_CAM_")}  # "fixed": MJL_CAM_FIXED, ...
RENDER_SHADOWS = _E["MJL_RENDER_SHADOWS"]


_PY = {C.c_int32: int, C.c_float: float, C.c_double: float}  # what a scalar field is set through
_CAP = {n: _D["MJL_MAX" + c] for n, c in (
    ("nbody", "BODY"), ("njnt", "JNT"), ("nv", "V"), ("nq", "Q"), ("ngeom", "GEOM"), ("npair", "PAIR"),
    ("nsite", "SITE"), ("nu", "U"), ("ntendon", "TENDON"), ("nsensor", "SENSOR"),
    ("nrsensor", "RSENSOR"), ("nrsensordata", "RSENSORDATA"))}
# readout sensors (mjl_sensors): "gyro": MJL_SENS_GYRO, ...; "pos" / "vel" / "acc": MJL_SENS_STAGE_*
SENSOR_TYPE = {k[9:].lower(): v for k, v in _E.items() if k.startswith("MJL_SENS_") and not k.startswith("MJL_SENS_STAGE_")}
SENSOR_STAGE = {k[15:].lower(): v for k, v in _E.items() if k.startswith("MJL_SENS_STAGE_")}
SENSOR_OBJ = {k[8:].lower(): v for k, v in _E.items() if k.startswith("MJL_OBJ_")}
RAY_STATIC = _E["MJL_RAY_STATIC"]  # mjl_ray / mjl_ray_scan flags
SCAN_ALIGN = {k[9:].lower(): v for k, v in _E.items() if k.startswith("MJL_SCAN_")}  # "pose", "yaw"
JAC_TANGENT = _E["MJL_JAC_TANGENT"]  # mjl_step_jacobian flags
# mjl_jac: "world", "local"
JAC_FRAME = {k[8:].lower(): v for k, v in _E.items() if k.startswith("MJL_JAC_") and k != "MJL_JAC_TANGENT"}
INV_DISCRETE = _E["MJL_INV_DISCRETE"]  # mjl_inverse flags
IK_LIMITS = _E["MJL_IK_LIMITS"]  # mjl_ik flags


class UnsupportedModel(ValueError):
    pass


def model_desc(m) -> ModelDesc:
    """Pack a CompiledModel into the C descriptor (range-checked against the capacities)."""
    if any(getattr(m, n) > cap for n, cap in _CAP.items()):
        raise UnsupportedModel("model exceeds kernel capacities (see include/mjx355.h MJL_MAX*)")
    d = ModelDesc()
    for name, ct in ModelDesc._fields_:
        if ct in _PY:
            setattr(d, name, _PY[ct](getattr(m, name)))
        elif name == "gravity":
            _fill(d.gravity, m.gravity)
        elif name in m.arrays:
            _fill(getattr(d, name), m.arrays[name])
    return d


def _fill(carr, arr):
    arr = np.asarray(arr)
    if arr.ndim == 1:
        for i, v in enumerate(arr):
            carr[i] = v.item()
    elif arr.ndim == 2:
        if arr.shape[1] > len(carr[0]):
            raise UnsupportedModel("array exceeds capacity")
        for i in range(arr.shape[0]):
            row = carr[i]
            for j in range(arr.shape[1]):
                row[j] = arr[i, j].item()


def visual_desc(m) -> VisualDesc:
    """Pack a CompiledModel's visual description (mjcf._compile_visual) into the C descriptor. A camera the
    renderer cannot take (mjcf.camera_id raises for it) keeps its slot with mode -1."""
    v = m.visual
    if v is None:
        raise UnsupportedModel("model has no visual description (compile it from MJCF)")
    if len(v["cameras"]) > MAXCAM:
        raise UnsupportedModel(f"model has {len(v['cameras'])} cameras (MJL_MAXCAM = {MAXCAM})")
    d = VisualDesc()
    d.ncam = len(v["cameras"])
    _fill(d.geom_rgba, np.asarray(v["geom_rgba"], float).reshape(-1, 4))
    ck = v["checker"]
    d.checker_geom = -1 if ck is None else int(ck["geom"])
    if ck is not None:
        for name in ("rgb1", "rgb2", "cell", "xaxis", "yaxis"):
            _fill(getattr(d, "checker_" + name), np.asarray(ck[name], float))
    _fill(d.sky_rgb1, np.asarray(v["sky"]["rgb1"], float))
    _fill(d.sky_rgb2, np.asarray(v["sky"]["rgb2"], float))
    d.light_directional = int(v["light"]["directional"])
    for name in ("pos", "dir", "diffuse", "ambient"):
        _fill(getattr(d, "light_" + name), np.asarray(v["light"][name], float))
    d.znear, d.zfar = float(v["znear"]), float(v["zfar"])
    for i, c in enumerate(v["cameras"]):
        d.cam_body[i] = int(c["body"])
        d.cam_mode[i] = -1 if c["error"] else CAM_MODE[c["mode"]]
        d.cam_fovy[i] = float(c["fovy"])
        pos0 = c["pos0_trackcom"] if c["mode"] == "trackcom" else c["pos0_track"]
        for k in range(3):
            d.cam_pos[i][k], d.cam_pos0[i][k] = float(c["pos"][k]), float(pos0[k])
        for k in range(9):
            d.cam_mat[i][k], d.cam_mat0[i][k] = float(c["mat"][k]), float(c["mat0"][k])
    return d


def desc_size() -> int:
    return C.sizeof(ModelDesc)


def env_config_c(cfg, m, obs_dim: int) -> EnvConfigC:
    """EnvConfig (src/config.py:29-66) -> C struct, building the flip tables the way
    create_env_functions does (reference src/envs.py:48-74)."""
    c = EnvConfigC()
    tables = dict(zip(("act_perm", "act_sign", "obs_perm", "obs_sign"), flip_tables(cfg, m.nu, obs_dim)))
    for name, ct in EnvConfigC._fields_:
        if name in tables:
            _fill(getattr(c, name), tables[name])
        elif name == "obs_dim":
            c.obs_dim = int(obs_dim)
        elif name == "random_flip":
            c.random_flip = int(bool(cfg.random_flip))
        else:
            setattr(c, name, _PY[ct](getattr(cfg, name)))
    return c


def flip_tables(cfg, nu: int, obs_dim: int):
    """act_perm/act_sign/obs_perm/obs_sign exactly as reference src/envs.py:48-74."""
    act_perm = np.arange(nu)
    act_sign = np.ones(nu, np.float32)
    obs_perm = np.arange(obs_dim)
    obs_sign = np.ones(obs_dim, np.float32)
    if cfg.random_flip:
        r, l = np.array(cfg.flip_action_right), np.array(cfg.flip_action_left)
        act_perm[r] = l
        act_perm[l] = r
        act_sign[np.array(cfg.flip_action_sign)] = -1.0
        ro, lo = np.array(cfg.flip_obs_right), np.array(cfg.flip_obs_left)
        obs_perm[ro] = lo
        obs_perm[lo] = ro
        obs_sign[np.array(cfg.flip_obs_sign)] = -1.0
    return act_perm, act_sign, obs_perm, obs_sign
