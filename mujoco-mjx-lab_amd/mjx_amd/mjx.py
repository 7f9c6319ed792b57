"""mjx-shaped front end over the native library (the reference calls `mujoco.mjx`).

    reference                                   here
    mujoco.MjModel.from_xml_path(path)          mjcf.load_model(path)       (host compile)
    mjx.put_model(m)            training_utils.py:105      put_model(m)    -> Model (constants)
    mjx.make_data(sys) (vmapped)   envs.py:110             make_data(sys, nenv, device) -> Data
    mjx.forward(sys, d)            envs.py:112             forward(sys, d, mask=None)
    mjx.step(sys, d)               envs.py:345             step(sys, d, ctrl=None)

Differences forced by a batched, device-resident design: `Data` is a handle to state owned by the
library (one row per env, all envs in one HBM slab), `forward`/`step` update it in place and
return it, and fields are read/written as torch tensors on the batch's GPU.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import NamedTuple, Optional

import torch

from . import abi, mjcf
from ._lib import MjlError, check, lib


def _stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t: Optional[torch.Tensor]):
    if t is None:
        return None
    if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
        raise MjlError("device buffers must be contiguous float32 CUDA tensors")
    return C.c_void_p(t.data_ptr())


class Model:
    """Device-ready model (mjx.Model analog). Holds the compiled constants and the C handle."""

    def __init__(self, compiled: mjcf.CompiledModel):
        self.m = compiled
        self.desc = abi.model_desc(compiled)
        h = C.c_void_p()
        check(lib().mjl_model_create(C.byref(self.desc), C.byref(h)))
        self._h = h
        self.nq, self.nv, self.nu, self.nbody = compiled.nq, compiled.nv, compiled.nu, compiled.nbody
        self.nsensordata = compiled.nsensordata
        self.timestep = compiled.timestep

    @property
    def handle(self):
        return self._h

    @property
    def nefc_max(self) -> int:
        return lib().mjl_model_nefc_max(self._h)

    @property
    def ncon_max(self) -> int:
        """Most contacts one env can have: one per candidate pair, two per plane-capsule pair."""
        return lib().mjl_model_ncon_max(self._h)

    @property
    def nrsensordata(self) -> int:
        """Width of a sensordata row of `sensors` (every sensor of the model, MuJoCo's Data.sensordata layout)."""
        return lib().mjl_model_nrsensordata(self._h)

    def sensor_slice(self, name: str) -> slice:
        """Where sensor `name` lies in a row of `sensors`."""
        return self.m.sensor_slice(name)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib().mjl_model_destroy(self._h)
                self._h = None
        except Exception:
            pass


_FIELD_DIM = {
    "qpos": lambda m: m.nq, "qvel": lambda m: m.nv, "qacc_warmstart": lambda m: m.nv, "time": lambda m: 1,
    "ctrl": lambda m: m.nu, "qacc": lambda m: m.nv, "xpos": lambda m: m.nbody * 3, "xquat": lambda m: m.nbody * 4,
    "qfrc_actuator": lambda m: m.nv, "sensordata": lambda m: max(1, m.nsensordata), "aux": lambda m: abi.AUX_DIM,
    "stats": lambda m: 4, "qfrc_bias": lambda m: m.nv, "qfrc_passive": lambda m: m.nv,
    "qfrc_constraint": lambda m: m.nv, "qacc_smooth": lambda m: m.nv,
}


class Data:
    """Batched simulation state (mjx.Data with a leading env axis), owned by the library in HBM."""

    def __init__(self, model: Model, nenv: int, device: int = 0):
        if not torch.cuda.is_available():
            raise MjlError("mjx355 needs a GPU (torch.cuda.is_available() is False)")
        self.model = model
        self.nenv = int(nenv)
        self.device = torch.device("cuda", device)
        h = C.c_void_p()
        check(lib().mjl_batch_create(model.handle, self.nenv, int(device), C.byref(h)))
        self._h = h

    @property
    def handle(self):
        return self._h

    def set_option(self, option: int, value: int):
        check(lib().mjl_batch_set_option(self._h, option, int(value)))

    def get(self, field: str) -> torch.Tensor:
        dim = _FIELD_DIM[field](self.model)
        out = torch.empty((self.nenv, dim), dtype=torch.float32, device=self.device)
        check(lib().mjl_get(self._h, abi.FIELD[field], _ptr(out), _stream()))
        if field == "xpos":
            return out.view(self.nenv, self.model.nbody, 3)
        if field == "xquat":
            return out.view(self.nenv, self.model.nbody, 4)
        if field == "time":
            return out.view(self.nenv)
        return out

    def set(self, field: str, value: torch.Tensor, mask: Optional[torch.Tensor] = None):
        dim = _FIELD_DIM[field](self.model)
        v = value.to(device=self.device, dtype=torch.float32).reshape(self.nenv, dim).contiguous()
        mk = None if mask is None else mask.to(device=self.device, dtype=torch.float32).contiguous()
        check(lib().mjl_set(self._h, abi.FIELD[field], _ptr(v), _ptr(mk), _stream()))

    def attach_applied(self, qfrc_applied: Optional[torch.Tensor] = None,
                       xfrc_applied: Optional[torch.Tensor] = None):
        """mjx.Data.qfrc_applied [nenv, nv] / xfrc_applied [nenv, nbody, 6] (world-frame force and torque at
        xipos; row 0 ignored): forward, forward_contacts, step and the env step read the tensors at
        execution time, so update them in place (`d.replace(xfrc_applied=x)` becomes `buf.copy_(x)`). Either
        may be None; both None detaches. The step VJPs raise while anything is attached."""
        for t, shape, what in ((qfrc_applied, (self.nenv, self.model.nv), "qfrc_applied"),
                               (xfrc_applied, (self.nenv, self.model.nbody, 6), "xfrc_applied")):
            if t is None:
                continue
            if tuple(t.shape) != shape:
                raise MjlError(f"{what} must have shape {shape}")
            if t.device != self.device:
                raise MjlError(f"{what} must live on {self.device}")
            _ptr(t)  # contiguous float32 CUDA
        check(lib().mjl_batch_attach_applied(self._h, _ptr(qfrc_applied), _ptr(xfrc_applied)))
        self._applied = (qfrc_applied, xfrc_applied)  # keep the buffers alive while the library points at them

    def detach_applied(self):
        self.attach_applied(None, None)

    def enable_model_params(self, on: bool = True):
        """Give every env a model block of its own (MJL_OPT_PER_ENV_MODEL; nenv x ~46 KB), filled with the
        model's values; False frees them. Outside stream capture. While on, forward, forward_contacts, step,
        the env step and the resets run env e on its block, the speed test on the model's, and the step VJPs
        raise."""
        self.set_option(abi.OPT_PER_ENV_MODEL, int(bool(on)))

    def set_model_params(self, mask: Optional[torch.Tensor] = None, **fields: Optional[torch.Tensor]):
        """Per-env model parameters (domain randomisation; jax.vmap over a model with batched fields):
        body_mass [nenv, nbody], body_inertia [nenv, nbody, 6], dof_damping / dof_armature [nenv, nv],
        actuator_gear [nenv, nu], pair_friction [nenv, npair] as float32 tensors on the batch's device. A
        field left out (or None) keeps every env's current value; envs with mask <= 0.5 keep their block.
        One launch, capturable; the tensors are read at execution time and no reference to them or to the mask
        is kept here: an eager call is ordered on the current stream like any torch op, but a caller that
        captures the call in a graph keeps the value tensors (and the float32 device mask it passed) alive for
        as long as the graph is replayed, and updates them in place. See include/mjx355.h
        mjl_batch_set_model_params for what follows a replaced field and what stays the model's."""
        unknown = set(fields) - set(abi.MODEL_PARAM)
        if unknown:
            raise MjlError(f"unknown model parameter {sorted(unknown)} (known: {sorted(abi.MODEL_PARAM)})")
        table = (C.c_void_p * abi.NMP)()
        for name, t in fields.items():
            if t is None:
                continue
            dim = self.model_param_dim(name)
            if t.numel() != self.nenv * dim:
                raise MjlError(f"{name} must have {self.nenv} x {dim} elements")
            if t.device != self.device:
                raise MjlError(f"{name} must live on {self.device}")
            table[abi.MODEL_PARAM[name]] = _ptr(t).value
        mk = None if mask is None else mask.to(device=self.device, dtype=torch.float32).contiguous()
        check(lib().mjl_batch_set_model_params(self._h, table, _ptr(mk), _stream()))

    def model_param_dim(self, name: str) -> int:
        return int(lib().mjl_model_param_dim(self.model.handle, abi.MODEL_PARAM[name]))

    def get_model_params(self, name: str) -> torch.Tensor:
        """Field `name` of every env's model block, [nenv, dim]: what the kernels will use."""
        out = torch.empty((self.nenv, self.model_param_dim(name)), dtype=torch.float32, device=self.device)
        if out.numel() == 0:
            return out
        check(lib().mjl_batch_get_model_params(self._h, abi.MODEL_PARAM[name], _ptr(out), _stream()))
        return out.view(self.nenv, self.model.nbody, 6) if name == "body_inertia" else out

    def __getattr__(self, name):
        if name in _FIELD_DIM:
            return self.get(name)
        raise AttributeError(name)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib().mjl_batch_destroy(self._h)
                self._h = None
        except Exception:
            pass


def put_model(m: mjcf.CompiledModel) -> Model:
    return Model(m)


def make_data(sys: Model, nenv: int = 1, device: int = 0) -> Data:
    """Fresh batched data: qpos = qpos0, everything else zero (mjx.make_data per env)."""
    return Data(sys, nenv, device)


def forward(sys: Model, d: Data, mask: Optional[torch.Tensor] = None) -> Data:
    check(lib().mjl_forward(d.handle, _ptr(mask), _stream()))
    return d


@dataclass
class Contacts:
    """Data.contact with a leading env axis, plus mj_contactForce's per-contact forces (forward_contacts).
    Contact c of env e is valid for c < min(ncon[e], max_con); the entries past ncon[e] (and every entry of
    an env outside the call's mask) hold geom -1 and zeros. Order: the kernel's emission order, which is
    the order of the contacts' constraint rows."""
    ncon: torch.Tensor         # int32 [nenv], the true count (may exceed max_con)
    geom: torch.Tensor         # int32 [nenv, max_con, 2]: geom1, geom2
    dim: torch.Tensor          # int32 [nenv, max_con]: condim, 1 or 3
    efc_address: torch.Tensor  # int32 [nenv, max_con]: the contact's first constraint row
    dist: torch.Tensor         # [nenv, max_con]
    pos: torch.Tensor          # [nenv, max_con, 3]
    frame: torch.Tensor        # [nenv, max_con, 3, 3]: rows = normal (geom1 -> geom2), tangent 1, tangent 2
    force: torch.Tensor        # [nenv, max_con, 3]: contact-frame force (normal, tangent 1, tangent 2)
    body_force: Optional[torch.Tensor]  # [nenv, nbody, 3]: net world-frame contact force per body, or None

    def force_world(self) -> torch.Tensor:
        """frame^T force [nenv, max_con, 3]: the force on geom2's body in the world frame (geom1's gets
        the opposite)."""
        return torch.einsum("ecij,eci->ecj", self.frame, self.force)


def _iptr(t: torch.Tensor):
    if not t.is_cuda or t.dtype != torch.int32 or not t.is_contiguous():
        raise MjlError("device index buffers must be contiguous int32 CUDA tensors")
    return C.c_void_p(t.data_ptr())


def forward_contacts(sys: Model, d: Data, mask: Optional[torch.Tensor] = None, max_con: Optional[int] = None,
                     body_force: bool = False) -> Contacts:
    """mjx.forward on the envs with mask > 0.5 (None: all), returning that pass's contacts: what the
    reference reads from Data.contact and mj_contactForce after mjx.forward. max_con (None: sys.ncon_max,
    which truncates nothing) is the per-env capacity of the returned arrays; ncon and body_force always
    cover every contact. See include/mjx355.h mjl_forward_contacts."""
    mc = sys.ncon_max if max_con is None else int(max_con)
    if mc < 1:
        raise MjlError("max_con must be >= 1")
    n, dev = d.nenv, d.device
    # with a mask the library leaves masked-out rows untouched: pre-fill them with the sentinel
    def buf(dtype, *shape, fill=0):
        if mask is None:
            return torch.empty(shape, dtype=dtype, device=dev)
        return torch.full(shape, fill, dtype=dtype, device=dev)
    i32, f32 = torch.int32, torch.float32
    c = Contacts(ncon=buf(i32, n), geom=buf(i32, n, mc, 2, fill=-1), dim=buf(i32, n, mc), efc_address=buf(i32, n, mc),
                 dist=buf(f32, n, mc), pos=buf(f32, n, mc, 3), frame=buf(f32, n, mc, 3, 3), force=buf(f32, n, mc, 3),
                 body_force=buf(f32, n, sys.nbody, 3) if body_force else None)
    mk = None if mask is None else mask.to(device=dev, dtype=torch.float32).contiguous()
    check(lib().mjl_forward_contacts(d.handle, _ptr(mk), mc, _iptr(c.ncon), _iptr(c.geom), _iptr(c.dim),
                                     _iptr(c.efc_address), _ptr(c.dist), _ptr(c.pos), _ptr(c.frame), _ptr(c.force),
                                     _ptr(c.body_force), _stream()))
    return c


def sensors(sys: Model, d: Data, mask: Optional[torch.Tensor] = None, stages: Optional[int] = None,
            out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Data.sensordata [nenv, sys.nrsensordata] of the current state: every sensor of the model (IMU, joint,
    frame, force and touch sensors), sensor `name` at `sys.sensor_slice(name)`. stages: a mask of
    abi.SENSOR_STAGE["pos" | "vel" | "acc"] (None: all three). With "acc" the call runs mjx.forward on the envs
    with mask > 0.5 first, and the result is mjx.forward(d).sensordata; without it, it is one launch that reads
    qpos / qvel only (observations after an env step, capturable). Slots of stages left out, and rows of envs
    outside the mask, keep what `out` held (a fresh `out` is zeros). See include/mjx355.h mjl_sensors."""
    st = sum(abi.SENSOR_STAGE.values()) if stages is None else int(stages)
    n = sys.nrsensordata
    if out is None:
        out = torch.zeros((d.nenv, n), dtype=torch.float32, device=d.device)
    elif tuple(out.shape) != (d.nenv, n) or out.device != d.device:
        raise MjlError(f"out must have shape {(d.nenv, n)} on {d.device}")
    mk = None if mask is None else mask.to(device=d.device, dtype=torch.float32).contiguous()
    if n:  # (a model without sensors: nothing to launch, and an empty tensor has no address to pass)
        check(lib().mjl_sensors(d.handle, _ptr(mk), st, _ptr(out), _stream()))
    return out


@dataclass
class BodyData:
    """The body-level half of mjx.Data with a leading env axis (body_data): each field [nenv, nbody, ...] or
    None where it was not asked for. World frame; see include/mjx355.h mjl_body_data for the definitions."""
    xipos: Optional[torch.Tensor] = None           # [nenv, nbody, 3]
    ximat: Optional[torch.Tensor] = None           # [nenv, nbody, 3, 3]
    subtree_com: Optional[torch.Tensor] = None     # [nenv, nbody, 3]
    cinert: Optional[torch.Tensor] = None          # [nenv, nbody, 10]
    cvel: Optional[torch.Tensor] = None            # [nenv, nbody, 6]: angular, linear
    subtree_linvel: Optional[torch.Tensor] = None  # [nenv, nbody, 3]
    subtree_angmom: Optional[torch.Tensor] = None  # [nenv, nbody, 3]
    cfrc_ext: Optional[torch.Tensor] = None        # [nenv, nbody, 6]: torque, force
    cfrc_int: Optional[torch.Tensor] = None        # [nenv, nbody, 6]: torque, force


# mjl_body_data's outputs in argument order, with the trailing shape of each
BODY_FIELDS = {"xipos": (3,), "ximat": (3, 3), "subtree_com": (3,), "cinert": (10,), "cvel": (6,),
               "subtree_linvel": (3,), "subtree_angmom": (3,), "cfrc_ext": (6,), "cfrc_int": (6,)}


def body_data(sys: Model, d: Data, fields=("subtree_com",), mask: Optional[torch.Tensor] = None,
              out: Optional[BodyData] = None) -> BodyData:
    """Body-level fields of the current state: any of xipos, ximat, subtree_com, cinert, cvel, subtree_linvel,
    subtree_angmom, cfrc_ext, cfrc_int (BODY_FIELDS), as MuJoCo / MJX define them. Without a cfrc field the call
    is one launch that reads qpos / qvel only (the call to make after an env step, capturable); with one it runs
    mjx.forward on the envs with mask > 0.5 first and reads that pass's qacc and contacts. Masses and inertias
    are the env's own while per-env model parameters are on. out: a BodyData whose tensors of `fields` are
    written into (rows of envs outside the mask keep their content); fresh tensors are zeros under a mask. See
    include/mjx355.h mjl_body_data."""
    fields = (fields,) if isinstance(fields, str) else tuple(fields)
    unknown = [f for f in fields if f not in BODY_FIELDS]
    if unknown:
        raise MjlError(f"unknown body_data field {unknown} (known: {list(BODY_FIELDS)})")
    if not fields:
        raise MjlError("body_data needs at least one field")
    res = BodyData() if out is None else out
    ptrs = []
    for name, tail in BODY_FIELDS.items():
        if name not in fields:
            ptrs.append(None)
            continue
        shape = (d.nenv, sys.nbody) + tail
        t = getattr(res, name)
        if t is None:
            if out is not None:
                raise MjlError(f"out.{name} is None but {name} was asked for")
            t = (torch.empty if mask is None else torch.zeros)(shape, dtype=torch.float32, device=d.device)
            setattr(res, name, t)
        elif tuple(t.shape) != shape or t.device != d.device:
            raise MjlError(f"out.{name} must have shape {shape} on {d.device}")
        ptrs.append(_ptr(t))
    mk = None if mask is None else mask.to(device=d.device, dtype=torch.float32).contiguous()
    check(lib().mjl_body_data(d.handle, _ptr(mk), *ptrs, _stream()))
    return res


def _body_arg(sys: Model, body, carrying: int = -1) -> int:
    """bodyexclude as the library takes it: an id (-1: none), a body name, or "self" (the carrying body)."""
    if isinstance(body, str):
        if body == "self":
            if carrying < 0:
                raise MjlError('bodyexclude="self" needs a carrying frame (ray_scan)')
            return carrying
        b = sys.m.name2id("body", body)
        if b < 0:
            raise MjlError(f"no body named {body!r}")
        return b
    return int(body)


def _ray_out(d: Data, nray: int, out, masked: bool, hitpos: bool):
    """(dist, geomid, hitpos) to write into: the caller's (entries None: not computed), or fresh ones holding
    the miss values (what rows of envs outside the mask keep)."""
    n, dev = d.nenv, d.device
    if out is None:
        mk = (lambda sh, dt, v: torch.full(sh, v, dtype=dt, device=dev)) if masked else \
             (lambda sh, dt, v: torch.empty(sh, dtype=dt, device=dev))
        out = (mk((n, nray), torch.float32, -1.0), mk((n, nray), torch.int32, -1),
               mk((n, nray, 3), torch.float32, 0.0) if hitpos else None)
    dist, geomid, hp = (tuple(out) + (None,))[:3]
    if dist is None or tuple(dist.shape) != (n, nray):
        raise MjlError(f"dist must have shape {(n, nray)}")
    if geomid is not None and tuple(geomid.shape) != (n, nray):
        raise MjlError(f"geomid must have shape {(n, nray)}")
    if hp is not None and tuple(hp.shape) != (n, nray, 3):
        raise MjlError(f"hitpos must have shape {(n, nray, 3)}")
    return dist, geomid, hp


def ray(sys: Model, d: Data, pnt, vec, flg_static: bool = True, bodyexclude=-1, cutoff: float = 0.0,
        mask: Optional[torch.Tensor] = None, out=None):
    """mjx.ray with a leading env axis: (dist, geomid) [nenv, nray] of rays pnt + t vec (world frame,
    [nenv, nray, 3]; a [3] or [nray, 3] input is broadcast over the envs) against the geoms posed by the batch's
    current qpos: no forward call is needed first. dist is the ray parameter of the nearest surface (metres for
    a unit vec), -1 with geomid -1 for a miss; a ray starting inside a sphere or capsule reports the exit.
    flg_static=False leaves out the geoms of the world body (the floor); bodyexclude (id, name, -1: none) the
    geoms of one body; cutoff > 0 bounds t. Rows of envs with mask <= 0.5 keep what `out` held. out: (dist,
    geomid) to write into, geomid may be None (then it is not computed and None is returned for it). One
    launch, capturable when pnt / vec / out are device tensors of the full shape. See include/mjx355.h mjl_ray."""
    def rays(x, what):
        t = torch.as_tensor(x, dtype=torch.float32).to(d.device)
        if t.dim() == 1:
            t = t.view(1, 1, 3)
        if t.dim() == 2:
            t = t.unsqueeze(0)
        if t.dim() != 3 or t.shape[-1] != 3:
            raise MjlError(f"{what} must be [3], [nray, 3] or [nenv, nray, 3]")
        return t
    p, v = rays(pnt, "pnt"), rays(vec, "vec")
    nray = max(p.shape[1], v.shape[1])
    try:
        p, v = (t.expand(d.nenv, nray, 3).contiguous() for t in (p, v))
    except RuntimeError:
        raise MjlError(f"pnt {tuple(p.shape)} and vec {tuple(v.shape)} do not broadcast to {(d.nenv, nray, 3)}") from None
    dist, geomid, _ = _ray_out(d, nray, out, mask is not None, False)
    mk = None if mask is None else mask.to(device=d.device, dtype=torch.float32).contiguous()
    check(lib().mjl_ray(d.handle, _ptr(mk), nray, _ptr(p), _ptr(v), abi.RAY_STATIC if flg_static else 0,
                        _body_arg(sys, bodyexclude), float(cutoff), _ptr(dist),
                        None if geomid is None else _iptr(geomid), _stream()))
    return dist, geomid


def scan_frame(sys: Model, frame):
    """(objtype, objid, carrying body) of a scan frame: a body or site name (bodies first), or an
    ("xbody" | "site", id) pair."""
    m = sys.m
    if isinstance(frame, str):
        kind = "xbody" if m.name2id("body", frame) >= 0 else "site"
        i = m.name2id("body" if kind == "xbody" else "site", frame)
        if i < 0:
            raise MjlError(f"no body or site named {frame!r}")
    else:
        kind, i = frame[0], int(frame[1])
        if kind not in ("xbody", "site"):
            raise MjlError('frame must be a name or an ("xbody" | "site", id) pair')
    if kind == "xbody":
        return abi.SENSOR_OBJ["xbody"], i, i
    body = int(m.arrays["site_bodyid"][i]) if 0 <= i < m.nsite else -1
    return abi.SENSOR_OBJ["site"], i, body


def ray_scan(sys: Model, d: Data, frame, lpnt, lvec, align: str = "pose", flg_static: bool = True, bodyexclude=-1,
             cutoff: float = 0.0, mask: Optional[torch.Tensor] = None, out=None):
    """A ray pattern carried by a body or site frame (height scanner, lidar fan, rangefinder): (dist, geomid,
    hitpos), [nenv, nray], [nenv, nray] and [nenv, nray, 3] (world). lpnt / lvec [nray, 3] are in the frame and
    shared by the envs (mjx_amd.rays has patterns). align="pose": ray r is p + R lpnt[r], R lvec[r] with the
    frame's rotation R and origin p; align="yaw": R is the rotation about world z by the frame's heading, so a
    grid turns with the body but stays level. bodyexclude="self" leaves out the carrying body's geoms; the
    other arguments are `ray`'s. out: (dist, geomid, hitpos) to write into, the last two may be None. One
    launch, capturable when lpnt / lvec / out are device tensors. See include/mjx355.h mjl_ray_scan."""
    if align not in abi.SCAN_ALIGN:
        raise MjlError(f"align must be one of {sorted(abi.SCAN_ALIGN)}")
    objtype, objid, body = scan_frame(sys, frame)
    lp, lv = (torch.as_tensor(x, dtype=torch.float32).to(d.device).contiguous() for x in (lpnt, lvec))
    if lp.dim() != 2 or lp.shape[1] != 3 or lp.shape != lv.shape:
        raise MjlError("lpnt and lvec must both be [nray, 3]")
    nray = lp.shape[0]
    dist, geomid, hitpos = _ray_out(d, nray, out, mask is not None, True)
    mk = None if mask is None else mask.to(device=d.device, dtype=torch.float32).contiguous()
    check(lib().mjl_ray_scan(d.handle, _ptr(mk), objtype, objid, abi.SCAN_ALIGN[align], nray, _ptr(lp), _ptr(lv),
                             abi.RAY_STATIC if flg_static else 0, _body_arg(sys, bodyexclude, body), float(cutoff),
                             _ptr(dist), None if geomid is None else _iptr(geomid), _ptr(hitpos), _stream()))
    return dist, geomid, hitpos


MAX_DISTANCE_PAIRS = 65535  # mjl_geom_distance's npair


class GeomDistance(NamedTuple):
    dist: torch.Tensor              # [nenv, npair]
    fromto: Optional[torch.Tensor]  # [nenv, npair, 6]
    normal: Optional[torch.Tensor]  # [nenv, npair, 3]
    jac: Optional[torch.Tensor]     # [nenv, npair, nv]


class BodyDistance(NamedTuple):
    dist: torch.Tensor              # [nenv, nquery]
    fromto: torch.Tensor            # [nenv, nquery, 6]
    normal: torch.Tensor            # [nenv, nquery, 3]
    jac: Optional[torch.Tensor]     # [nenv, nquery, nv]
    geom1: torch.Tensor             # [nenv, nquery] int64: the nearest pair's geom of body1
    geom2: torch.Tensor             # [nenv, nquery] and of body2


def _ids(sys: Model, kind: str, x, n: int) -> list:
    """Ids of `x` (an id, a name, or a list of either) of object kind "geom" / "body", checked on the host."""
    ids = []
    for g in _as_list(x):
        if isinstance(g, str):
            i = sys.m.name2id(kind, g)
            if i < 0:
                raise ValueError(f"no {kind} named {g!r}")
        else:
            i = int(g)
        if not 0 <= i < n:
            raise ValueError(f"{kind} id {i} outside 0..{n - 1}")
        ids.append(i)
    return ids


def geom_pairs(sys: Model, geom1, geom2):
    """(ids1, ids2) of geom_distance's pairs: geom1 / geom2 are ids or names, scalars or equal-length lists. Bad
    ids or names, equal geoms and plane - plane pairs raise ValueError."""
    ids1, ids2 = _ids(sys, "geom", geom1, sys.m.ngeom), _ids(sys, "geom", geom2, sys.m.ngeom)
    if len(ids1) != len(ids2):
        raise ValueError(f"geom1 has {len(ids1)} entries and geom2 {len(ids2)}")
    if not 1 <= len(ids1) <= MAX_DISTANCE_PAIRS:
        raise ValueError(f"geom_distance takes 1..{MAX_DISTANCE_PAIRS} pairs, not {len(ids1)}")
    gtype = sys.m.arrays["geom_type"]
    for a, b in zip(ids1, ids2):
        if a == b:
            raise ValueError(f"geom {a} is paired with itself")
        if gtype[a] == mjcf.GEOM_PLANE and gtype[b] == mjcf.GEOM_PLANE:
            raise ValueError(f"geoms {a} and {b} are both planes: no distance is defined")
    return ids1, ids2


def collision_pairs(sys: Model):
    """The model's own collision pairs as two geom id lists (the pairs the step tests for contact), so that
    geom_distance(sys, d, *collision_pairs(sys), distmax=...) is the clearance of everything that can collide."""
    A = sys.m.arrays
    return [int(g) for g in A["pair_geom1"]], [int(g) for g in A["pair_geom2"]]


def geom_distance(sys: Model, d: Data, geom1, geom2, distmax: float = math.inf, mask: Optional[torch.Tensor] = None,
                  out=None, with_jac: bool = False, _dev=None) -> GeomDistance:
    """mj_geomDistance with a leading env axis: GeomDistance(dist [nenv, npair], fromto [nenv, npair, 6], normal
    [nenv, npair, 3], jac [nenv, npair, nv] or None) of the pairs (geom1[k], geom2[k]): ids or names, scalars or
    equal-length lists, checked on the host (ValueError). dist is the signed distance of the two surfaces (negative:
    overlap), fromto[..., :3] lies on geom1 and fromto[..., 3:] on geom2, normal points from geom1 to geom2
    (to = from + dist normal), jac = normal' (jacp(to) - jacp(from)) is the gradient: jac @ qvel is the rate of dist.
    A pair further apart than distmax gets dist = distmax and zeros elsewhere. Poses come from the batch's current
    qpos inside the call: no forward is needed first. Rows of envs with mask <= 0.5 keep what `out` held (fresh
    tensors are zeros under a mask). out: (dist, fromto, normal, jac) to write into, any but dist may be None
    (then it is not computed and None comes back for it); without out, jac is computed when with_jac. One launch,
    capturable when out holds device tensors and the pair tables are cached (HumanoidEnv.geom_distance). See
    include/mjx355.h mjl_geom_distance."""
    if _dev is None:
        ids1, ids2 = geom_pairs(sys, geom1, geom2)
        _dev = (torch.tensor(ids1, dtype=torch.int32, device=d.device), torch.tensor(ids2, dtype=torch.int32, device=d.device))
    g1, g2 = _dev
    n = g1.shape[0]
    if not float(distmax) > 0.0:
        raise ValueError(f"distmax must be greater than 0, not {distmax}")
    shapes = ((d.nenv, n), (d.nenv, n, 6), (d.nenv, n, 3), (d.nenv, n, sys.nv))
    if out is None:
        new = torch.zeros if mask is not None else torch.empty
        out = tuple(new(s, dtype=torch.float32, device=d.device) for s in shapes[:4 if with_jac else 3])
    out = (tuple(out) + (None, None, None))[:4]
    if out[0] is None:
        raise MjlError("geom_distance needs dist")
    for t, s, what in zip(out, shapes, GeomDistance._fields):
        if t is not None and (tuple(t.shape) != s or t.device != d.device):
            raise MjlError(f"{what} must have shape {s} on {d.device}")
    mk = None if mask is None else mask.to(device=d.device, dtype=torch.float32).contiguous()
    check(lib().mjl_geom_distance(d.handle, _ptr(mk), n, _iptr(g1), _iptr(g2), float(distmax), *(_ptr(t) for t in out),
                                  _stream()))
    return GeomDistance(*out)


def body_pairs(sys: Model, body1, body2):
    """The geom pairs behind body_distance's queries: (ids1, ids2, index [nquery, L]) with row k of `index` the
    positions in the pair lists of every (geom of body1[k], geom of body2[k]) pair, padded to the longest row by
    repeating its first entry. A body without geoms raises ValueError."""
    b1, b2 = _ids(sys, "body", body1, sys.nbody), _ids(sys, "body", body2, sys.nbody)
    if len(b1) != len(b2) or not b1:
        raise ValueError(f"body1 has {len(b1)} entries and body2 {len(b2)}")
    gb = sys.m.arrays["geom_bodyid"]
    ids1, ids2, rows = [], [], []
    for x, y in zip(b1, b2):
        ga, gc = [g for g in range(sys.m.ngeom) if gb[g] == x], [g for g in range(sys.m.ngeom) if gb[g] == y]
        for b, gs in ((x, ga), (y, gc)):
            if not gs:
                raise ValueError(f"body {b} has no geoms")
        rows.append(list(range(len(ids1), len(ids1) + len(ga) * len(gc))))
        ids1 += [a for a in ga for _ in gc]
        ids2 += [c for _ in ga for c in gc]
    ids1, ids2 = geom_pairs(sys, ids1, ids2)
    L = max(len(r) for r in rows)
    return ids1, ids2, [r + [r[0]] * (L - len(r)) for r in rows]


def body_distance(sys: Model, d: Data, body1, body2, distmax: float = math.inf, mask: Optional[torch.Tensor] = None,
                  with_jac: bool = False, _dev=None) -> BodyDistance:
    """The distance sensors' body form: per query (body1[k], body2[k]) (ids or names, scalars or equal-length
    lists) the smallest geom_distance over all geom pairs of the two bodies, with that pair's fromto, normal and
    jac and its geom ids (the first such pair in (geom1, geom2) order on a tie, so the first pair when every pair
    is beyond distmax). One geom_distance launch over all the pairs plus a torch min / gather. Under a mask the
    rows of the other envs are zeros. A body without geoms raises ValueError."""
    if _dev is None:
        ids1, ids2, index = body_pairs(sys, body1, body2)
        _dev = tuple(torch.tensor(x, dtype=dt, device=d.device)
                     for x, dt in ((ids1, torch.int32), (ids2, torch.int32), (index, torch.int64)))
    g1, g2, index = _dev
    nq, L = index.shape
    r = geom_distance(sys, d, None, None, distmax, mask, None, with_jac, _dev=(g1, g2))
    dist, k = r.dist[:, index].min(dim=2)                 # [nenv, nq]
    win = index.unsqueeze(0).expand(d.nenv, nq, L).gather(2, k.unsqueeze(2)).squeeze(2)  # positions in the pair list
    pick = lambda t: None if t is None else t.gather(1, win.unsqueeze(2).expand(-1, -1, t.shape[2]))
    return BodyDistance(dist, pick(r.fromto), pick(r.normal), pick(r.jac), g1.long()[win], g2.long()[win])


MAX_JAC_POINTS = 256  # mjl_jac's npoint


def _as_list(x) -> list:
    return list(x) if isinstance(x, (list, tuple)) else [x]


def _jac_bodies(sys: Model, body) -> list:
    """Body ids of `body` (an id, a name, or a list of either), checked against the model on the host."""
    ids = []
    for b in _as_list(body):
        if isinstance(b, str):
            i = sys.m.name2id("body", b)
            if i < 0:
                raise ValueError(f"no body named {b!r}")
        else:
            i = int(b)
        if not 0 <= i < sys.nbody:
            raise ValueError(f"body id {i} outside 0..{sys.nbody - 1}")
        ids.append(i)
    if not 1 <= len(ids) <= MAX_JAC_POINTS:
        raise ValueError(f"jac takes 1..{MAX_JAC_POINTS} points, not {len(ids)}")
    return ids


def jac_frames(sys: Model, frame, offset=None):
    """(body ids, local offsets [npoint, 3] float32 numpy) of jac_local's frames: a body or site as scan_frame
    resolves it (a name, bodies first, or an ("xbody" | "site", id) pair), or a list of them; a site is its
    body at site_pos. offset ([3] or [npoint, 3], in the body's frame, or the site's for a site) is added."""
    import numpy as np
    single = isinstance(frame, str) or (isinstance(frame, tuple) and len(frame) == 2 and isinstance(frame[0], str)
                                        and frame[0] in ("xbody", "site") and not isinstance(frame[1], str))
    frames = [frame] if single else list(frame)
    if not 1 <= len(frames) <= MAX_JAC_POINTS:
        raise ValueError(f"jac_local takes 1..{MAX_JAC_POINTS} frames, not {len(frames)}")
    off = np.zeros((len(frames), 3)) if offset is None else np.broadcast_to(
        np.asarray(offset.cpu() if torch.is_tensor(offset) else offset, np.float64), (len(frames), 3))
    bodies, local = [], np.zeros((len(frames), 3))
    for k, f in enumerate(frames):
        objtype, i, body = scan_frame(sys, f)
        if objtype == abi.SENSOR_OBJ["site"]:
            if not 0 <= i < sys.m.nsite:
                raise ValueError(f"site id {i} outside 0..{sys.m.nsite - 1}")
            local[k] = np.asarray(sys.m.arrays["site_pos"][i]) + np.asarray(mjcf.quat2mat(np.asarray(sys.m.arrays["site_quat"][i], np.float64))).reshape(3, 3) @ off[k]
        else:
            local[k] = off[k]
        if not 0 <= body < sys.nbody:
            raise ValueError(f"body id {body} outside 0..{sys.nbody - 1}")
        bodies.append(body)
    return bodies, np.float32(local)


def _jac_out(d: Data, npoint: int, nv: int, out, masked: bool, with_xpnt: bool):
    shapes = ((d.nenv, npoint, 3, nv), (d.nenv, npoint, 3, nv), (d.nenv, npoint, 3))
    if out is None:
        new = torch.zeros if masked else torch.empty
        out = tuple(new(s, dtype=torch.float32, device=d.device) for s in shapes[:3 if with_xpnt else 2])
    out = (tuple(out) + (None, None, None))[:3]
    if out[0] is None and out[1] is None:
        raise MjlError("jac needs jacp or jacr")
    for t, s, what in zip(out, shapes, ("jacp", "jacr", "xpnt")):
        if t is not None and (tuple(t.shape) != s or t.device != d.device):
            raise MjlError(f"{what} must have shape {s} on {d.device}")
    return out


def jac(sys: Model, d: Data, point, body, mask: Optional[torch.Tensor] = None, out=None):
    """mjx's support.jac / mj_jac with a leading env axis: (jacp, jacr), [nenv, npoint, 3, nv] each, of the world
    points `point` [nenv, npoint, 3] ([nenv, 3] with one body) carried by `body` (an id, a name, or a list of
    npoint of either; checked on the host, ValueError). jacp qvel is the point's world velocity, jacr qvel the
    body's angular velocity. Poses come from the batch's current qpos inside the call: no forward is needed first.
    Rows of envs with mask <= 0.5 keep what `out` held (fresh tensors are zeros under a mask). out: (jacp, jacr)
    to write into, either may be None (then it is not computed and None comes back for it). One launch,
    capturable when point and out are device tensors. See include/mjx355.h mjl_jac."""
    ids = _jac_bodies(sys, body)
    p = torch.as_tensor(point, dtype=torch.float32).to(d.device)
    if p.dim() == 2:
        p = p.unsqueeze(1)
    if tuple(p.shape) != (d.nenv, len(ids), 3):
        raise MjlError(f"point must have shape {(d.nenv, len(ids), 3)}")
    jp, jr, _ = _jac_out(d, len(ids), sys.nv, out, mask is not None, False)
    mk = None if mask is None else mask.to(device=d.device, dtype=torch.float32).contiguous()
    bt = torch.tensor(ids, dtype=torch.int32, device=d.device)
    check(lib().mjl_jac(d.handle, _ptr(mk), len(ids), _iptr(bt), abi.JAC_FRAME["world"], _ptr(p.contiguous()),
                        _ptr(jp), _ptr(jr), None, _stream()))
    return jp, jr


def jac_local(sys: Model, d: Data, frame, offset=None, mask: Optional[torch.Tensor] = None, out=None, _dev=None):
    """Jacobians of points fixed in body or site frames: (jacp, jacr, xpnt), [nenv, npoint, 3, nv] twice and the
    world points [nenv, npoint, 3]. frame: a body or site (a name, bodies first, or an ("xbody" | "site", id)
    pair, as ray_scan's frame) or a list of npoint of them; offset ([3] or [npoint, 3], in that frame) moves the
    point off the frame's origin. The other arguments are `jac`'s; out: (jacp, jacr, xpnt), any may be None but
    not both Jacobians. One launch. See include/mjx355.h mjl_jac (MJL_JAC_LOCAL)."""
    if _dev is None:
        bodies, local = jac_frames(sys, frame, offset)
        _dev = (torch.tensor(bodies, dtype=torch.int32, device=d.device), torch.tensor(local, device=d.device))
    bt, lt = _dev
    n = bt.shape[0]
    jp, jr, xp = _jac_out(d, n, sys.nv, out, mask is not None, True)
    mk = None if mask is None else mask.to(device=d.device, dtype=torch.float32).contiguous()
    check(lib().mjl_jac(d.handle, _ptr(mk), n, _iptr(bt), abi.JAC_FRAME["local"], _ptr(lt), _ptr(jp), _ptr(jr),
                        _ptr(xp), _stream()))
    return jp, jr, xp


def _jac_dot_out(d: Data, npoint: int, nv: int, out, masked: bool):
    shapes = ((d.nenv, npoint, 3, nv), (d.nenv, npoint, 3, nv), (d.nenv, npoint, 6))
    if out is None:
        new = torch.zeros if masked else torch.empty
        out = tuple(new(s, dtype=torch.float32, device=d.device) for s in shapes)
    out = (tuple(out) + (None, None, None))[:3]
    if all(t is None for t in out):
        raise MjlError("jac_dot needs jacp_dot, jacr_dot or jdotv")
    for t, s, what in zip(out, shapes, ("jacp_dot", "jacr_dot", "jdotv")):
        if t is not None and (tuple(t.shape) != s or t.device != d.device):
            raise MjlError(f"{what} must have shape {s} on {d.device}")
    return out


def jac_dot(sys: Model, d: Data, point, body, mask: Optional[torch.Tensor] = None, out=None):
    """mj_jacDot with a leading env axis: (jacp_dot, jacr_dot, jdotv), the time derivatives [nenv, npoint, 3, nv]
    of `jac`'s Jacobians along the batch's current qvel, and jdotv [nenv, npoint, 6] = (jacp_dot qvel ; jacr_dot
    qvel), the velocity-product term of the task acceleration J qacc + Jdot qvel. point / body / mask as `jac`;
    a world point is attached to its body at this instant. out: (jacp_dot, jacr_dot, jdotv) to write into, any may
    be None but not all (then it is not computed and None comes back for it): (None, None, jdotv) is the cheap
    call. With qvel = 0 everything is exactly zero. One launch, capturable when point and out are device
    tensors. See include/mjx355.h mjl_jac_dot."""
    ids = _jac_bodies(sys, body)
    p = torch.as_tensor(point, dtype=torch.float32).to(d.device)
    if p.dim() == 2:
        p = p.unsqueeze(1)
    if tuple(p.shape) != (d.nenv, len(ids), 3):
        raise MjlError(f"point must have shape {(d.nenv, len(ids), 3)}")
    jp, jr, jv = _jac_dot_out(d, len(ids), sys.nv, out, mask is not None)
    mk = None if mask is None else mask.to(device=d.device, dtype=torch.float32).contiguous()
    bt = torch.tensor(ids, dtype=torch.int32, device=d.device)
    check(lib().mjl_jac_dot(d.handle, _ptr(mk), len(ids), _iptr(bt), abi.JAC_FRAME["world"], _ptr(p.contiguous()),
                            _ptr(jp), _ptr(jr), _ptr(jv), _stream()))
    return jp, jr, jv


def jac_dot_local(sys: Model, d: Data, frame, offset=None, mask: Optional[torch.Tensor] = None, out=None, _dev=None):
    """`jac_dot` of points fixed in body or site frames: (jacp_dot, jacr_dot, jdotv) of `jac_local`'s points
    (frame / offset as there). One launch. See include/mjx355.h mjl_jac_dot (MJL_JAC_LOCAL)."""
    if _dev is None:
        bodies, local = jac_frames(sys, frame, offset)
        _dev = (torch.tensor(bodies, dtype=torch.int32, device=d.device), torch.tensor(local, device=d.device))
    bt, lt = _dev
    n = bt.shape[0]
    jp, jr, jv = _jac_dot_out(d, n, sys.nv, out, mask is not None)
    mk = None if mask is None else mask.to(device=d.device, dtype=torch.float32).contiguous()
    check(lib().mjl_jac_dot(d.handle, _ptr(mk), n, _iptr(bt), abi.JAC_FRAME["local"], _ptr(lt), _ptr(jp), _ptr(jr),
                            _ptr(jv), _stream()))
    return jp, jr, jv


MAX_SUBTREES = 32  # mjl_centroidal's nsub


def _subtree_roots(sys: Model, body) -> list:
    """Body ids of the subtree roots `body` (an id, a name, or a list of either; 0: the whole model)."""
    ids = []
    for b in _as_list(body):
        if isinstance(b, str):
            i = sys.m.name2id("body", b)
            if i < 0:
                raise ValueError(f"no body named {b!r}")
        else:
            i = int(b)
        if not 0 <= i < sys.nbody:
            raise ValueError(f"body id {i} outside 0..{sys.nbody - 1}")
        ids.append(i)
    if not 1 <= len(ids) <= MAX_SUBTREES:
        raise ValueError(f"centroidal takes 1..{MAX_SUBTREES} subtrees, not {len(ids)}")
    return ids


def centroidal(sys: Model, d: Data, body=0, mask: Optional[torch.Tensor] = None, out=None, _dev=None):
    """The centroidal quantities of the subtrees rooted at `body` (an id, a name, or a list of up to 32 of
    either; 0: the whole model): (jac_com, angmom_mat, bias). jac_com [nenv, nsub, 3, nv] is mj_jacSubtreeCom
    (jac_com qvel = subtree_linvel), angmom_mat [nenv, nsub, 3, nv] mj_angmomMat, the angular momentum about the
    subtree's own centre of mass (angmom_mat qvel = subtree_angmom), and bias [nenv, nsub, 6] their derivatives
    applied to qvel: the centre of mass's acceleration and the angular momentum's rate at qacc = 0. Masses and
    inertias are the env's own while per-env model parameters are on. out: (jac_com, angmom_mat, bias) to write
    into, any may be None but not all (then it is not computed and None comes back for it). Rows of envs with
    mask <= 0.5 keep what `out` held (fresh tensors are zeros under a mask). Nothing of `d` is written. One
    launch, capturable when out holds device tensors. See include/mjx355.h mjl_centroidal."""
    if _dev is None:
        _dev = torch.tensor(_subtree_roots(sys, body), dtype=torch.int32, device=d.device)
    n = _dev.shape[0]
    shapes = ((d.nenv, n, 3, sys.nv), (d.nenv, n, 3, sys.nv), (d.nenv, n, 6))
    if out is None:
        new = torch.empty if mask is None else torch.zeros
        out = tuple(new(s, dtype=torch.float32, device=d.device) for s in shapes)
    out = (tuple(out) + (None, None, None))[:3]
    if all(t is None for t in out):
        raise MjlError("centroidal needs jac_com, angmom_mat or bias")
    for t, s, what in zip(out, shapes, ("jac_com", "angmom_mat", "bias")):
        if t is not None and (tuple(t.shape) != s or t.device != d.device):
            raise MjlError(f"{what} must have shape {s} on {d.device}")
    mk = None if mask is None else mask.to(device=d.device, dtype=torch.float32).contiguous()
    check(lib().mjl_centroidal(d.handle, _ptr(mk), n, _iptr(_dev), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _stream()))
    return out


def _centroidal_one(sys: Model, d: Data, body, mask, out, which: int):
    n = len(_subtree_roots(sys, body))
    shape = (d.nenv, n, 3, sys.nv)
    if out is None:
        out = (torch.empty if mask is None else torch.zeros)(shape, dtype=torch.float32, device=d.device)
    outs = [None, None, None]
    outs[which] = out
    return centroidal(sys, d, body, mask, tuple(outs))[which]


def jac_subtree_com(sys: Model, d: Data, body=0, mask: Optional[torch.Tensor] = None,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mj_jacSubtreeCom with a leading env axis: [nenv, nsub, 3, nv], the Jacobian of the centre of mass of the
    subtrees rooted at `body` (`centroidal`'s first output alone). mask / out as there."""
    return _centroidal_one(sys, d, body, mask, out, 0)


def angmom_mat(sys: Model, d: Data, body=0, mask: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mj_angmomMat with a leading env axis: [nenv, nsub, 3, nv], the angular-momentum matrix of the subtrees
    rooted at `body` about their own centres of mass (`centroidal`'s second output alone). mask / out as there."""
    return _centroidal_one(sys, d, body, mask, out, 1)


def _mass_matrix(sys: Model, d: Data, mask, full, vec, mul, solve):
    mk = None if mask is None else mask.to(device=d.device, dtype=torch.float32).contiguous()
    nvec = 0 if vec is None else vec.shape[1]
    check(lib().mjl_mass_matrix(d.handle, _ptr(mk), _ptr(full), nvec, _ptr(vec), _ptr(mul), _ptr(solve), _stream()))


def _vec_arg(sys: Model, d: Data, vec, out, masked: bool):
    """(vec as [nenv, nvec, nv], the result tensor viewed the same way, the result in the caller's shape)"""
    v = torch.as_tensor(vec, dtype=torch.float32).to(d.device)
    if v.dim() not in (2, 3) or v.shape[0] != d.nenv or v.shape[-1] != sys.nv:
        raise MjlError(f"vec must be [{d.nenv}, {sys.nv}] or [{d.nenv}, nvec, {sys.nv}]")
    v3 = v.reshape(d.nenv, -1, sys.nv).contiguous()
    if not 1 <= v3.shape[1] <= 64:
        raise MjlError(f"nvec must be in 1..64, not {v3.shape[1]}")
    if out is None:
        out = (torch.zeros if masked else torch.empty)(tuple(v.shape), dtype=torch.float32, device=d.device)
    elif tuple(out.shape) != tuple(v.shape) or out.device != d.device:
        raise MjlError(f"out must have shape {tuple(v.shape)} on {d.device}")
    _ptr(out)
    return v3, out.view(d.nenv, -1, sys.nv), out


def full_m(sys: Model, d: Data, mask: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mjx's support.full_m with a leading env axis: the dense joint-space inertia [nenv, nv, nv] of the current
    qpos (composite rigid bodies plus dof_armature; the env's own masses, inertias and armatures while per-env
    model parameters are on), symmetric bit for bit. No forward is needed first. Rows of envs with mask <= 0.5
    keep what `out` held (a fresh tensor is zeros under a mask). One launch, capturable. See include/mjx355.h
    mjl_mass_matrix."""
    shape = (d.nenv, sys.nv, sys.nv)
    if out is None:
        out = (torch.empty if mask is None else torch.zeros)(shape, dtype=torch.float32, device=d.device)
    elif tuple(out.shape) != shape or out.device != d.device:
        raise MjlError(f"out must have shape {shape} on {d.device}")
    _mass_matrix(sys, d, mask, out, None, None, None)
    return out


def mul_m(sys: Model, d: Data, vec, mask: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mjx's support.mul_m: M vec of the current qpos, vec [nenv, nv] or [nenv, nvec, nv] (nvec <= 64), the result
    in the same shape. mask / out as full_m. One launch (M is built in the kernel and not stored)."""
    v3, o3, res = _vec_arg(sys, d, vec, out, mask is not None)
    _mass_matrix(sys, d, mask, None, v3, o3, None)
    return res


def solve_m(sys: Model, d: Data, vec, mask: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mjx's smooth.solve_m: M^-1 vec of the current qpos by a Cholesky factor computed in the kernel, vec
    [nenv, nv] or [nenv, nvec, nv] (nvec <= 64), the result in the same shape. mask / out as full_m. One launch."""
    v3, o3, res = _vec_arg(sys, d, vec, out, mask is not None)
    _mass_matrix(sys, d, mask, None, v3, None, o3)
    return res


def inverse(sys: Model, d: Data, qacc=None, discrete: bool = False, mask: Optional[torch.Tensor] = None, out=None,
            with_constraint: bool = False):
    """mjx.inverse with a leading env axis: qfrc_inverse [nenv, nv], the generalized force that gives the current
    qpos / qvel the acceleration `qacc` ([nenv, nv]; None: the stored qacc of the last forward), limits and
    contacts included: M a + qfrc_bias - qfrc_passive - qfrc_constraint with the constraint force evaluated at a,
    no solver. discrete: `qacc` is a step's (qvel' - qvel) / timestep and is first mapped back through the
    integrator's damping solve. with_constraint: (qfrc_inverse, qfrc_constraint) come back. out: the tensor, or
    with_constraint the pair of tensors, to write into. ctrl and applied forces take no part (the result is their
    total); per-env model parameters do. Rows of envs with mask <= 0.5 keep what `out` held (a fresh tensor is
    zeros under a mask). Nothing of `d` is written. One launch, capturable. See include/mjx355.h mjl_inverse."""
    shape = (d.nenv, sys.nv)
    if qacc is not None:
        qacc = torch.as_tensor(qacc, dtype=torch.float32).to(d.device).contiguous()
        if tuple(qacc.shape) != shape:
            raise MjlError(f"qacc must have shape {shape}")
    outs = list(out) if isinstance(out, (tuple, list)) else [out, None]
    if len(outs) != 2 or (outs[1] is not None and not with_constraint):
        raise MjlError("out is one tensor, or (qfrc_inverse, qfrc_constraint) with with_constraint")
    for i in range(2 if with_constraint else 1):
        if outs[i] is None:
            outs[i] = (torch.empty if mask is None else torch.zeros)(shape, dtype=torch.float32, device=d.device)
        elif tuple(outs[i].shape) != shape or outs[i].device != d.device:
            raise MjlError(f"out must have shape {shape} on {d.device}")
    mk = None if mask is None else mask.to(device=d.device, dtype=torch.float32).contiguous()
    flags = abi.INV_DISCRETE if discrete else 0
    check(lib().mjl_inverse(d.handle, _ptr(mk), _ptr(qacc), flags, _ptr(outs[0]), _ptr(outs[1]), _stream()))
    return (outs[0], outs[1]) if with_constraint else outs[0]


def step(sys: Model, d: Data, ctrl: Optional[torch.Tensor] = None, nstep: int = 1) -> Data:
    """mjx.step, `nstep` times in one call (mjl_step_n): the same ctrl (None: the stored one) holds for every
    substep, and the state and derived fields are those `nstep` single steps leave. Not differentiated."""
    if not 1 <= int(nstep) <= abi.MAXSUBSTEP:
        raise MjlError(f"nstep must be in 1..{abi.MAXSUBSTEP}, not {nstep}")
    if ctrl is not None:
        ctrl = ctrl.to(device=d.device, dtype=torch.float32).contiguous()
        if ctrl.shape != (d.nenv, sys.nu):
            raise MjlError(f"ctrl must have shape {(d.nenv, sys.nu)}")
    check(lib().mjl_step_n(d.handle, _ptr(ctrl), int(nstep), _stream()))
    return d


def speedtest_step(sys: Model, d: Data, vel: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mjx_humanoid_speed_test.py:48-57 step(vel): fresh data, qvel[0]=vel, one step -> qpos[0]."""
    if vel.shape != (d.nenv,):
        raise MjlError("vel must have shape (nenv,)")
    out = torch.empty_like(vel) if out is None else out
    check(lib().mjl_speedtest_step(d.handle, _ptr(vel), _ptr(out), _stream()))
    return out


def step_vjp(sys: Model, d: Data, g_qpos: torch.Tensor, g_qvel: torch.Tensor):
    """Reverse-mode derivative of one mjx.step at the batch's current state (not modified):
    cotangents of (qpos', qvel') -> cotangents of (qpos, qvel, ctrl). See include/mjx355.h."""
    dev = d.device
    gq = g_qpos.to(dev, torch.float32).reshape(d.nenv, sys.nq).contiguous()
    gv = g_qvel.to(dev, torch.float32).reshape(d.nenv, sys.nv).contiguous()
    oq = torch.empty_like(gq)
    ov = torch.empty_like(gv)
    oc = torch.empty((d.nenv, sys.nu), dtype=torch.float32, device=dev)
    check(lib().mjl_step_vjp(d.handle, _ptr(gq), _ptr(gv), _ptr(oq), _ptr(ov), _ptr(oc), _stream()))
    return oq, ov, oc


def _step_jacobian(sys: Model, d: Data, ctrl, mask, out, flags: int, nx: int):
    """mjl_step_jacobian into (A [nenv, nx, nx], B [nenv, nx, nu]); `out` = (A, B), either None to skip it."""
    if ctrl is not None:
        ctrl = torch.as_tensor(ctrl, dtype=torch.float32).to(d.device).contiguous()
        if tuple(ctrl.shape) != (d.nenv, sys.nu):
            raise MjlError(f"ctrl must have shape {(d.nenv, sys.nu)}")
    shapes = ((d.nenv, nx, nx), (d.nenv, nx, sys.nu))
    if out is None:
        outs = [(torch.empty if mask is None else torch.zeros)(s, dtype=torch.float32, device=d.device) for s in shapes]
    else:
        outs = list(out) if isinstance(out, (tuple, list)) else None
        if outs is None or len(outs) != 2 or (outs[0] is None and outs[1] is None):
            raise MjlError("out is (A, B), at most one of them None")
        for o, s, what in zip(outs, shapes, "AB"):
            if o is not None and (tuple(o.shape) != s or o.device != d.device or o.dtype != torch.float32):
                raise MjlError(f"out {what} must be float32 of shape {s} on {d.device}")
    mk = None if mask is None else mask.to(device=d.device, dtype=torch.float32).contiguous()
    check(lib().mjl_step_jacobian(d.handle, _ptr(mk), _ptr(ctrl), flags, _ptr(outs[0]), _ptr(outs[1]), _stream()))
    return outs[0], outs[1]


def transition(sys: Model, d: Data, ctrl=None, mask: Optional[torch.Tensor] = None, out=None):
    """mjd_transitionFD's matrices of one mjx.step at the batch's current state, exact rather than by finite
    differences: (A [nenv, 2nv, 2nv], B [nenv, 2nv, nu]) with the state x = (dq, qvel) in the tangent space (a free
    joint's rotation as a body-frame rotation vector, mj_integratePos / mj_differentiatePos). ctrl [nenv, nu]:
    where to linearise (None: the stored ctrl). out = (A, B) to write into; one of them may be None, and is then
    neither computed nor returned (None comes back in its place). The constraint solve is differentiated at its
    converged active set, as step_vjp does by default. Rows of envs with mask <= 0.5 keep what `out` held (fresh
    tensors are zeros under a mask). Nothing of `d` is written. One launch; the first call allocates scratch, so it
    happens outside graph capture. See include/mjx355.h mjl_step_jacobian (MJL_JAC_TANGENT)."""
    return _step_jacobian(sys, d, ctrl, mask, out, abi.JAC_TANGENT, 2 * sys.nv)


def step_jacobian(sys: Model, d: Data, ctrl=None, mask: Optional[torch.Tensor] = None, out=None) -> torch.Tensor:
    """jax.jacobian(mjx.step) in raw coordinates: J [nenv, nq+nv, nq+nv+nu], rows (qpos', qvel'), columns (qpos,
    qvel, ctrl), the oracle's Oracle.step_jacobian per env. out: a tensor of that shape to write into. ctrl and
    mask as transition(). Assembled from mjl_step_jacobian's two raw outputs (one launch and one copy each)."""
    nx, shape = sys.nq + sys.nv, (d.nenv, sys.nq + sys.nv, sys.nq + sys.nv + sys.nu)
    if out is not None and (tuple(out.shape) != shape or out.device != d.device or out.dtype != torch.float32):
        raise MjlError(f"out must be float32 of shape {shape} on {d.device}")
    A, B = _step_jacobian(sys, d, ctrl, mask, None, 0, nx)
    if out is None:
        return torch.cat([A, B], dim=2)
    if mask is None:
        out[:, :, :nx], out[:, :, nx:] = A, B
    else:
        keep = (mask.to(device=d.device, dtype=torch.float32) > 0.5).view(-1, 1, 1)
        out.copy_(torch.where(keep, torch.cat([A, B], dim=2), out))
    return out


MAX_IK_TASKS = 32  # mjl_ik's ntask


class IKResult(NamedTuple):
    """What `ik` returns: the solution, the residual there and the iterations taken."""
    qpos: torch.Tensor             # [nenv, nq]
    err: Optional[torch.Tensor]    # [nenv, ntask, 6]: (e_p ; e_r), world frame, unweighted
    niter: Optional[torch.Tensor]  # [nenv] int32


def ik_dofmask(sys: Model, dofs) -> int:
    """mjl_ik's dofmask of `dofs`: None (every dof), a bool list over nv, a list of dof indices, or joint names (a
    free joint stands for its six dofs)."""
    nv = sys.nv
    if dofs is None:
        return (1 << 32) - 1
    dofs = dofs.tolist() if hasattr(dofs, "tolist") else list(dofs)
    if len(dofs) == nv and all(isinstance(x, bool) for x in dofs):
        return sum(1 << i for i, x in enumerate(dofs) if x)
    mask = 0
    for x in dofs:
        if isinstance(x, str):
            j = sys.m.name2id("joint", x)
            if j < 0:
                raise ValueError(f"no joint named {x!r}")
            a = int(sys.m.arrays["jnt_dofadr"][j])
            ids = range(a, a + (6 if sys.m.arrays["jnt_type"][j] == mjcf.JNT_FREE else 1))
        else:
            if isinstance(x, bool):
                raise ValueError(f"a bool list over the dofs has {nv} entries, not {len(dofs)}")
            ids = [int(x)]
        for i in ids:
            if not 0 <= i < nv:
                raise ValueError(f"dof {i} outside 0..{nv - 1}")
            mask |= 1 << i
    return mask


def ik_tables(sys: Model, frame, offset=None, weight=None):
    """Host tables of ik's tasks: (body ids, body-frame offsets [ntask, 3] float32, conj(site_quat) [ntask, 4] float32
    or None when every frame is a body, weights [ntask, 2] float32 or None). frame / offset as jac_local's."""
    import numpy as np
    bodies, local = jac_frames(sys, frame, offset)
    if len(bodies) > MAX_IK_TASKS:
        raise ValueError(f"ik takes 1..{MAX_IK_TASKS} tasks, not {len(bodies)}")
    single = isinstance(frame, str) or (isinstance(frame, tuple) and len(frame) == 2 and isinstance(frame[0], str)
                                        and frame[0] in ("xbody", "site") and not isinstance(frame[1], str))
    conj, any_site = np.tile(np.float32([1, 0, 0, 0]), (len(bodies), 1)), False
    for k, f in enumerate([frame] if single else list(frame)):
        objtype, i, _ = scan_frame(sys, f)
        if objtype == abi.SENSOR_OBJ["site"]:
            q = np.asarray(sys.m.arrays["site_quat"][i], np.float64)
            conj[k] = np.float32([q[0], -q[1], -q[2], -q[3]] / np.linalg.norm(q))
            any_site = True
    w = None
    if weight is not None:
        w = np.float32(np.broadcast_to(np.asarray(weight.cpu() if torch.is_tensor(weight) else weight, np.float64),
                                       (len(bodies), 2)))
        if not (w >= 0).all():
            raise ValueError("ik weights must be >= 0")
    return bodies, local, conj if any_site else None, w


def _qmul_t(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    aw, ax, ay, az = a.unbind(-1)
    bw, bx, by, bz = b.unbind(-1)
    return torch.stack((aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw), -1)


def ik(sys: Model, d: Data, frame, target_pos=None, target_quat=None, offset=None, weight=None, qpos_start=None,
       qpos_ref=None, dofs=None, iterations: int = 20, damping: float = 1e-3, posture: float = 0.0,
       max_step: float = 0.0, tol: float = 0.0, limits: bool = True, mask: Optional[torch.Tensor] = None, out=None,
       _dev=None) -> IKResult:
    """Batched inverse kinematics: per env a qpos that brings the frames (bodies or sites: names or ("xbody" | "site",
    id) pairs, as jac_local's, with `offset` in the frame) to the world targets target_pos [nenv, ntask, 3] and / or
    target_quat [nenv, ntask, 4] (the frame's own orientation; [nenv, 3] / [nenv, 4] with one frame). A damped
    Gauss-Newton iteration, dq = (J'W'WJ + (damping + posture) I)^-1 (J'W'W e + posture (qpos_ref - q)), run
    `iterations` times, or until every weighted residual is below tol > 0, inside one launch. weight [ntask, 2]:
    (w_pos, w_rot) per task; qpos_start: None = the batch's current qpos; qpos_ref: None = qpos0; dofs: the dofs that
    may move (see ik_dofmask); max_step > 0 bounds max |dq| of an iteration; limits: clamp limited hinges to
    jnt_range. Nothing of `d` is written. Returns IKResult(qpos, err, niter); out: (qpos, err, niter) to write into,
    err and niter may be None. Rows of envs with mask <= 0.5 keep what `out` held (fresh tensors are zeros under a
    mask). Capturable when the targets and out are device tensors. See include/mjx355.h mjl_ik."""
    if _dev is None:
        bodies, local, conj, w = ik_tables(sys, frame, offset, weight)
        dev = d.device
        _dev = (torch.tensor(bodies, dtype=torch.int32, device=dev), torch.tensor(local, device=dev),
                None if conj is None else torch.tensor(conj, device=dev), None if w is None else torch.tensor(w, device=dev))
    bt, lt, cq, wt = _dev
    n = bt.shape[0]

    def arg(t, shape, what):
        if t is None:
            return None
        t = torch.as_tensor(t, dtype=torch.float32).to(d.device)
        if t.dim() == len(shape) - 1 and n == 1 and len(shape) == 3:
            t = t.unsqueeze(1)
        if tuple(t.shape) != shape:
            raise MjlError(f"{what} must have shape {shape}")
        return t.contiguous()
    tp = arg(target_pos, (d.nenv, n, 3), "target_pos")
    tq = arg(target_quat, (d.nenv, n, 4), "target_quat")
    if tp is None and tq is None:
        raise MjlError("ik needs target_pos or target_quat")
    if tq is not None and cq is not None:
        tq = _qmul_t(tq, cq.unsqueeze(0)).contiguous()  # the site's target -> its body's
    qs = arg(qpos_start, (d.nenv, sys.nq), "qpos_start")
    qr = arg(qpos_ref, (d.nenv, sys.nq), "qpos_ref")
    shapes = ((d.nenv, sys.nq), (d.nenv, n, 6), (d.nenv,))
    if out is None:
        new = torch.zeros if mask is not None else torch.empty
        out = (new(shapes[0], dtype=torch.float32, device=d.device), new(shapes[1], dtype=torch.float32, device=d.device),
               new(shapes[2], dtype=torch.int32, device=d.device))
    qo, eo, no = (tuple(out) + (None, None))[:3]
    for t, s, what in zip((qo, eo, no), shapes, ("qpos", "err", "niter")):
        if t is None and what == "qpos":
            raise MjlError("ik needs the qpos output")
        if t is not None and (tuple(t.shape) != s or t.device != d.device):
            raise MjlError(f"{what} must have shape {s} on {d.device}")
    mk = None if mask is None else mask.to(device=d.device, dtype=torch.float32).contiguous()
    dm = ik_dofmask(sys, dofs)
    check(lib().mjl_ik(d.handle, _ptr(mk), n, _iptr(bt), _ptr(lt), _ptr(tp), _ptr(tq), _ptr(wt), _ptr(qs), _ptr(qr),
                       dm - (1 << 32) if dm >= 1 << 31 else dm, int(iterations), float(damping), float(posture),
                       float(max_step), float(tol), abi.IK_LIMITS if limits else 0, _ptr(qo),
                       _ptr(eo), None if no is None else _iptr(no), _stream()))
    return IKResult(qo, eo, no)


MAX_IK_PAIRS = 32  # mjl_ik_wb's npair


class WBIKResult(NamedTuple):
    """What `ik_wb` returns: IKResult's fields, the CoM residual and the pairs' signed distances at the solution."""
    qpos: torch.Tensor                 # [nenv, nq]
    err: Optional[torch.Tensor]        # [nenv, ntask, 6]
    niter: Optional[torch.Tensor]      # [nenv] int32
    com_err: Optional[torch.Tensor]    # [nenv, 3]: com_target - CoM, zeros in dropped rows
    clearance: Optional[torch.Tensor]  # [nenv, npair]: the signed distance of every pair


def ik_wb_tables(sys: Model, com_body=0, com_weight=None, clearance=None, clearance_min=0.0, clearance_weight=None):
    """Host tables of ik_wb's added tasks, checked here (ValueError): (com body id, com weights float32 [3] or None,
    geom ids 1, geom ids 2, clear_min float32 [npair], clear weights float32 [npair] or None). clearance: None or
    (geom1, geom2), ids or names, scalars or equal-length lists, at most 32 pairs; clearance_min / clearance_weight:
    a scalar or one value per pair."""
    import numpy as np
    cb = _subtree_roots(sys, com_body)
    if len(cb) != 1:
        raise ValueError(f"ik_wb takes one com_body, not {len(cb)}")
    cw = None
    if com_weight is not None:
        cw = np.float32(np.broadcast_to(np.asarray(com_weight, np.float64), (3,)))
        if not (np.isfinite(cw).all() and (cw >= 0).all()):
            raise ValueError("com_weight must be finite and >= 0")
    ids1, ids2 = [], []
    if clearance is not None:
        g1, g2 = clearance
        n1, n2 = len(_as_list(g1)), len(_as_list(g2))
        if max(n1, n2) > MAX_IK_PAIRS:
            raise ValueError(f"ik_wb takes at most {MAX_IK_PAIRS} clearance pairs, not {max(n1, n2)}")
        if n1 or n2:
            ids1, ids2 = geom_pairs(sys, g1, g2)
    n = len(ids1)
    cmin = np.float32(np.broadcast_to(np.asarray(clearance_min, np.float64), (n,)))
    if not (np.isfinite(cmin).all() and (cmin >= 0).all()):
        raise ValueError("clearance_min must be finite and >= 0")
    cwt = None
    if clearance_weight is not None:
        cwt = np.float32(np.broadcast_to(np.asarray(clearance_weight, np.float64), (n,)))
        if not (np.isfinite(cwt).all() and (cwt >= 0).all()):
            raise ValueError("clearance_weight must be finite and >= 0")
    return cb[0], cw, ids1, ids2, np.ascontiguousarray(cmin), cwt


def ik_wb(sys: Model, d: Data, frame=None, target_pos=None, target_quat=None, *, com_target=None, com_body=0,
          com_weight=None, clearance=None, clearance_min=0.0, clearance_weight=None, offset=None, weight=None,
          qpos_start=None, qpos_ref=None, dofs=None, iterations: int = 20, damping: float = 1e-3, posture: float = 0.0,
          max_step: float = 0.0, tol: float = 0.0, limits: bool = True, mask: Optional[torch.Tensor] = None, out=None,
          _dev=None) -> WBIKResult:
    """Whole-body inverse kinematics: `ik`'s solve with two more kinds of rows in the same normal equations, still
    one launch. frame / target_pos / target_quat and the keywords from offset on are ik's; frame may be None (no
    frame task) when another task exists.
    com_target [nenv, 3]: brings the centre of mass of the subtree rooted at com_body (an id or a name; 0: the whole
    model) to this world point; com_weight: one weight >= 0 per world axis, (1, 1, 0) holds the CoM above a point
    on the ground and leaves its height free. The env's own masses count while per-env model parameters are on.
    clearance = (geom1, geom2), ids or names as geom_distance's (mjx.collision_pairs(sys) when it has <= 32 pairs):
    every pair whose signed distance at the iterate is below clearance_min (metres; a scalar or one per pair) gets a
    row that pushes the distance up to it, weighted by clearance_weight; a pair at or beyond clearance_min adds
    nothing. A plane - geom pair keeps a foot above the floor. The rows are one-sided penalties of a least-squares
    step, not constraints of a QP: check WBIKResult.clearance.
    Returns WBIKResult(qpos, err, niter, com_err, clearance); out: five tensors to write into, all but qpos may be
    None. Rows of envs with mask <= 0.5 keep what `out` held. Capturable when the targets and out are device
    tensors. See include/mjx355.h mjl_ik_wb."""
    import numpy as np
    dev = d.device
    if _dev is None:
        if frame is None:
            tabs = (None, None, None, None)
        else:
            bodies, local, conj, w = ik_tables(sys, frame, offset, weight)
            tabs = (torch.tensor(bodies, dtype=torch.int32, device=dev), torch.tensor(local, device=dev),
                    None if conj is None else torch.tensor(conj, device=dev), None if w is None else torch.tensor(w, device=dev))
        _dev = (tabs, ik_wb_tables(sys, com_body, com_weight, clearance, clearance_min, clearance_weight))
    (bt, lt, cq, wt), (cb, cw, ids1, ids2, cmin, cwt) = _dev
    n, npair = (0 if bt is None else bt.shape[0]), len(ids1)

    def arg(t, shape, what):
        if t is None:
            return None
        t = torch.as_tensor(t, dtype=torch.float32).to(dev)
        if t.dim() == len(shape) - 1 and n == 1 and len(shape) == 3:
            t = t.unsqueeze(1)
        if tuple(t.shape) != shape:
            raise MjlError(f"{what} must have shape {shape}")
        return t.contiguous()
    tp = arg(target_pos, (d.nenv, n, 3), "target_pos") if n else None
    tq = arg(target_quat, (d.nenv, n, 4), "target_quat") if n else None
    if n and tp is None and tq is None:
        raise MjlError("ik_wb needs target_pos or target_quat for its frames")
    if tq is not None and cq is not None:
        tq = _qmul_t(tq, cq.unsqueeze(0)).contiguous()
    ct = arg(com_target, (d.nenv, 3), "com_target")
    if n == 0 and ct is None and npair == 0:
        raise MjlError("ik_wb needs a frame task, com_target or clearance pairs")
    qs = arg(qpos_start, (d.nenv, sys.nq), "qpos_start")
    qr = arg(qpos_ref, (d.nenv, sys.nq), "qpos_ref")
    shapes = ((d.nenv, sys.nq), (d.nenv, n, 6), (d.nenv,), (d.nenv, 3), (d.nenv, npair))
    if out is None:
        new = torch.zeros if mask is not None else torch.empty
        out = tuple(new(s, dtype=torch.int32 if i == 2 else torch.float32, device=dev) for i, s in enumerate(shapes))
    out = (tuple(out) + (None,) * 4)[:5]
    for t, s, what in zip(out, shapes, WBIKResult._fields):
        if t is None and what == "qpos":
            raise MjlError("ik_wb needs the qpos output")
        if t is not None and (tuple(t.shape) != s or t.device != dev):
            raise MjlError(f"{what} must have shape {s} on {dev}")
    qo, eo, no, co, cl = out
    mk = None if mask is None else mask.to(device=dev, dtype=torch.float32).contiguous()
    dm = ik_dofmask(sys, dofs)
    host = lambda a, t: None if a is None or len(a) == 0 else (t * len(a))(*a)
    check(lib().mjl_ik_wb(d.handle, _ptr(mk), n, None if bt is None else _iptr(bt), _ptr(lt), _ptr(tp), _ptr(tq),
                          _ptr(wt), _ptr(qs), _ptr(qr), dm - (1 << 32) if dm >= 1 << 31 else dm, int(iterations),
                          float(damping), float(posture), float(max_step), float(tol), abi.IK_LIMITS if limits else 0,
                          _ptr(qo), _ptr(eo) if n else None, None if no is None else _iptr(no),
                          cb if ct is not None else -1, _ptr(ct), host(cw, C.c_float), npair, host(ids1, C.c_int32),
                          host(ids2, C.c_int32), host(cmin, C.c_float), host(cwt, C.c_float), _ptr(co),
                          _ptr(cl) if npair else None, _stream()))
    return WBIKResult(qo, eo, no, co, cl)


def step_vjp_full(sys: Model, d: Data, g_qpos: torch.Tensor, g_qvel: torch.Tensor, g_qacc_ws: torch.Tensor):
    """step_vjp with the carried warm start (mjl_step_vjp_full): cotangents of (qpos', qvel',
    qacc_warmstart') -> (qpos, qvel, qacc_warmstart, ctrl)."""
    dev = d.device
    gq = g_qpos.to(dev, torch.float32).reshape(d.nenv, sys.nq).contiguous()
    gv = g_qvel.to(dev, torch.float32).reshape(d.nenv, sys.nv).contiguous()
    gw = g_qacc_ws.to(dev, torch.float32).reshape(d.nenv, sys.nv).contiguous()
    oq, ov, ow = torch.empty_like(gq), torch.empty_like(gv), torch.empty_like(gw)
    oc = torch.empty((d.nenv, sys.nu), dtype=torch.float32, device=dev)
    check(lib().mjl_step_vjp_full(d.handle, _ptr(gq), _ptr(gv), _ptr(gw), _ptr(oq), _ptr(ov), _ptr(ow), _ptr(oc),
                                  _stream()))
    return oq, ov, ow, oc
