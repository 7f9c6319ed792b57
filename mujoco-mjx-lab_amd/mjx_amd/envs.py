"""Batched humanoid walker env on the device (reference src/envs.py, train_ppo.py auto-reset).

The reference builds pure functions `single_reset`/`single_step` and vmaps them
(`create_env_functions`, src/envs.py:26-497); PPO then computes a reset for *every* env on
*every* step and merges it with `where(done, reset, step)` over the whole mjx.Data pytree
(train_ppo.py:149-161). Here one native launch does step + reward + obs and, for the envs that
finished, the reset, in place (`mjl_env_step(auto_reset=1)`); the merged state, obs, reward and
done flags are exactly those of the reference's merge.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import abi
from ._lib import MjlError, check, lib
from .config import EnvConfig
from .mjx import Data, Model, _ptr, _stream, make_data


def obs_size(nq: int, nv: int) -> int:
    """1 (height) + 3 (rpy) + (nq-7) joints + nv velocities + 2 target features (src/envs.py:54-56)."""
    return 1 + 3 + (nq - 7) + nv + 2


def resolve_ids(m, cfg: EnvConfig) -> EnvConfig:
    """Body / sensor id lookup done by reference load_model_and_create_env (training_utils.py:84-89)."""
    cfg.pelvis_body_id = m.name2id("body", "pelvis")
    cfg.head_body_id = m.name2id("body", "head")
    def touch(name):  # the env's touch ids index the touch list, not the model's sensors (the readout table)
        s = m.name2id("sensor", name)
        if s < 0 or "rsensor_type" not in m.arrays:
            return s
        return int(m.arrays["rsensor_objid"][s]) if m.arrays["rsensor_type"][s] == 0 else -1
    cfg.touch_sensor_right_id = touch("touch_foot_right")
    cfg.touch_sensor_left_id = touch("touch_foot_left")
    if min(cfg.pelvis_body_id, cfg.head_body_id, cfg.touch_sensor_right_id, cfg.touch_sensor_left_id) < 0:
        raise MjlError("model lacks pelvis/head bodies or touch_foot_* sensors")
    return cfg


class HumanoidEnv:
    """`num_envs` walker envs resident on one GPU. State lives in `self.data` (native batch)."""

    def __init__(self, sys: Model, cfg: EnvConfig, num_envs: int, device: int = 0, seed: int = 0,
                 store_derived: bool = False, n_frames: int = 1):
        """n_frames: physics steps per step() (Brax's n_frames, Gym's frame_skip), one mjl_env_step_n call:
        the action holds for all of them and reward, observation and termination are evaluated once, after
        the last; `dt` = n_frames * timestep is the control period (the reward's own dt stays the timestep)."""
        if not 1 <= int(n_frames) <= abi.MAXSUBSTEP:
            raise MjlError(f"n_frames must be in 1..{abi.MAXSUBSTEP}, not {n_frames}")
        self.n_frames = int(n_frames)
        self.dt = self.n_frames * float(sys.m.timestep)
        self.sys = sys
        self.cfg = cfg
        self.num_envs = int(num_envs)
        self.obs_dim = obs_size(sys.nq, sys.nv)
        self.act_dim = sys.nu
        self.data: Data = make_data(sys, self.num_envs, device)
        self.data.set_option(abi.OPT_STORE_DERIVED, int(store_derived))
        self._cfg_c = abi.env_config_c(cfg, sys.m, self.obs_dim)
        check(lib().mjl_env_config(self.data.handle, C.byref(self._cfg_c)))
        dev = self.data.device
        self.obs = torch.zeros((self.num_envs, self.obs_dim), dtype=torch.float32, device=dev)
        self.rew = torch.zeros(self.num_envs, dtype=torch.float32, device=dev)
        self.term = torch.zeros(self.num_envs, dtype=torch.float32, device=dev)
        self.trunc = torch.zeros(self.num_envs, dtype=torch.float32, device=dev)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.counter = 0
        # device RNG counter base (0 in eager use): a hipGraph-captured rollout passes counters
        # 1..T and the trainer moves the base before each replay (mjl_batch_set_counter_base)
        self.ctr_base = torch.zeros(1, dtype=torch.int64, device=dev)
        check(lib().mjl_batch_set_counter_base(self.data.handle, C.c_void_p(self.ctr_base.data_ptr())))

    def set_reset_keys(self, keys: Optional[torch.Tensor], mode: int = 1):
        """Draw resets (reset() and the auto-reset of step()) from per-env jax.random keys
        [num_envs, 2] (int32/uint32 bits, device; read at execution time, so update in place), as
        single_reset(key) does (src/envs.py:116-147); None returns to the (seed, counter) stream."""
        if keys is not None:
            if keys.shape != (self.num_envs, 2) or keys.dtype not in (torch.int32, torch.uint32) or not keys.is_cuda \
                    or not keys.is_contiguous():
                raise MjlError("reset keys must be a contiguous [num_envs, 2] int32 CUDA tensor")
        self._keys = keys  # keep the buffer alive while the library points at it
        check(lib().mjl_env_set_reset_keys(self.data.handle, None if keys is None else C.c_void_p(keys.data_ptr()),
                                           int(mode)))

    def attach_applied(self, qfrc_applied: Optional[torch.Tensor] = None,
                       xfrc_applied: Optional[torch.Tensor] = None):
        """Applied forces for step() (Data.attach_applied): read at execution time, never written by a step
        or cleared by a reset; resets and pooled resets run without them. Both None detaches."""
        self.data.attach_applied(qfrc_applied, xfrc_applied)
        self.xfrc_applied = xfrc_applied
        if xfrc_applied is not None and getattr(self, "push_timer", None) is None:  # push()'s per-env timers
            self.push_timer = torch.zeros((self.num_envs, 2), dtype=torch.int32, device=self.obs.device)

    def push(self, body: int, interval: Tuple[int, int], duration: int, force: Tuple[float, float],
             done: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None,
             counter: Optional[int] = None):
        """One step of the random-push schedule, called before step() (mjl_env_push): every `interval`
        (lo, hi) steps, drawn per env, a horizontal force of magnitude in `force` (lo, hi) and uniform
        direction is held on `body` for `duration` steps in the attached xfrc_applied. `done` [num_envs]
        (the previous step's max(term, trunc)) ends an env's push and redraws its interval. The timer tensor
        is the env's. `noise` [num_envs, 3] replaces the on-device draws (tests); `counter` as in step()
        (default: the counter the next step() will use; the push stream is a domain of its own)."""
        if getattr(self, "xfrc_applied", None) is None:
            raise MjlError("push needs attach_applied(xfrc_applied=...) first")
        for t, n, what in ((done, self.num_envs, "done"), (noise, self.num_envs * 3, "noise")):
            if t is not None and t.numel() != n:
                raise MjlError(f"{what} must have {n} elements")
        check(lib().mjl_env_push(self.data.handle, int(body), C.c_void_p(self.push_timer.data_ptr()),
                                 int(interval[0]), int(interval[1]), int(duration), float(force[0]), float(force[1]),
                                 _ptr(done), self.seed, self.counter + 1 if counter is None else int(counter),
                                 _ptr(noise), _stream()))

    def enable_model_params(self, on: bool = True):
        """Per-env model blocks for this env's batch (Data.enable_model_params); outside stream capture."""
        self.data.enable_model_params(on)

    def set_model_params(self, mask: Optional[torch.Tensor] = None, **fields: Optional[torch.Tensor]):
        """Per-env model parameters (Data.set_model_params): step(), its auto-resets, reset() and the pooled
        resets run env e on its own body_mass / body_inertia / dof_damping / dof_armature / actuator_gear /
        pair_friction. Pooled resets are computed with the values at fill_reset_pool()."""
        self.data.set_model_params(mask, **fields)

    def get_model_params(self, name: str) -> torch.Tensor:
        return self.data.get_model_params(name)

    def sensors(self, mask: Optional[torch.Tensor] = None, stages: Optional[int] = None,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Data.sensordata [num_envs, sys.nrsensordata] of the envs' current state (mjx.sensors): after step(),
        with stages = pos | vel, one launch on the post-step state, capturable with the step."""
        from .mjx import sensors
        return sensors(self.sys, self.data, mask, stages, out)

    def body_data(self, fields=("subtree_com",), mask: Optional[torch.Tensor] = None):
        """Body-level fields of the envs' current state (mjx.body_data) in tensors this env owns: allocated
        (zeros) at the first call that asks for a field and written again by every later one, so the same
        BodyData comes back. Without a cfrc field it is one launch on the post-step state that can be captured
        with the step, as sensors()."""
        from .mjx import BODY_FIELDS, BodyData, body_data
        fields = (fields,) if isinstance(fields, str) else tuple(fields)
        bufs = self.__dict__.setdefault("_body_bufs", BodyData())
        for f in fields:
            if f in BODY_FIELDS and getattr(bufs, f) is None:
                setattr(bufs, f, torch.zeros((self.num_envs, self.sys.nbody) + BODY_FIELDS[f], dtype=torch.float32,
                                             device=self.obs.device))
        return body_data(self.sys, self.data, fields, mask, bufs)

    def jac(self, frames, offset=None, mask: Optional[torch.Tensor] = None):
        """Jacobians of points fixed in body or site frames of the envs' current state (mjx.jac_local): (jacp,
        jacr, xpnt) in tensors this env owns. The frames' device tables and the three outputs are allocated
        (zeros) at the first call with these (frames, offset) and written again by every later one, so after one
        eager call it is one launch on the post-step state that can be captured with the step, as sensors()."""
        from .mjx import jac_frames, jac_local
        bodies, local = jac_frames(self.sys, frames, offset)
        key = (tuple(bodies), local.tobytes())
        bufs = self.__dict__.setdefault("_jac_bufs", {})
        if key not in bufs:
            dev, n, p, nv = self.obs.device, self.num_envs, len(bodies), self.sys.nv
            bufs[key] = ((torch.tensor(bodies, dtype=torch.int32, device=dev), torch.tensor(local, device=dev)),
                         (torch.zeros((n, p, 3, nv), device=dev), torch.zeros((n, p, 3, nv), device=dev),
                          torch.zeros((n, p, 3), device=dev)))
        tabs, out = bufs[key]
        return jac_local(self.sys, self.data, frames, offset, mask, out, _dev=tabs)

    def ik(self, frames, target_pos=None, target_quat=None, offset=None, weight=None, qpos_start=None, qpos_ref=None,
           dofs=None, iterations: int = 20, damping: float = 1e-3, posture: float = 0.0, max_step: float = 0.0,
           tol: float = 0.0, limits: bool = True, mask: Optional[torch.Tensor] = None):
        """Inverse kinematics from the envs' current qpos (mjx.ik; qpos_start overrides the start): IKResult(qpos,
        err, niter) in tensors this env owns. The tasks' device tables and the three outputs are allocated (zeros)
        at the first call with these (frames, offset, weight) and written again by every later one; targets given
        as device tensors are read at execution time. After one eager call it is one launch that writes nothing of
        the envs' state and can be captured with the step, as jac()."""
        from .mjx import ik, ik_tables
        bodies, local, conj, w = ik_tables(self.sys, frames, offset, weight)
        key = (tuple(bodies), local.tobytes(), None if conj is None else conj.tobytes(), None if w is None else w.tobytes())
        bufs = self.__dict__.setdefault("_ik_bufs", {})
        if key not in bufs:
            dev, n, p = self.obs.device, self.num_envs, len(bodies)
            bufs[key] = ((torch.tensor(bodies, dtype=torch.int32, device=dev), torch.tensor(local, device=dev),
                          None if conj is None else torch.tensor(conj, device=dev),
                          None if w is None else torch.tensor(w, device=dev)),
                         (torch.zeros((n, self.sys.nq), device=dev), torch.zeros((n, p, 6), device=dev),
                          torch.zeros((n,), dtype=torch.int32, device=dev)))
        tabs, out = bufs[key]
        return ik(self.sys, self.data, frames, target_pos, target_quat, offset, weight, qpos_start, qpos_ref, dofs,
                  iterations, damping, posture, max_step, tol, limits, mask, out, _dev=tabs)

    def ik_wb(self, frames=None, target_pos=None, target_quat=None, *, com_target=None, com_body=0, com_weight=None,
              clearance=None, clearance_min=0.0, clearance_weight=None, offset=None, weight=None, qpos_start=None,
              qpos_ref=None, dofs=None, iterations: int = 20, damping: float = 1e-3, posture: float = 0.0,
              max_step: float = 0.0, tol: float = 0.0, limits: bool = True, mask: Optional[torch.Tensor] = None):
        """Whole-body inverse kinematics from the envs' current qpos (mjx.ik_wb): WBIKResult(qpos, err, niter,
        com_err, clearance) in tensors this env owns, allocated (zeros) with the frame tasks' device tables at the
        first call with these tasks and written again by every later one. The CoM and clearance tables are host
        values that travel in the launch itself; com_target and the frame targets given as device tensors are read
        at execution time. After one eager call it is one launch that writes nothing of the envs' state and can be
        captured with the step, as ik()."""
        from .mjx import ik_tables, ik_wb, ik_wb_tables
        ft = (None, None, None, None) if frames is None else ik_tables(self.sys, frames, offset, weight)
        wb = ik_wb_tables(self.sys, com_body, com_weight, clearance, clearance_min, clearance_weight)
        key = tuple(None if x is None else (x.tobytes() if hasattr(x, "tobytes") else tuple(x)) for x in ft + wb[1:]) + (wb[0],)
        bufs = self.__dict__.setdefault("_ik_wb_bufs", {})
        if key not in bufs:
            dev, n, p = self.obs.device, self.num_envs, 0 if ft[0] is None else len(ft[0])
            tabs = (None if ft[0] is None else torch.tensor(ft[0], dtype=torch.int32, device=dev),) + tuple(
                None if x is None else torch.tensor(x, device=dev) for x in ft[1:])
            bufs[key] = (tabs, (torch.zeros((n, self.sys.nq), device=dev), torch.zeros((n, p, 6), device=dev),
                                torch.zeros((n,), dtype=torch.int32, device=dev), torch.zeros((n, 3), device=dev),
                                torch.zeros((n, len(wb[2])), device=dev)))
        tabs, out = bufs[key]
        return ik_wb(self.sys, self.data, frames, target_pos, target_quat, com_target=com_target, qpos_start=qpos_start,
                     qpos_ref=qpos_ref, dofs=dofs, iterations=iterations, damping=damping, posture=posture,
                     max_step=max_step, tol=tol, limits=limits, mask=mask, out=out, _dev=(tabs, wb))

    def jac_dot(self, frames, offset=None, mask: Optional[torch.Tensor] = None):
        """Time derivatives of jac()'s Jacobians and the velocity-product term (mjx.jac_dot_local): (jacp_dot,
        jacr_dot, jdotv) in tensors this env owns, allocated (zeros) at the first call with these (frames,
        offset) and written again by every later one: after one eager call it is one launch on the post-step
        state that can be captured with the step, as jac()."""
        from .mjx import jac_dot_local, jac_frames
        bodies, local = jac_frames(self.sys, frames, offset)
        key = (tuple(bodies), local.tobytes())
        bufs = self.__dict__.setdefault("_jac_dot_bufs", {})
        if key not in bufs:
            dev, n, p, nv = self.obs.device, self.num_envs, len(bodies), self.sys.nv
            bufs[key] = ((torch.tensor(bodies, dtype=torch.int32, device=dev), torch.tensor(local, device=dev)),
                         (torch.zeros((n, p, 3, nv), device=dev), torch.zeros((n, p, 3, nv), device=dev),
                          torch.zeros((n, p, 6), device=dev)))
        tabs, out = bufs[key]
        return jac_dot_local(self.sys, self.data, frames, offset, mask, out, _dev=tabs)

    def centroidal(self, body=0, mask: Optional[torch.Tensor] = None):
        """Centroidal quantities of the subtrees rooted at `body` (mjx.centroidal; 0: the whole model): (jac_com,
        angmom_mat, bias) in tensors this env owns, allocated (zeros) with the roots' device table at the first
        call with these roots and written again by every later one: one launch on the post-step state,
        capturable with the step."""
        from .mjx import _subtree_roots, centroidal
        roots = tuple(_subtree_roots(self.sys, body))
        bufs = self.__dict__.setdefault("_centroidal_bufs", {})
        if roots not in bufs:
            dev, n, s, nv = self.obs.device, self.num_envs, len(roots), self.sys.nv
            bufs[roots] = (torch.tensor(roots, dtype=torch.int32, device=dev),
                           (torch.zeros((n, s, 3, nv), device=dev), torch.zeros((n, s, 3, nv), device=dev),
                            torch.zeros((n, s, 6), device=dev)))
        tab, out = bufs[roots]
        return centroidal(self.sys, self.data, body, mask, out, _dev=tab)

    def full_m(self, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The joint-space inertia [num_envs, nv, nv] of the envs' current state (mjx.full_m) in a tensor this env
        owns (zeros at first, written again by every call): one launch on the post-step state, capturable with
        the step."""
        from .mjx import full_m
        if getattr(self, "_full_m", None) is None:
            self._full_m = torch.zeros((self.num_envs, self.sys.nv, self.sys.nv), device=self.obs.device)
        return full_m(self.sys, self.data, mask, self._full_m)

    def inverse(self, qacc=None, discrete: bool = False, mask: Optional[torch.Tensor] = None):
        """Inverse dynamics of the envs' current state (mjx.inverse): (qfrc_inverse, qfrc_constraint), each
        [num_envs, nv], in tensors this env owns (zeros at first, written again by every call). qacc None: the
        stored qacc of the last forward; a tensor is read at execution time, so a captured call sees what it
        holds at each replay. One launch that writes nothing of the envs' state, capturable with the step."""
        from .mjx import inverse
        if getattr(self, "_inverse", None) is None:
            self._inverse = (torch.zeros((self.num_envs, self.sys.nv), device=self.obs.device),
                             torch.zeros((self.num_envs, self.sys.nv), device=self.obs.device))
        return inverse(self.sys, self.data, qacc, discrete, mask, self._inverse, with_constraint=True)

    def transition(self, mask: Optional[torch.Tensor] = None):
        """Linearization of the physics step at the envs' current state and stored ctrl (mjx.transition): (A
        [num_envs, 2nv, 2nv], B [num_envs, 2nv, nu]) in tensors this env owns (zeros at first, written again by
        every call). It is mjx.step's derivative: the env's action flip / clip and its reward are not part of it,
        and it covers one physics step, so an env with n_frames != 1 raises. One launch that writes nothing of the
        envs' state; after one eager call (which allocates the scratch) it can be captured with the step."""
        from .mjx import transition
        if self.n_frames != 1:
            raise MjlError(f"transition() linearises one physics step; this env runs n_frames = {self.n_frames}")
        if getattr(self, "_transition", None) is None:
            n, nv, nu, dev = self.num_envs, self.sys.nv, self.sys.nu, self.obs.device
            self._transition = (torch.zeros((n, 2 * nv, 2 * nv), device=dev), torch.zeros((n, 2 * nv, nu), device=dev))
        return transition(self.sys, self.data, None, mask, self._transition)

    def scan(self, frame, pattern, align: str = "pose", flg_static: bool = True, bodyexclude="self",
             cutoff: float = 0.0, mask: Optional[torch.Tensor] = None):
        """Range scan of the envs' current state (mjx.ray_scan): `pattern` = (lpnt, lvec) [nray, 3] in the frame
        of body / site `frame` (mjx_amd.rays.grid_pattern, fan_pattern) -> (dist, geomid, hitpos). The pattern's
        device copy and the three outputs are allocated at the first call with this (frame, align, pattern) and
        written again by every later one (the same tensors come back; rows of envs outside `mask` keep their
        content, -1 / -1 / 0 at first), so after one eager call the scan is one launch on the post-step state
        that can be captured with the step, as sensors()."""
        from .mjx import ray_scan
        lp, lv = (np.ascontiguousarray(np.asarray(x.cpu() if torch.is_tensor(x) else x, np.float32)) for x in pattern)
        key = (str(frame), align, lp.tobytes(), lv.tobytes())
        bufs = self.__dict__.setdefault("_scan_bufs", {})
        if key not in bufs:
            dev, n, r = self.obs.device, self.num_envs, lp.shape[0]
            bufs[key] = (torch.tensor(lp, device=dev), torch.tensor(lv, device=dev),
                         (torch.full((n, r), -1.0, device=dev), torch.full((n, r), -1, dtype=torch.int32, device=dev),
                          torch.zeros((n, r, 3), device=dev)))
        dlp, dlv, out = bufs[key]
        return ray_scan(self.sys, self.data, frame, dlp, dlv, align, flg_static, bodyexclude, cutoff, mask, out)

    def geom_distance(self, geom1, geom2, distmax: float = math.inf, with_jac: bool = False,
                      mask: Optional[torch.Tensor] = None):
        """Signed geom distances of the envs' current state (mjx.geom_distance): GeomDistance(dist, fromto, normal,
        jac) in tensors this env owns. The pairs' device tables and the outputs are allocated (zeros) at the first
        call with this pair list (jac at the first call that asks for it) and written again by every later one, so
        after one eager call it is one launch on the post-step state that can be captured with the step, as jac()."""
        from .mjx import geom_distance, geom_pairs
        ids1, ids2 = geom_pairs(self.sys, geom1, geom2)
        key = (tuple(ids1), tuple(ids2))
        bufs = self.__dict__.setdefault("_distance_bufs", {})
        dev, n, p = self.obs.device, self.num_envs, len(ids1)
        if key not in bufs:
            bufs[key] = [(torch.tensor(ids1, dtype=torch.int32, device=dev), torch.tensor(ids2, dtype=torch.int32, device=dev)),
                         torch.zeros((n, p), device=dev), torch.zeros((n, p, 6), device=dev),
                         torch.zeros((n, p, 3), device=dev), None]
        b = bufs[key]
        if with_jac and b[4] is None:
            b[4] = torch.zeros((n, p, self.sys.nv), device=dev)
        return geom_distance(self.sys, self.data, None, None, distmax, mask, (b[1], b[2], b[3], b[4] if with_jac else None),
                             _dev=b[0])

    def _next_counter(self) -> int:
        self.counter += 1
        return self.counter

    def reset(self, mask: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None,
              counter: Optional[int] = None) -> torch.Tensor:
        """v_reset (src/envs.py:115-202,494) on all envs, or on envs with mask > 0.5.
        `noise` [num_envs, nq-7+nv+2] of uniforms replaces the on-device RNG (parity tests).
        `counter` (graph capture) is the RNG counter relative to `ctr_base`; default: the next one."""
        mk = None if mask is None else mask.to(self.obs.device, torch.float32).contiguous()
        nz = None if noise is None else noise.to(self.obs.device, torch.float32).contiguous()
        check(lib().mjl_env_reset(self.data.handle, _ptr(mk), self.seed,
                                  self._next_counter() if counter is None else int(counter), _ptr(nz),
                                  _ptr(self.obs), _stream()))
        return self.obs

    def enable_reset_pool(self, slots: int = 16):
        """Allocate `slots` pooled resets per env (MJL_OPT_RESET_POOL); outside stream capture."""
        self.data.set_option(abi.OPT_RESET_POOL, int(slots))
        self.pool_slots = int(slots)

    def fill_reset_pool(self, n: torch.Tensor, counter: Optional[int] = None):
        """Compute min(n, slots) resets per env in bulk (mjl_env_fill_reset_pool; n: device int32 [1],
        read at execution time); the next auto-resets of step() merge them in order. `counter`:
        the draw's counter (relative to ctr_base under graph capture); default the current counter,
        which the pool's own counter domain keeps apart from the steps' draws."""
        check(lib().mjl_env_fill_reset_pool(self.data.handle, C.c_void_p(n.data_ptr()), self.seed,
                                            self.counter if counter is None else int(counter), _stream()))

    def step(self, act: torch.Tensor, auto_reset: bool = True,
             out: Optional[Tuple[torch.Tensor, ...]] = None, counter: Optional[int] = None) -> Tuple[torch.Tensor, ...]:
        """v_step (src/envs.py:333-495) fused with merge_if_done (train_ppo.py:147-161).
        Returns (obs, reward, terminated, truncated); obs is post-reset for finished envs.
        `counter` (graph capture) is the RNG counter relative to `ctr_base`; default: the next one."""
        act = act.to(self.obs.device, torch.float32).contiguous()
        if act.shape != (self.num_envs, self.act_dim):
            raise MjlError(f"action must have shape {(self.num_envs, self.act_dim)}")
        obs, rew, term, trunc = out if out is not None else (self.obs, self.rew, self.term, self.trunc)
        check(lib().mjl_env_step_n(self.data.handle, _ptr(act), self.n_frames, _ptr(obs), _ptr(rew), _ptr(term),
                                   _ptr(trunc), int(auto_reset), self.seed,
                                   self._next_counter() if counter is None else int(counter), _stream()))
        return obs, rew, term, trunc

    def step_vjp(self, act: torch.Tensor, g_qpos: torch.Tensor, g_qvel: torch.Tensor, g_rew: torch.Tensor,
                 g_aux: Optional[torch.Tensor] = None, nonfinite: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, ...]:
        """VJP of one env step (src/envs.py:333-492, no reset merge) at the current state and aux:
        cotangents of (qpos', qvel', reward, aux') -> (qpos, qvel, action, aux). State unchanged.
        With `nonfinite` (a device float counter) an env whose cotangents come out non-finite gets
        zero outputs and is counted there."""
        dev, B = self.obs.device, self.num_envs
        f = lambda x, *shape: x.to(dev, torch.float32).reshape(B, *shape).contiguous()  # noqa: E731
        act = f(act, self.act_dim)
        gq, gv, gr = f(g_qpos, self.sys.nq), f(g_qvel, self.sys.nv), f(g_rew)
        ga = torch.zeros((B, abi.AUX_DIM), device=dev) if g_aux is None else f(g_aux, abi.AUX_DIM)
        oq, ov = torch.empty_like(gq), torch.empty_like(gv)
        oa, oaux = torch.empty_like(act), torch.empty_like(ga)
        check(lib().mjl_env_step_vjp_guarded(self.data.handle, _ptr(act), _ptr(gq), _ptr(gv), _ptr(gr), _ptr(ga),
                                             _ptr(oq), _ptr(ov), _ptr(oa), _ptr(oaux), _ptr(nonfinite), _stream()))
        return oq, ov, oa, oaux

    def step_vjp_full(self, act: torch.Tensor, g_qpos: torch.Tensor, g_qvel: torch.Tensor, g_ws: torch.Tensor,
                      g_rew: torch.Tensor, g_aux: Optional[torch.Tensor] = None,
                      nonfinite: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, ...]:
        """step_vjp plus the carried warm start (mjl_env_step_vjp_full): g_ws is the cotangent of the
        output qacc_warmstart; returns (qpos, qvel, qacc_warmstart, action, aux) cotangents. The
        warm-start cotangent is nonzero only with the unrolled VJP (jax.grad through the Data carry)."""
        dev, B = self.obs.device, self.num_envs
        f = lambda x, *shape: x.to(dev, torch.float32).reshape(B, *shape).contiguous()  # noqa: E731
        act = f(act, self.act_dim)
        gq, gv, gw, gr = f(g_qpos, self.sys.nq), f(g_qvel, self.sys.nv), f(g_ws, self.sys.nv), f(g_rew)
        ga = torch.zeros((B, abi.AUX_DIM), device=dev) if g_aux is None else f(g_aux, abi.AUX_DIM)
        oq, ov, ow = torch.empty_like(gq), torch.empty_like(gv), torch.empty_like(gw)
        oa, oaux = torch.empty_like(act), torch.empty_like(ga)
        check(lib().mjl_env_step_vjp_full(self.data.handle, _ptr(act), _ptr(gq), _ptr(gv), _ptr(gw), _ptr(gr),
                                          _ptr(ga), _ptr(oq), _ptr(ov), _ptr(ow), _ptr(oa), _ptr(oaux),
                                          _ptr(nonfinite), _stream()))
        return oq, ov, ow, oa, oaux

    @property
    def state_size(self) -> int:
        return int(lib().mjl_state_size(self.data.handle))

    def get_state(self, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The persistent per-env state as packed rows [num_envs, state_size] = [qpos | qvel |
        qacc_warmstart | aux | time] (one launch)."""
        if out is None:
            out = torch.empty((self.num_envs, self.state_size), dtype=torch.float32, device=self.obs.device)
        check(lib().mjl_get_state(self.data.handle, _ptr(out), _stream()))
        return out

    def set_state(self, src: torch.Tensor, ws_src: Optional[torch.Tensor] = None):
        """Restore packed rows (get_state layout); qacc_warmstart from ws_src's rows if given."""
        check(lib().mjl_set_state(self.data.handle, _ptr(src.contiguous()), _ptr(ws_src), _stream()))

    @property
    def aux(self) -> torch.Tensor:
        return self.data.get("aux")

    def render(self, camera="side_view", width: int = 64, height: int = 64, shadows: bool = True, rgb: bool = True,
               depth: bool = False, seg: bool = False):
        """Per-env camera images of the batch's current qpos, [num_envs, H, W, .] each (render.Frames): the
        pixel-observation entry. Forward kinematics only; the batch is not touched."""
        if getattr(self, "_renderer", None) is None:
            from .render import Renderer
            self._renderer = Renderer(self.sys, self.num_envs, self.data.device.index or 0)
        return self._renderer.render(self.data.get("qpos"), camera, width, height, shadows, rgb, depth, seg)


def gym_humanoid_obs(sys: Model, d: Data, body) -> torch.Tensor:
    """The Gym Humanoid observation of every env, [nenv, (nq - 2) + nv + 10 (nbody - 1) + 6 (nbody - 1) + nv +
    6 (nbody - 1)]: qpos[2:], qvel, cinert[1:], cvel[1:], qfrc_actuator, cfrc_ext[1:] in Gym's order, from `d`
    and a mjx.BodyData holding cinert, cvel and cfrc_ext of the same state (asking for cfrc_ext runs the forward
    pass that also leaves qfrc_actuator). Plain torch; the trainers do not use it."""
    for f in ("cinert", "cvel", "cfrc_ext"):
        if getattr(body, f) is None:
            raise MjlError(f"gym_humanoid_obs needs body.{f} (mjx.body_data(..., fields=('cinert', 'cvel', 'cfrc_ext')))")
    n = d.nenv
    return torch.cat([d.get("qpos")[:, 2:], d.get("qvel"), body.cinert[:, 1:].reshape(n, -1),
                      body.cvel[:, 1:].reshape(n, -1), d.get("qfrc_actuator"), body.cfrc_ext[:, 1:].reshape(n, -1)],
                     dim=1)


class EnvState(NamedTuple):
    """The `(mjx.Data, aux)` pair v_reset / v_step pass around (src/envs.py:200,490). `data` is the
    device-resident batch, updated in place by v_step; `aux` [B, 9] is a view of its aux rows."""
    data: Data
    aux: torch.Tensor


def create_env_functions(sys: Model, cfg: EnvConfig, q0=None, nq: Optional[int] = None, nv: Optional[int] = None,
                         device: int = 0, key_mode: int = 1):
    """Reference `create_env_functions(sys, cfg, q0, nq, nv)` (src/envs.py:26,494-497): returns
    `(single_reset, single_step, v_reset, v_step)` with the reference's argument meaning.

    * `v_reset(keys [B, 2] uint32/int32)` -> `(EnvState, obs [B, obs_dim])`: every env reset from its
      jax.random key exactly as `single_reset(key)` draws it (src/envs.py:115-202; `mjl_env_set_reset_keys`);
    * `v_step(state, action [B, nu])` -> `(EnvState, obs, reward, terminated, truncated)` (floats
      {0, 1}), no reset merge (src/envs.py:333-492; train_ppo.py merges, here `HumanoidEnv.step`
      does it in the same launch);
    * `single_reset(key [2])` / `single_step(state, action [nu])`: the same on a one-env batch.

    Not functional: the returned state aliases the batch, which v_step advances in place (the
    library owns the device state; keeping old states would mean copying the pytree every step, the
    cost the fused step avoids). One batch per B is built on first use. `q0` must be the model's
    qpos0 (the reset base; the kernel takes it from the model), `nq` / `nv` the model's sizes.
    The trainers use `HumanoidEnv` directly (step with the fused auto-reset)."""
    import numpy as np
    if nq is not None and nq != sys.nq or nv is not None and nv != sys.nv:
        raise MjlError(f"nq/nv ({nq}, {nv}) do not match the model ({sys.nq}, {sys.nv})")
    if q0 is not None and not np.allclose(np.asarray(q0, np.float64), np.asarray(sys.m.qpos0, np.float64), atol=1e-6):
        raise MjlError("q0 must equal the model's qpos0 (the reset base of the native env)")
    envs = {}

    def _env(B: int) -> HumanoidEnv:
        if B not in envs:
            envs[B] = HumanoidEnv(sys, cfg, B, device=device)
        return envs[B]

    def v_reset(keys: torch.Tensor):
        keys = torch.as_tensor(keys)
        if keys.dim() != 2 or keys.shape[1] != 2:
            raise MjlError("keys must have shape [B, 2]")
        env = _env(keys.shape[0])
        k = keys.to(torch.int64).to(torch.int32).to(env.obs.device).contiguous()
        env.set_reset_keys(k, key_mode)
        obs = env.reset().clone()
        env.set_reset_keys(None)
        return EnvState(env.data, env.aux), obs

    def v_step(state: EnvState, action: torch.Tensor):
        env = next((e for e in envs.values() if e.data is state.data), None)
        if env is None:
            raise MjlError("state does not come from this v_reset")
        obs, rew, term, trunc = env.step(action, auto_reset=False)
        return EnvState(env.data, env.aux), obs.clone(), rew.clone(), term.clone(), trunc.clone()

    def single_reset(key: torch.Tensor):
        st, obs = v_reset(torch.as_tensor(key).reshape(1, 2))
        return st, obs[0]

    def single_step(state: EnvState, action: torch.Tensor):
        st, obs, rew, term, trunc = v_step(state, torch.as_tensor(action).reshape(1, -1))
        return st, obs[0], rew[0], term[0], trunc[0]

    return single_reset, single_step, v_reset, v_step
