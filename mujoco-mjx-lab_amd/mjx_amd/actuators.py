"""General (PD) actuators on compiled models.

The step kernels run MuJoCo's stateless general actuator with joint transmission on a hinge (include/mjx355.h,
DESIGN.md "Actuators"):

    force = gain * clip(ctrl) + b0 + b1 * gear * qpos[j] + b2 * gear * qvel[d],  clipped to forcerange
    qfrc_actuator[d] += gear * force

`pd_actuators` turns a model's torque motors into joint-target PD controllers that keep the motors' torque limits:
the policy's action becomes a joint target around the model's default pose instead of a torque.
"""
from __future__ import annotations

import dataclasses

import numpy as np

from .mjcf import ACT_GENERAL, GENERAL_ACTUATOR_ARRAYS, CompiledModel, MJCFError, general_actuator_arrays


def has_general_actuators(m: CompiledModel) -> bool:
    return "actuator_kind" in m.arrays and bool(np.any(np.asarray(m.arrays["actuator_kind"]) != 0))


def _per_actuator(x, nu: int, what: str) -> np.ndarray:
    v = np.asarray(x, np.float64)
    if v.ndim == 0:
        return np.full(nu, float(v))
    if v.shape != (nu,):
        raise ValueError(f"{what}: a scalar or an array of {nu} values (one per actuator), got shape {v.shape}")
    return v.copy()


def pd_actuators(m: CompiledModel, kp, kv, action_scale=1.0) -> CompiledModel:
    """A copy of `m` whose motors are general actuators holding joint targets:

        target_j = qpos0_j + action_scale * ctrl,   torque = kp (target_j - qpos_j) - kv qvel_j,

    clipped to the motor's torque limit, i.e. per actuator gain = kp * action_scale, biasprm = (kp * qpos0_j, -kp,
    -kv), gear 1, ctrlrange / ctrllimited the motor's, forcerange = +- |gear| * max|ctrlrange| (limited iff the
    motor's ctrl is). `kp`, `kv` and `action_scale` are scalars or arrays of one value per actuator. `m` is not
    modified; only a model of motors alone is accepted."""
    if has_general_actuators(m):
        raise MJCFError("pd_actuators: the model already has general actuators")
    nu = m.nu
    kp, kv, scale = (_per_actuator(x, nu, n) for x, n in ((kp, "kp"), (kv, "kv"), (action_scale, "action_scale")))
    A = {k: np.array(v, copy=True) for k, v in m.arrays.items() if k not in GENERAL_ACTUATOR_ARRAYS}
    qadr = np.asarray(A["jnt_qposadr"])[np.asarray(A["actuator_trnid"])]
    q0 = np.asarray(A["qpos0"], np.float64)[qadr]
    limit = np.abs(np.asarray(A["actuator_gear"], np.float64)) * np.abs(np.asarray(A["actuator_ctrlrange"], np.float64)).max(1)
    A["actuator_gear"] = np.ones(nu)
    A.update(general_actuator_arrays(
        kind=np.full(nu, ACT_GENERAL), gain=kp * scale, biasprm=np.stack([kp * q0, -kp, -kv], 1),
        forcelimited=np.asarray(A["actuator_ctrllimited"], np.int32).copy(), forcerange=np.stack([-limit, limit], 1)))
    return dataclasses.replace(m, arrays=A, names={k: list(v) for k, v in m.names.items()})
