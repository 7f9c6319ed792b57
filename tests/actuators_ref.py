"""float64 restatement of the general actuator (MJX forward.fwd_actuation, joint transmission on a hinge) and
the motor models that tie it to the oracle, which has motors only:

  forces      F_u = clip(gain_u clip(ctrl_u) + b0_u + b1_u gear_u qpos[j] + b2_u gear_u qvel[d], forcerange_u)
  euler       motors, same gear, ctrllimited off, ctrl'_u = F_u: the same qfrc_actuator
  implicit    also dof_damping'[d] = dof_damping[d] - sum_u gear_u^2 b2_u and ctrl'_u = F_u - b2_u gear_u qvel[d]:
              the same total smooth force and the same integrator matrix M + dt diag(damping')."""
import dataclasses

import numpy as np

from mjx_amd.mjcf import GENERAL_ACTUATOR_ARRAYS, general_actuator_arrays

MODELS = ["humanoid_mjx", "humanoid"]
INTEGRATORS = {"euler": 0, "implicitfast": 3}


def with_arrays(m, integrator=None, **arrays):
    """A copy of compiled model m with arrays replaced (and nu following actuator_trnid)."""
    A = {k: np.array(v, copy=True) for k, v in {**m.arrays, **arrays}.items()}
    kw = {"arrays": A, "nu": len(A["actuator_trnid"])}
    if integrator is not None:
        kw["integrator"] = INTEGRATORS[integrator]
    return dataclasses.replace(m, **kw)


def general_model(m, kp, kv, seed, integrator=None, forcerange=None, damping=None, extra_velocity=0):
    """m's motors as general actuators that keep the motors' gear: joint-space stiffness kp and damping kv, so
    b1 = -kp / gear^2, b2 = -kv / gear^2; gain in [0.5, 1.5] and b0 in [-0.2, 0.2] drawn from `seed`.
    forcerange f: clamp to [-f, 0.7 f]. extra_velocity n: n more actuators, <velocity>-like, on the first n
    actuated joints (two actuators on one dof)."""
    rng = np.random.default_rng(seed)
    nu = m.nu
    gear = np.asarray(m.actuator_gear, np.float64)
    gain, b0 = rng.uniform(0.5, 1.5, nu), rng.uniform(-0.2, 0.2, nu)
    bias = np.stack([b0, -kp / gear**2 * np.ones(nu), -kv / gear**2 * np.ones(nu)], 1)
    arrays = {}
    trnid, cr, cl = (np.asarray(m.arrays[k]) for k in ("actuator_trnid", "actuator_ctrlrange", "actuator_ctrllimited"))
    if extra_velocity:
        n = extra_velocity
        xg = rng.uniform(5.0, 15.0, n)
        gear, gain = np.concatenate([gear, xg]), np.concatenate([gain, rng.uniform(0.5, 1.5, n)])
        bias = np.concatenate([bias, np.stack([np.zeros(n), np.zeros(n), -rng.uniform(0.5, 2.0, n) / xg**2], 1)])
        trnid, cr, cl = np.concatenate([trnid, trnid[:n]]), np.concatenate([cr, cr[:n]]), np.concatenate([cl, cl[:n]])
        arrays.update(actuator_trnid=trnid, actuator_gear=gear, actuator_ctrlrange=cr, actuator_ctrllimited=cl)
    nu = len(gear)
    flim = np.zeros(nu, np.int32) if forcerange is None else np.ones(nu, np.int32)
    fr = np.zeros((nu, 2)) if forcerange is None else np.tile([-forcerange, 0.7 * forcerange], (nu, 1))
    arrays.update(general_actuator_arrays(np.ones(nu, np.int32), gain, bias, flim, fr))
    if damping is not None:
        arrays["dof_damping"] = np.full(m.nv, float(damping))
    g = with_arrays(m, integrator, **arrays)
    if extra_velocity:
        g.names = {**m.names, "actuator": list(m.names["actuator"]) + [f"extra{i}" for i in range(extra_velocity)]}
    return g


def _adr(g):
    j = np.asarray(g.actuator_trnid)
    return np.asarray(g.jnt_qposadr)[j], np.asarray(g.jnt_dofadr)[j]


def forces(g, qpos, qvel, ctrl):
    """(F [nu] after the clamp, unclamped [nu], qfrc_actuator [nv]) in float64."""
    qadr, dof = _adr(g)
    gear = np.asarray(g.actuator_gear, np.float64)
    c = np.asarray(ctrl, np.float64)
    lim = np.asarray(g.actuator_ctrllimited) != 0
    c = np.where(lim, np.clip(c, g.actuator_ctrlrange[:, 0], g.actuator_ctrlrange[:, 1]), c)
    b = np.asarray(g.actuator_biasprm, np.float64)
    raw = g.actuator_gain * c + b[:, 0] + b[:, 1] * (gear * qpos[qadr]) + b[:, 2] * (gear * qvel[dof])
    fl = np.asarray(g.actuator_forcelimited) != 0
    F = np.where(fl, np.clip(raw, g.actuator_forcerange[:, 0], g.actuator_forcerange[:, 1]), raw)
    q = np.zeros(g.nv)
    np.add.at(q, dof, gear * F)
    return F, raw, q


def motor_model(g, implicit):
    """The oracle's model for g: motors of the same gear without ctrl limits; with `implicit` the damping that
    carries the actuators' velocity derivative."""
    arrays = {k: v for k, v in g.arrays.items() if k not in GENERAL_ACTUATOR_ARRAYS}
    arrays["actuator_ctrllimited"] = np.zeros(g.nu, np.int32)
    if implicit:
        _, dof = _adr(g)
        d = np.array(g.dof_damping, np.float64)
        np.add.at(d, dof, -np.asarray(g.actuator_gear) ** 2 * np.asarray(g.actuator_biasprm)[:, 2])
        arrays["dof_damping"] = d
    return dataclasses.replace(g, arrays={k: np.array(v, copy=True) for k, v in arrays.items()})


def motor_ctrl(g, qpos, qvel, ctrl, implicit):
    F, _, _ = forces(g, qpos, qvel, ctrl)
    if implicit:
        _, dof = _adr(g)
        F = F - np.asarray(g.actuator_biasprm)[:, 2] * np.asarray(g.actuator_gear) * qvel[dof]
    return F
