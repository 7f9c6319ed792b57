"""Shared by tests/test_model_params_abi.py and tests/test_model_params_gpu.py: the draw the per-env model
parameter tests use, and the model "with env i's values substituted" that the library's rule refers to."""
import numpy as np

import mjx_amd
from mjx_amd.randomize import FIELDS, draw_model_params

MODELS = ["humanoid_mjx", "humanoid"]
# the modest ranges of the physics check: mass 0.5-1.5, friction 0.3-1.5, damping / armature 0.5-2, gear 0.7-1.3
RANGES = {"mass": (0.5, 1.5), "friction": (0.3, 1.5), "damping": (0.5, 2.0), "armature": (0.5, 2.0),
          "gear": (0.7, 1.3)}
SEED = 20


def draw(m, n):
    """The tests' draw: every env its own value of all six fields; env n // 2 has no damping at all (the
    any_damping flag of its block differs from the damped model's)."""
    p = {k: v.numpy().copy() for k, v in draw_model_params(m, n, RANGES, SEED).items()}
    p["dof_damping"][n // 2] = 0
    return p


def substituted(name, params, i, fields=FIELDS, zero_damping=False):
    """A fresh compiled model `name` whose descriptor fields take env i's values of `params` (float32 values,
    held as float64: `(double)(float)`), nothing else recomputed. zero_damping: the base model's damping is
    zeroed first (for a nominal model without damping)."""
    m = mjx_amd.load_model(name)
    A = m.arrays
    if zero_damping:
        A["dof_damping"] = np.zeros_like(A["dof_damping"])
    for k in fields:
        v = np.asarray(params[k][i], np.float32).astype(np.float64)
        if k == "pair_friction":
            A[k] = np.array(A[k], np.float64).reshape(-1, 5)
            # the sliding coefficient: MuJoCo keeps it twice, [0] and [1], one per tangent direction, always
            # equal for a compiled model; the kernels read [0] as the mu of both, the oracle reads both
            A[k][:, 0] = A[k][:, 1] = v
        else:
            A[k] = v.reshape(np.shape(A[k]))
    return m


def nominal_params(m, n):
    """The six fields of the compiled model itself, one row per env (float32, as the library holds them)."""
    return {k: v.numpy().copy() for k, v in draw_model_params(m, n, {}, 0).items()}
