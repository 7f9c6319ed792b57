"""Domain randomisation draws for per-env model parameters (Data.set_model_params / HumanoidEnv.set_model_params).

The reference stack randomises a model by vmapping a function that scales fields of the mjx.Model (Brax's
`domain_randomize`: friction, gains, masses drawn per env, `sys.tree_replace` under `jax.vmap`). Here the draw
is a host function over the compiled model: it returns the six tensors the library takes, float32 [nenv, dim],
on the CPU (move them to the batch's device; pure numpy / torch, no GPU needed).
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

FIELDS = ("body_mass", "body_inertia", "dof_damping", "dof_armature", "actuator_gear", "pair_friction")
RANGES = ("mass", "friction", "damping", "armature", "gear")


def pair_friction_from_geoms(model, geom_scale: np.ndarray) -> np.ndarray:
    """pair_friction[:, 0] [nenv, npair] for per-geom sliding-friction scales [nenv, ngeom]: the pair takes
    max(scaled geom1, scaled geom2), the rule the MJCF compiler mixes equal-priority geoms with
    (mjcf.candidate pairs: `fr = np.maximum(A["friction"], B["friction"])`). A pair whose compiled value is not
    that maximum (an explicit <pair> with its own friction) is scaled by the larger of its geoms' scales."""
    g1, g2 = np.asarray(model.pair_geom1), np.asarray(model.pair_geom2)
    gf = np.asarray(model.geom_friction, np.float64)[:, 0]
    nominal = np.asarray(model.pair_friction, np.float64).reshape(-1, 5)[:, 0]
    s = np.asarray(geom_scale, np.float64)
    mixed = np.maximum(gf[g1] * s[:, g1], gf[g2] * s[:, g2])
    by_rule = nominal == np.maximum(gf[g1], gf[g2])
    return np.where(by_rule[None, :], mixed, nominal[None, :] * np.maximum(s[:, g1], s[:, g2]))


def draw_model_params(model, nenv: int, ranges: Dict[str, Optional[Tuple[float, float]]],
                      seed: int = 0) -> Dict[str, torch.Tensor]:
    """Uniform scale draws per env -> {"body_mass": [nenv, nbody], "body_inertia": [nenv, nbody, 6],
    "dof_damping" / "dof_armature": [nenv, nv], "actuator_gear": [nenv, nu], "pair_friction": [nenv, npair]}.

    ranges: (lo, hi) scale ranges by name; a name left out or None keeps the model's values (scale 1):
      mass      one scale per body; the body's inertia is scaled with it (the same shape, denser or lighter)
      friction  one scale per geom; a pair takes max(scaled geom1, scaled geom2) (pair_friction_from_geoms)
      damping, armature   one scale per dof
      gear      one scale per actuator
    Every draw comes from numpy's default_rng(seed), field by field in the order above, so a (model, nenv,
    ranges, seed) names one randomisation."""
    unknown = set(ranges) - set(RANGES)
    if unknown:
        raise ValueError(f"unknown range {sorted(unknown)} (known: {list(RANGES)})")
    rng = np.random.default_rng(seed)
    n = int(nenv)

    def scale(name, dim):
        r = ranges.get(name)
        if r is None:
            return np.ones((n, dim))
        lo, hi = float(r[0]), float(r[1])
        if not 0 <= lo <= hi:
            raise ValueError(f"{name}: need 0 <= lo <= hi, got {r}")
        return rng.uniform(lo, hi, (n, dim))

    sm = scale("mass", model.nbody)
    out = {
        "body_mass": np.asarray(model.body_mass, np.float64)[None, :] * sm,
        "body_inertia": np.asarray(model.body_inertia, np.float64).reshape(1, model.nbody, 6) * sm[:, :, None],
        "pair_friction": pair_friction_from_geoms(model, scale("friction", model.ngeom)),
        "dof_damping": np.asarray(model.dof_damping, np.float64)[None, :] * scale("damping", model.nv),
        "dof_armature": np.asarray(model.dof_armature, np.float64)[None, :] * scale("armature", model.nv),
        "actuator_gear": np.asarray(model.actuator_gear, np.float64)[None, :] * scale("gear", model.nu),
    }
    return {k: torch.from_numpy(np.ascontiguousarray(out[k], np.float32)) for k in FIELDS}
