"""Start states and actions of the substep tests (test_substeps.py picks and checks them on the float64 oracle,
test_substeps_gpu.py runs them), computed once per model and shared.

A case is B envs of one model: states reached by seeded oracle rollouts of 120 to 225 steps from a lowered
random pose (the body has come down on the floor and is still moving, so contacts are made and broken), and one action per env in [-1.3, 1.3] (some components clip).
`contact_counts(name, nstep)` is the oracle's active contact count of every env in every substep."""
import functools

import numpy as np

import mjx_amd
from oracle import Oracle, state_arrays

B = 8
MAXK = 5  # the longest fused step of the GPU cases
SEEDS = {"humanoid_mjx": 11, "humanoid": 12, "tail": 13}


@functools.lru_cache(maxsize=None)
def model(name):
    if name == "tail":
        import generic_models
        return generic_models.tail()
    return mjx_amd.load_model(name)


@functools.lru_cache(maxsize=None)
def case(name):
    """(qpos [B, nq], qvel [B, nv], qacc_warmstart [B, nv], act [B, nu]) as float32-exact float64 arrays."""
    m = model(name)
    rng = np.random.default_rng(SEEDS[name])
    orc = Oracle(m)
    rows = []
    for e in range(B):
        q = m.qpos0.copy()
        q[7:] += rng.uniform(-0.3, 0.3, m.nq - 7)
        q[2] += rng.uniform(-0.25, 0.0)
        s = orc.new_state(q, rng.uniform(-1, 1, m.nv), ctrl=rng.uniform(-1, 1, m.nu))
        orc.rollout(s, rng.uniform(-0.4, 0.4, (120 + 15 * e, m.nu)))  # down on the floor, still moving
        a = state_arrays(m, s)
        rows.append((a["qpos"], a["qvel"], a["qacc_warmstart"], rng.uniform(-1.3, 1.3, m.nu)))
    return tuple(np.float32(np.array([r[i] for r in rows])).astype(np.float64) for i in range(4))


@functools.lru_cache(maxsize=None)
def contact_counts(name, nstep=MAXK):
    """ncon [B, nstep] of the oracle's forward pass in each of nstep physics steps under the case's clipped action
    (the unflipped control: what mjl_step_n runs, and the env step of every env whose flip is off)."""
    m = model(name)
    q, v, w, act = case(name)
    orc = Oracle(m)
    out = np.zeros((B, nstep), int)
    for e in range(B):
        s = orc.new_state(q[e], v[e], w[e], np.clip(act[e], -1, 1))
        for k in range(nstep):
            orc.step(s)
            out[e, k] = s.ncon
    return out
