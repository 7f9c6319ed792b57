"""One Newton / CG iteration passes over the rows once: the line search leaves the new point's jar, D,
qacc and Ma in registers, solver_update takes them and derives the active set once, and the exact-exit
test, the Hessian's row selection and the FLOP count share that one set (step_kernels.hip IterRegs,
ActiveSet). No float operation changes, so these cases pin the paths at the smallest shapes that
reach them, against the fp32 oracle with the bounds of tests/test_solver_branches.py
(5e-3 * (1 + max|ref|) per env and quantity)."""
import numpy as np
import pytest
import torch

import mjx_amd
from mjx_amd import abi, mjcf, mjx
from oracle import Oracle, state_arrays
from test_solver_branches import _load, _random_states

pytestmark = pytest.mark.gpu

FIELDS = ("qpos", "qvel", "qacc", "sensordata")
REL = 5e-3


@pytest.fixture(scope="module")
def model_states():
    m = mjx_amd.load_model("humanoid_mjx")
    return m, _random_states(m, 24, seed=31)


def _fresh():
    return mjx_amd.load_model("humanoid_mjx")


def _airborne(m):
    """No contact, no limit row: nefc == 0."""
    q = m.qpos0.copy()
    q[2] += 1.0
    return tuple(np.float32(x).astype(np.float64) for x in (q, np.zeros(m.nv), np.zeros(m.nv), np.zeros(m.nu)))


def _step(m, states, forward_first=False):
    sys_ = mjx.put_model(m)
    d = _load(sys_, states)
    if forward_first:
        mjx.forward(sys_, d)
        np.testing.assert_array_equal(d.get("qacc_warmstart").cpu().numpy(), d.get("qacc").cpu().numpy())
    mjx.step(sys_, d)
    return {f: d.get(f).cpu().numpy() for f in FIELDS + ("stats",)}


def _check_against_oracle(m, states, got, what, forward_first=False, skip=()):
    orc = Oracle(m, use_float=True)
    worst = {f: 0.0 for f in FIELDS}
    for i, (q, v, w, c) in enumerate(states):
        if i in skip:
            continue
        s = orc.new_state(q, v, w, c)
        if forward_first:
            s = orc.forward(s)
        a = state_arrays(m, orc.step(s))
        for f in FIELDS:
            ref = np.asarray(a[f], np.float64)
            err = np.abs(got[f][i] - ref).max() / (1 + np.abs(ref).max()) if ref.size else 0.0
            worst[f] = max(worst[f], err)
            assert err <= REL, f"{what}: env {i} {f}: {err:.2e}"
    print(what, "worst relative errors", worst)


def test_changing_active_set_next_to_first_exit_and_empty(model_states):
    """Contact-rich envs whose active set changes between Newton iterations (>= 3 iterations), envs that
    leave on the first exact-exit test (1 iteration) and envs without rows, in one batch."""
    m, rnd = model_states
    states = rnd + [_airborne(m)] * 2
    got = _step(m, states)
    nefc, nit = got["stats"][:, 1], got["stats"][:, 2]
    print("nefc", nefc, "iterations", nit)
    assert nit.max() >= 3 and (nit == 1).any() and (nefc[-2:] == 0).all() and (nit[-2:] == 0).all()
    _check_against_oracle(m, states, got, "changing active set")


def test_wide_env_next_to_narrow_envs(model_states):
    """An env of more than 64 rows (global slab, the second register slot and its mask word) between
    narrow envs: the wide env meets the optimality condition as in test_solver_branches, the narrow
    envs the oracle, and they are bit for bit what they are without the wide env."""
    m, rnd = model_states
    q = m.key_qpos[m.names["key"].index("supine")].copy()
    for j in range(1, m.njnt):
        q[m.jnt_qposadr[j]] = m.jnt_range[j][1] + 0.05
    wide = tuple(np.float32(x).astype(np.float64) for x in (q, np.zeros(m.nv), np.zeros(m.nv), np.zeros(m.nu)))
    narrow = rnd[:3]
    states = [narrow[0], wide, narrow[1], narrow[2]]
    sys_ = mjx.put_model(m)
    d = _load(sys_, states)
    mjx.step(sys_, d)
    got = {f: d.get(f).cpu().numpy() for f in FIELDS + ("stats",)}
    a = state_arrays(m, Oracle(m).forward(Oracle(m).new_state(wide[0])))
    assert got["stats"][1][1] == a["nefc"] and a["nefc"] > 64
    assert (got["stats"][[0, 2, 3], 1] < 64).all()
    qacc, qsm, fcon = (d.get(f).cpu().numpy()[1].astype(np.float64) for f in ("qacc", "qacc_smooth", "qfrc_constraint"))
    resid = a["M"] @ (qacc - qsm) - fcon
    print("wide env: nefc", got["stats"][1][1], "iterations", got["stats"][1][2], "residual", np.abs(resid).max())
    assert np.abs(resid).max() <= 2e-3 * (1 + np.abs(fcon).max())
    _check_against_oracle(m, states, got, "wide next to narrow", skip=(1,))
    alone = _step(m, narrow)
    for f in FIELDS:
        np.testing.assert_array_equal(got[f][[0, 2, 3]], alone[f])
    d = _load(sys_, states)  # every env on the global slab: the variant is chosen at run time
    d.set_option(abi.OPT_FORCE_GLOBAL_ROWS, 1)
    mjx.step(sys_, d)
    for f in FIELDS:
        np.testing.assert_array_equal(got[f], d.get(f).cpu().numpy())


@pytest.mark.parametrize("iterations", [1, 2])
def test_iteration_limits(model_states, iterations):
    """iterations == 1 (one body, unconditionally) and a cap that cuts the solve short."""
    _, rnd = model_states
    m = _fresh()
    m.iterations = iterations
    got = _step(m, rnd[:8])
    nit = got["stats"][:, 2]
    print("cap", iterations, "iterations", nit)
    assert nit.max() == iterations
    _check_against_oracle(m, rnd[:8], got, f"iterations = {iterations}")


def test_cg_4_4(model_states):
    """CG shares the update and the line search: 4 iterations of 4 line-search iterations."""
    _, rnd = model_states
    m = _fresh()
    m.solver, m.iterations, m.ls_iterations = mjcf.SOLVER_CG, 4, 4
    got = _step(m, rnd[8:16])
    assert got["stats"][:, 2].max() == 4
    _check_against_oracle(m, rnd[8:16], got, "CG 4/4")


def test_forward_then_step(model_states):
    """mjx.forward leaves qacc_warmstart = qacc; the step's solve starts from it."""
    m, rnd = model_states
    got = _step(m, rnd[16:24], forward_first=True)
    _check_against_oracle(m, rnd[16:24], got, "forward then step", forward_first=True)


def test_nan_stops_one_env_only(model_states):
    """A NaN qvel ends that env's loop within the cap; its neighbours equal a run without it."""
    m, rnd = model_states
    states = rnd[:4]
    clean = _step(m, states)
    bad = list(states)
    v = bad[2][1].copy()
    v[0] = np.nan
    bad[2] = (bad[2][0], v, bad[2][2], bad[2][3])
    got = _step(m, bad)
    assert got["stats"][2, 2] <= m.iterations
    keep = [0, 1, 3]
    for f in FIELDS:
        np.testing.assert_array_equal(got[f][keep], clean[f][keep])
        assert np.isfinite(got[f][keep]).all()


@pytest.mark.parametrize("solver,vjp", [("model", "implicit"), ("cg44", "unrolled")])
def test_apg_record_and_replay(solver, vjp):
    """16 envs x 4 steps, record + replay VJP (unrolled: the solve records its tape through the hooks,
    which read jar, qacc, Ma, Jv and Mv from LDS). As tests/test_vjp_scale_gpu.py compares a detached
    trainer with a scaled one: losses, gradients and parameters bit for bit, nothing non-finite."""
    from test_vjp_scale_gpu import _same_update, _trainers
    on = {"scale_cotangents": True, "scale_threshold_log2": 1}
    trs = _trainers(solver, vjp, 16, 4, [{"use_graph": False}, {"use_graph": False, **on}])
    ms = [tr.update(0) for tr in trs]
    _same_update(ms, trs, 0)
    assert ms[0]["nonfinite_envs"] == 0 and ms[0]["grad_norm"] == ms[0]["grad_norm"] and ms[0]["grad_norm"] > 0
    for p in trs[0].policy.parameters():
        assert bool(torch.isfinite(p.grad).all())
