"""The primal solver's wave-uniform decisions run as scalar branches and selects, and envs of at most
64 rows skip the passes over rows 64.. (step_kernels.hip solver_t / solver_linesearch / solver_update).
Neither changes a float operation, so these cases pin the paths the rewrite touches at the smallest
shapes that reach them: the speed-test step, the truncated CG zoom loop (every swap rule decides the
answer), the wide (nefc > 64) line search next to a narrow env in one batch, and the NaN stop."""
import numpy as np
import pytest
import torch

import mjx_amd
from mjx_amd import abi, mjcf, mjx
from mjx_amd.config import reference_ppo_config
from mjx_amd.envs import HumanoidEnv, resolve_ids
from oracle import Oracle, state_arrays

pytestmark = pytest.mark.gpu


def _load(sys_, states):
    d = mjx.make_data(sys_, len(states))
    for i, f in enumerate(("qpos", "qvel", "qacc_warmstart", "ctrl")):
        d.set(f, torch.tensor(np.array([s[i] for s in states]), dtype=torch.float32))
    return d


def _random_states(m, n, seed):
    """Contact-rich states: random poses dropped towards the floor, rolled out by the oracle."""
    rng = np.random.default_rng(seed)
    od = Oracle(m)
    out = []
    for _ in range(n):
        q = m.qpos0.copy()
        q[7:] += rng.uniform(-0.3, 0.3, m.nq - 7)
        q[2] += rng.uniform(-0.25, 0.05)
        s = od.new_state(q, rng.uniform(-1, 1, m.nv), ctrl=rng.uniform(-1, 1, m.nu))
        od.rollout(s, rng.uniform(-1, 1, (int(rng.integers(1, 40)), m.nu)))
        a = state_arrays(m, s)
        out.append((a["qpos"], a["qvel"], a["qacc_warmstart"], rng.uniform(-1, 1, m.nu)))
    return [tuple(np.float32(x).astype(np.float64) for x in st) for st in out]


def test_speedtest_parity_64():
    """(a) humanoid_mjx speed-test step, B = 64, against the oracle: every env's qpos[0] to 1e-6."""
    m = mjx_amd.load_model("humanoid_mjx")
    sys_ = mjx.put_model(m)
    vel = torch.linspace(0, 1, 64, device="cuda")
    out = mjx.speedtest_step(sys_, mjx.make_data(sys_, 64), vel).cpu().numpy()
    ref = Oracle(m).speedtest(vel.cpu().numpy().astype(np.float64))
    print("speedtest B=64 max |err|", np.abs(out - ref).max())
    np.testing.assert_allclose(out, ref, atol=1e-6)


def test_truncated_cg_step():
    """(b) CG, 4 iterations, 4 line-search iterations (train_apg.py's override): one step of 8 envs
    against the fp32 oracle, 5e-3 * (1 + max|qvel|) as in test_cg_solver_parity. With the zoom loop cut
    at 4 iterations the result depends on each swap rule, now a select."""
    m = mjx_amd.load_model("humanoid_mjx")
    states = _random_states(m, 8, seed=21)  # before the override: Newton-made warm starts
    m.solver, m.iterations, m.ls_iterations = mjcf.SOLVER_CG, 4, 4
    sys_ = mjx.put_model(m)
    d = _load(sys_, states)
    mjx.step(sys_, d)
    v1 = d.get("qvel").cpu().numpy()
    nit = d.get("stats").cpu().numpy()[:, 2]
    orc = Oracle(m, use_float=True)
    errs = []
    for i, (q, v, w, c) in enumerate(states):
        a = state_arrays(m, orc.step(orc.new_state(q, v, w, c)))
        errs.append(np.abs(v1[i] - a["qvel"]).max() / (1 + np.abs(a["qvel"]).max()))
    print("truncated CG: errs", np.array(errs), "iterations", nit)
    assert nit.max() == 4  # the cap is reached: the truncated loop ran
    assert max(errs) <= 5e-3, f"worst env {max(errs):.2e}"


def test_wide_and_narrow_line_search_in_one_batch():
    """(c) The 89-row pose of test_overflow_state_parity (the wide line search: a second register slot
    for rows 64..127) stepped once next to contact-rich envs of fewer than 64 rows. The wide env keeps
    that test's check (the oracle's row count; the optimality condition M (qacc - qacc_smooth) =
    qfrc_constraint to 2e-3 * (1 + max|qfrc_constraint|)); each narrow env's result is bit for bit what
    it is in a batch without the wide env, on the LDS rows and, forced onto the global slab where the
    variant is chosen at run time, there too (and the two storages agree)."""
    m = mjx_amd.load_model("humanoid_mjx")
    sys_ = mjx.put_model(m)
    q = m.key_qpos[m.names["key"].index("supine")].copy()
    for j in range(1, m.njnt):
        q[m.jnt_qposadr[j]] = m.jnt_range[j][1] + 0.05
    wide = tuple(np.float32(x).astype(np.float64) for x in (q, np.zeros(m.nv), np.zeros(m.nv), np.zeros(m.nu)))
    narrow = _random_states(m, 3, seed=22)
    fields = ("qpos", "qvel", "qacc", "sensordata")

    def run(states, force):
        d = _load(sys_, states)
        d.set_option(abi.OPT_FORCE_GLOBAL_ROWS, force)
        mjx.step(sys_, d)
        return d, [d.get(f).cpu().numpy() for f in fields]

    d, mixed = run([narrow[0], wide, narrow[1], narrow[2]], 0)
    st = d.get("stats").cpu().numpy()
    a = state_arrays(m, Oracle(m).forward(Oracle(m).new_state(wide[0])))
    assert st[1][1] == a["nefc"] and a["nefc"] > 64
    assert (st[[0, 2, 3], 1] < 64).all() and (st[[0, 2, 3], 1] > 0).all()
    qacc, qsm, fcon = (d.get(f).cpu().numpy()[1].astype(np.float64) for f in ("qacc", "qacc_smooth", "qfrc_constraint"))
    resid = a["M"] @ (qacc - qsm) - fcon
    print("wide env: nefc", st[1][1], "residual", np.abs(resid).max(), "bound", 2e-3 * (1 + np.abs(fcon).max()))
    assert np.abs(resid).max() <= 2e-3 * (1 + np.abs(fcon).max())
    _, alone = run(narrow, 0)
    _, mixed_g = run([narrow[0], wide, narrow[1], narrow[2]], 1)
    for x, y, z in zip(mixed, alone, mixed_g):
        np.testing.assert_array_equal(x[[0, 2, 3]], y)
        np.testing.assert_array_equal(x, z)


def test_nan_stops_the_solver():
    """(d) NaN in one env's qvel: its line search returns NaN costs, the solver stops (no hang), the
    env step raises that env's non-finite flag (stats[:, 3]) and no other's."""
    B, bad = 4, 2
    m = mjx_amd.load_model("humanoid_mjx")
    sys_ = mjx.put_model(m)
    cfg = resolve_ids(m, reference_ppo_config().env_config)
    env = HumanoidEnv(sys_, cfg, B, seed=5, store_derived=True)
    env.reset()
    qv = env.data.get("qvel").clone()
    qv[bad, 0] = float("nan")
    env.data.set("qvel", qv)
    env.step(torch.zeros((B, m.nu), device="cuda"), auto_reset=False)
    torch.cuda.synchronize()
    st = env.data.get("stats").cpu().numpy()
    print("nan env: stats", st[bad], "iterations of the others", np.delete(st[:, 2], bad))
    assert st[bad, 3] == 1.0 and (np.delete(st[:, 3], bad) == 0.0).all()
    assert st[bad, 2] <= m.iterations
    assert torch.isfinite(env.data.get("qpos")[[i for i in range(B) if i != bad]]).all()
