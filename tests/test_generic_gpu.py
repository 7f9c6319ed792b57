"""The generic kernel instantiation (DGen = Dims<32, 32, 32, 32, 32, 16>, csrc/step_kernels.hip) on the GPU
against the fp64 oracle, on the models of tests/generic_models.py: mjl_model_create selects it as soon as one of
nv > 27, nbody > 17, njnt > 22, ngeom > 20 holds, so the models that cross one threshold each, the humanoids
with a tail and `full` (nv = nbody = ngeom = 32) all run it; the near-miss models (one link fewer) run the
humanoid instantiation against the same oracle. What only DGen reaches: the row stride LD = 36, the nv = 32
column of the dense factor + solve, an LDS row capacity of 32 (so the LDS -> global row overflow happens at
ordinary contact counts), and the serial subtree loops for models past 17 bodies.

Tolerances are those of tests/test_gpu_parity.py (fp32 kernel vs fp64 oracle, s = 1 + max|ref| of the env):
xpos, xquat, qpos after a step 2e-5; qfrc_bias / passive / actuator 2e-5 * s; qacc_smooth, qacc,
qfrc_constraint, qvel after a step 2e-3 * s; 20-step trajectories 1e-3; contact / row counts exact.

No env is left out: a contact or limit decided at its activation distance differs between fp32 and fp64, so
every compared state is checked, on the oracle alone, to have no candidate within 1e-4 of activation
(`assert_decided`: the oracle's contact list and row count do not change when every margin moves by -1e-4 or
+1e-4); the states' seeds were chosen for that.

The measured maxima (err / bound per quantity and model) are in profiles/generic/parity.json; a run of this
whole file with MJL_GENERIC_PARITY_OUT=<file> writes them again when the module's tests are done."""
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

from mjx_amd import abi, apg, mjcf, mjx
from mjx_amd.config import reference_ppo_config
from mjx_amd.envs import HumanoidEnv, resolve_ids
from oracle import Oracle, state_arrays

import bodydata_ref as br
import generic_models as gm

pytestmark = pytest.mark.gpu

ALL = list(gm.MODELS)
EPS = 1e-4
ERRS = {}  # (model, quantity) -> max err / bound


@pytest.fixture(scope="module", autouse=True)
def _write_measured_errors():
    """With MJL_GENERIC_PARITY_OUT set, the err / bound maxima this module's tests saw go to that file at its end."""
    yield
    path = os.environ.get("MJL_GENERIC_PARITY_OUT")
    if path:
        with open(path, "w") as f:
            json.dump(dict(sorted(ERRS.items())), f, indent=1)
            f.write("\n")


def _note(name, what, err, bound):
    k = f"{name}/{what}"
    ERRS[k] = max(ERRS.get(k, 0.0), float(err) / float(bound))


def _close(name, what, got, ref, rel):
    ref = np.asarray(ref, np.float64)
    s = 1.0 + (np.abs(ref).max() if ref.size else 0.0)
    err = np.abs(np.asarray(got, np.float64) - ref).max() if ref.size else 0.0
    _note(name, what, err, rel * s)
    assert err <= rel * s, f"{name} {what}: err {err:.3e} > {rel:.1e} * {s:.3g}"


def _abs_close(name, what, got, ref, atol):
    err = np.abs(np.asarray(got, np.float64) - ref).max() if np.size(ref) else 0.0
    _note(name, what, err, atol)
    assert err <= atol, f"{name} {what}: err {err:.3e} > {atol:.1e}"


def _with_margins(m, delta):
    A = {k: np.array(v, copy=True) for k, v in m.arrays.items()}
    for k in ("pair_margin", "jnt_margin", "tendon_margin"):
        A[k] = A[k] + delta
    return dataclasses.replace(m, arrays=A)


_shifted = {}


def decided(m, st):
    """True when no contact candidate, joint limit or tendon limit of state st = (qpos, qvel, warm start, ctrl)
    lies within EPS of its activation distance: the fp64 oracle's contact list and row count are the same with
    every margin at -EPS and +EPS."""
    if id(m) not in _shifted:
        _shifted[id(m)] = (m, [Oracle(_with_margins(m, d)) for d in (-EPS, 0.0, EPS)])
    seen = []
    for o in _shifted[id(m)][1]:
        a = state_arrays(m, o.forward(o.new_state(*st)))
        seen.append((a["ncon"], a["nefc"], a["con_geom"].tolist()))
    return seen[0] == seen[1] == seen[2]


def assert_decided(m, st, what):
    assert decided(m, st), f"{what}: a contact or limit within {EPS} of its activation distance"


def _f32(*xs):
    return tuple(np.float32(x).astype(np.float64) for x in xs)


def _hinges(m):
    return [j for j in range(m.njnt) if m.jnt_type[j] != mjcf.JNT_FREE]


def _free_z(m):
    return [int(m.jnt_qposadr[j]) + 2 for j in range(m.njnt) if m.jnt_type[j] == mjcf.JNT_FREE]


def make_states(m, seed):
    """rest (qpos0 with every free root 2 mm lower: the humanoid stands with its feet within 1e-4 of the floor,
    which is no decided state); three falls (random pose lowered towards the floor, random velocities and controls, 10..40 oracle
    steps, so contacts and limits are active); one of the falls again with two hinges past their range."""
    rng = np.random.default_rng(seed)
    od = Oracle(m)
    q = m.qpos0.copy()
    q[_free_z(m)] -= 0.002
    out = [_f32(q, np.zeros(m.nv), np.zeros(m.nv), np.zeros(m.nu))]
    for k in range(3):
        q = m.qpos0.copy()
        for j in _hinges(m):
            q[int(m.jnt_qposadr[j])] += rng.uniform(-0.3, 0.3)
        for z in _free_z(m):
            q[z] -= rng.uniform(0.0, 0.2) * q[z]
        s = od.new_state(q, rng.uniform(-1, 1, m.nv), ctrl=rng.uniform(-1, 1, m.nu))
        od.rollout(s, rng.uniform(-1, 1, (int(rng.integers(10, 40)), max(m.nu, 1)))[:, :m.nu].copy())
        a = state_arrays(m, s)
        out.append(_f32(a["qpos"], a["qvel"], a["qacc_warmstart"], rng.uniform(-1, 1, m.nu)))
    lim = [j for j in _hinges(m) if m.jnt_limited[j]]
    if lim:
        q, v, w, c = (x.copy() for x in out[1])
        for j, side in zip(rng.choice(lim, 2, replace=False), (0, 1)):
            q[int(m.jnt_qposadr[j])] = m.jnt_range[j][side] + (0.05 if side else -0.05)
            v[int(m.jnt_dofadr[j])] = 0.0
        out.append(_f32(q, 0.5 * v, w, c))
    return out


def thrown(m, rng):
    """Two starts for a model whose rest is no decided state (a slab lying on its spheres keeps them at their
    activation distance): qpos0 lifted 2 to 6 cm, tilted, thrown at the floor at 0.5 to 1.5 m/s, so the contacts
    of the 20 steps are impacts that cross the activation band within one step."""
    out = []
    for _ in range(2):
        q, v = m.qpos0.copy(), rng.uniform(-0.5, 0.5, m.nv)
        q[2] += rng.uniform(0.02, 0.06)
        q[3:7] += rng.uniform(-0.15, 0.15, 4)
        q[3:7] /= np.linalg.norm(q[3:7])
        v[2] = -rng.uniform(0.5, 1.5)
        out.append(_f32(q, v, np.zeros(m.nv), np.zeros(m.nu)))
    return out


_states = {}


def states_of(name):
    """The model's states from the first seed (from 100 up) whose states are all decided (EPS): a choice made on
    the oracle alone. (One step's parity depends on the pre-step rows only.)"""
    if name not in _states:
        m = gm.MODELS[name][0]()
        for seed in range(100, 140):
            st = make_states(m, seed)
            if all(decided(m, s) for s in st):
                _states[name] = st
                break
        else:
            raise AssertionError(f"{name}: no seed in 100..139 gives decided states")
    return _states[name]


_sys = {}


def system(name):
    if name not in _sys:
        m = gm.MODELS[name][0]()
        _sys[name] = (m, mjx.put_model(m))
    return _sys[name]


def _load(sys_, states, m):
    d = mjx.make_data(sys_, len(states))
    t = lambda i: torch.tensor(np.array([s[i] for s in states]), dtype=torch.float32)
    d.set("qpos", t(0))
    d.set("qvel", t(1))
    d.set("qacc_warmstart", t(2))
    if m.nu:
        d.set("ctrl", t(3))
    return d


def _uses_generic(d):
    """The library's own word on the instantiation: mjl_env_record_fused is 1 only for the humanoid kernels
    (rows not forced global, which no caller here has done at that point)."""
    from mjx_amd._lib import lib
    return lib().mjl_env_record_fused(d.handle) == 0


FWD = ("qacc", "qacc_smooth", "qfrc_bias", "qfrc_passive", "qfrc_actuator", "qfrc_constraint", "xpos", "xquat", "stats")


def _forward_check(name, m, sys_, states):
    d = _load(sys_, states, m)
    mjx.forward(sys_, d)
    G = {f: d.get(f).cpu().numpy() for f in FWD}
    orc = Oracle(m)
    for i, st in enumerate(states):
        assert_decided(m, st, f"{name} state {i}")
        a = state_arrays(m, orc.forward(orc.new_state(*st)))
        assert (G["stats"][i][0], G["stats"][i][1]) == (a["ncon"], a["nefc"]), f"{name} state {i}: contact / row counts"
        _abs_close(name, "xpos", G["xpos"][i].reshape(-1, 3), a["xpos"], 2e-5)
        _abs_close(name, "xquat", np.abs(G["xquat"][i].reshape(-1, 4)), np.abs(a["xquat"]), 2e-5)
        for f in ("qfrc_bias", "qfrc_passive", "qfrc_actuator"):
            _close(name, f, G[f][i], a[f], 2e-5)
        for f in ("qacc_smooth", "qacc", "qfrc_constraint"):
            _close(name, f, G[f][i], a[f], 2e-3)
    return d, G


# ------------------------------------------------------------------------------------------------
# forward, step, trajectory
# ------------------------------------------------------------------------------------------------
def test_instantiation_taken():
    """Every model takes the instantiation it is meant to take, by the library's own answer."""
    for name in ALL:
        m, sys_ = system(name)
        assert _uses_generic(mjx.make_data(sys_, 1)) == gm.MODELS[name][1] == gm.is_generic(m), name


@pytest.mark.parametrize("name", ALL)
def test_forward_parity(name):
    m, sys_ = system(name)
    states = states_of(name)
    _, G = _forward_check(name, m, sys_, states)
    if name in ("tail", "tail_euler", "nv_only", "ngeom_only", "full"):
        assert G["stats"][:, 0].max() > 0, "no state of the model has a contact"
    assert G["stats"][:, 1].max() > 0, "no state of the model has an active row"


@pytest.mark.parametrize("name", ALL)
def test_step_parity(name):
    m, sys_ = system(name)
    states = states_of(name)
    d = _load(sys_, states, m)
    mjx.step(sys_, d)
    q1, v1, w1, t1 = (d.get(f).cpu().numpy() for f in ("qpos", "qvel", "qacc_warmstart", "time"))
    orc = Oracle(m)
    for i, st in enumerate(states):
        a = state_arrays(m, orc.step(orc.new_state(*st)))
        _abs_close(name, "step qpos", q1[i], a["qpos"], 2e-5)
        _close(name, "step qvel", v1[i], a["qvel"], 2e-3)
        _close(name, "step qacc_warmstart", w1[i], a["qacc_warmstart"], 2e-3)
        assert t1[i] == pytest.approx(m.timestep, abs=1e-9)


@pytest.mark.parametrize("name", ALL)
def test_trajectory_parity(name):
    """20 chained steps with random controls from two of the falls: qpos within 1e-3 of the
    fp64 trajectory, every state on the way decided on the oracle.
    The sphere slabs start thrown at the floor instead (`thrown`)."""
    m, sys_ = system(name)
    T = 20
    for seed in range(200, 240):  # the first control sequence whose oracle trajectories stay decided
        rng = np.random.default_rng(seed)
        falls = states_of(name)[1:4]
        starts = [falls[seed % 3], falls[(seed + 1) % 3]]
        if name.startswith("ngeom"):  # (the slab at rest is no decided state)
            starts = thrown(m, rng)
        ctrl = np.float32(rng.uniform(-1, 1, (T, len(starts), max(m.nu, 1))))[:, :, :m.nu]
        orc, ok, ends = Oracle(m), True, []
        for i, st in enumerate(starts):
            s = orc.new_state(*st[:3])
            for t in range(T):
                a = state_arrays(m, s)
                ok = ok and decided(m, (a["qpos"], a["qvel"], a["qacc_warmstart"], ctrl[t, i].astype(np.float64)))
                orc.rollout(s, ctrl[t, i][None].astype(np.float64))
            ends.append(state_arrays(m, s)["qpos"])
        if ok:
            break
    assert ok, "no control sequence in 200..239 keeps the oracle trajectories decided"
    d = _load(sys_, starts, m)
    for t in range(T):
        mjx.step(sys_, d, torch.tensor(ctrl[t], device="cuda") if m.nu else None)
    q = d.get("qpos").cpu().numpy()
    for i in range(len(starts)):
        _abs_close(name, "trajectory qpos", q[i], ends[i], 1e-3)


# ------------------------------------------------------------------------------------------------
# solvers and integrators
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tail", "full"])
@pytest.mark.parametrize("solver", ["newton", "cg44"])
@pytest.mark.parametrize("integrator", ["euler_damp", "implicitfast"])
def test_solver_and_integrator_parity(name, solver, integrator):
    """Newton and CG 4/4 (tests/test_gpu_parity.py test_cg_solver_parity: against the fp32 oracle, since a line
    search cut at 4 iterations pins the zoom rules, qvel to 5e-3 * s) under Euler + eulerdamp and implicitfast.
    CG's qpos bound is that qvel bound integrated over one step, qpos' = qpos + dt qvel': dt * 5e-3 * (1 + max|qvel'|);
    Newton keeps the stated 2e-5. On these models (motors and joint damping only) Euler with eulerdamp and
    implicitfast both solve (M + dt D) v' = ..., so the two integrator cases differ in the code path taken
    (integrate's branches on the DGen dims), not in the numbers expected."""
    base = gm.MODELS[name][0]()
    kw = {"integrator": mjcf.INT_EULER, "eulerdamp": 1} if integrator == "euler_damp" else \
         {"integrator": mjcf.INT_IMPLICITFAST, "eulerdamp": 0}
    if solver == "cg44":
        kw.update(solver=mjcf.SOLVER_CG, iterations=4, ls_iterations=4)
    m = dataclasses.replace(base, **kw)
    sys_ = mjx.put_model(m)
    states = states_of(name)
    d = _load(sys_, states, m)
    assert _uses_generic(d)
    mjx.step(sys_, d)
    q1, v1 = (d.get(f).cpu().numpy() for f in ("qpos", "qvel"))
    orc = Oracle(m, use_float=solver == "cg44")
    tag = f"{solver} {integrator}"
    for i, st in enumerate(states):
        a = state_arrays(m, orc.step(orc.new_state(*st)))
        _close(name, tag + " qvel", v1[i], a["qvel"], 5e-3 if solver == "cg44" else 2e-3)
        _abs_close(name, tag + " qpos", q1[i], a["qpos"], 5e-3 * m.timestep * (1 + np.abs(a["qvel"]).max())
                   if solver == "cg44" else 2e-5)


# ------------------------------------------------------------------------------------------------
# row storage: LDS (32 rows), global, and the overflow between them
# ------------------------------------------------------------------------------------------------
def _lying(m):
    """`full` with its torso lowered to the floor, limbs flat: every limb body rests on the plane."""
    q = m.qpos0.copy()
    q[2] = 0.06
    return _f32(q, np.zeros(m.nv), np.zeros(m.nv), np.zeros(m.nu))


@pytest.mark.parametrize("name", ["tail", "full"])
def test_global_row_storage_matches_lds(name):
    m, sys_ = system(name)
    states = states_of(name) + ([_lying(m)] if name == "full" else [])
    res = []
    for force in (0, 1):
        d = _load(sys_, states, m)
        d.set_option(abi.OPT_FORCE_GLOBAL_ROWS, force)
        mjx.step(sys_, d)
        res.append([d.get(f).cpu().numpy() for f in ("qpos", "qvel", "qacc", "qfrc_constraint", "stats")])
    for a, b in zip(*res):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("name", ["ngeom_only", "full"])
def test_rows_do_not_depend_on_stale_memory(name):
    """A contact row's pad columns 32..35 (LD = 36) are written: the row dots run over all LD entries, and a NaN
    left there by an earlier allocation (an int -1 is one) silently switches the row off (jar < 0 is false). Device
    memory is filled with NaN and freed before the batch is created, rows forced into the global slab: the result
    is the one from before, bit for bit, and the oracle's (2e-3 * s on qacc). Best effort: nothing guarantees
    that the library's allocation lands on the freed, poisoned pages."""
    m, sys_ = system(name)
    states = states_of(name)
    res = []
    for poison in (False, True):
        if poison:
            junk = [torch.full((n,), float("nan"), device="cuda") for n in (1 << 10, 1 << 14, 1 << 18, 1 << 22, 1 << 24)
                    for _ in range(4)]
            torch.cuda.synchronize()
            del junk
            torch.cuda.empty_cache()
        d = _load(sys_, states, m)
        d.set_option(abi.OPT_FORCE_GLOBAL_ROWS, 1)
        mjx.forward(sys_, d)
        res.append([d.get(f).cpu().numpy() for f in ("qacc", "qfrc_constraint", "stats")])
    for a, b in zip(*res):
        np.testing.assert_array_equal(a, b)
    orc = Oracle(m)
    for i, st in enumerate(states):
        a = state_arrays(m, orc.forward(orc.new_state(*st)))
        _close(name, "poisoned qacc", res[1][0][i], a["qacc"], 2e-3)


def test_overflow_state_parity_and_kkt():
    """`full` lying on the floor: more active rows than the 32 the generic instantiation keeps in LDS, and more
    contacts than its 16, so the rows overflow into the env's global slab. Parity with the oracle at the forward
    tolerances, and the optimality condition M (qacc - qacc_smooth) = qfrc_constraint with the compiler's numpy
    mass matrix (tests/test_kat_gpu.py), 2e-3 * (1 + max|lhs|)."""
    m, sys_ = system("full")
    st = _lying(m)
    _, G = _forward_check("full/lying", m, sys_, [st])
    assert G["stats"][0][1] > 32 and G["stats"][0][0] > 16
    M = mjcf._fk_and_mass(m, st[0])["M"]
    lhs = M @ (G["qacc"][0].astype(np.float64) - G["qacc_smooth"][0])
    _abs_close("full/lying", "kkt", lhs, G["qfrc_constraint"][0].astype(np.float64), 2e-3 * (1 + np.abs(lhs).max()))


# ------------------------------------------------------------------------------------------------
# known answers that do not come from the oracle
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tail", "full", "nv_only", "nbody_only"])
def test_gravity_bias_and_fk_kat(name):
    """tests/test_kat_gpu.py's check: qvel = 0, qfrc_bias = sum_b -J_b(xipos_b)' m_b g from numpy Jacobians,
    2e-5 * (1 + max|expected|); xpos = the numpy forward kinematics, 2e-5."""
    m, sys_ = system(name)
    rng = np.random.default_rng(1)
    qs = []
    for _ in range(4):
        q = m.qpos0.copy()
        for j in range(m.njnt):
            a = int(m.jnt_qposadr[j])
            if m.jnt_type[j] == mjcf.JNT_FREE:
                q[a + 3:a + 7] = rng.normal(size=4)
                q[a + 3:a + 7] /= np.linalg.norm(q[a + 3:a + 7])
            else:
                q[a] += rng.uniform(-0.5, 0.5)
        qs.append(np.float32(q).astype(np.float64))
    d = mjx.make_data(sys_, len(qs))
    d.set("qpos", torch.tensor(np.array(qs), dtype=torch.float32))
    mjx.forward(sys_, d)
    bias = d.get("qfrc_bias").cpu().numpy().astype(np.float64)
    xpos = d.get("xpos").cpu().numpy().astype(np.float64).reshape(len(qs), m.nbody, 3)
    for i, q in enumerate(qs):
        kin = mjcf._fk_and_mass(m, q)
        expect = np.zeros(m.nv)
        for b in range(1, m.nbody):
            jp, _ = mjcf.body_jacobian(m, kin, b, kin["xipos"][b])
            expect -= jp.T @ (m.body_mass[b] * m.gravity)
        _abs_close(name, "kat qfrc_bias", bias[i], expect, 2e-5 * (1 + np.abs(expect).max()))
        _abs_close(name, "kat xpos", xpos[i], kin["xpos"], 2e-5)


@pytest.mark.parametrize("name", ["tail", "full"])
def test_solver_optimality_kat(name):
    """M (qacc - qacc_smooth) = qfrc_constraint with the compiler's numpy M on the parity states,
    2e-3 * (1 + max|lhs|) (tests/test_kat_gpu.py)."""
    m, sys_ = system(name)
    states = states_of(name)
    d = _load(sys_, states, m)
    mjx.forward(sys_, d)
    qacc, qsm, qfc = (d.get(f).cpu().numpy().astype(np.float64) for f in ("qacc", "qacc_smooth", "qfrc_constraint"))
    assert (d.get("stats").cpu().numpy()[:, 1] > 0).sum() >= 3
    for i, st in enumerate(states):
        lhs = mjcf._fk_and_mass(m, st[0])["M"] @ (qacc[i] - qsm[i])
        _abs_close(name, "kat kkt", lhs, qfc[i], 2e-3 * (1 + np.abs(lhs).max()))


# ------------------------------------------------------------------------------------------------
# batch edges
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tail", "full"])
def test_batch_sizes_mask_and_nan_isolation(name):
    """Batches of 1, 3 and 65 envs of the same states give each env the same bits; a masked forward leaves the
    envs outside the mask untouched; a NaN env stays alone in being non-finite and the others are bit-identical
    (the flag is the env step's: test_nan_env_is_flagged_and_isolated_on_tail)."""
    m, sys_ = system(name)
    base = states_of(name)
    big = [base[i % len(base)] for i in range(65)]
    out = {}
    for B in (1, 3, 65):
        d = _load(sys_, big[:B], m)
        mjx.step(sys_, d)
        out[B] = [d.get(f).cpu().numpy() for f in ("qpos", "qvel", "qacc")]
    for B in (1, 3):
        for a, b in zip(out[B], out[65]):
            np.testing.assert_array_equal(a, b[:B])
    for a in out[65]:
        np.testing.assert_array_equal(a[:len(base)], a[len(base):2 * len(base)])
        assert np.isfinite(a).all()
    # masked forward
    d = _load(sys_, base, m)
    mask = torch.tensor([1.0, 0.0] * 3, device="cuda")[:len(base)]
    before = d.get("qacc").cpu().numpy().copy()
    mjx.forward(sys_, d, mask)
    after = d.get("qacc").cpu().numpy()
    full_ = _load(sys_, base, m)
    mjx.forward(sys_, full_)
    ref = full_.get("qacc").cpu().numpy()
    np.testing.assert_array_equal(after[1::2], before[1::2])
    np.testing.assert_array_equal(after[0::2], ref[0::2])
    # a NaN env
    bad = 2
    d1, d2 = _load(sys_, base, m), _load(sys_, base, m)
    qv = d1.get("qvel").clone()
    qv[bad, 0] = float("nan")
    d1.set("qvel", qv)
    mjx.step(sys_, d1)
    mjx.step(sys_, d2)
    assert not torch.isfinite(d1.get("qvel")[bad]).all()
    keep = [i for i in range(len(base)) if i != bad]
    for f in ("qpos", "qvel", "qacc"):
        assert torch.equal(d1.get(f)[keep], d2.get(f)[keep])


# ------------------------------------------------------------------------------------------------
# readouts
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tail", "full", "ngeom_only"])
def test_forward_contacts_readout(name):
    """contacts_kernel<DGen>: the contact list of mjx.forward_contacts is the oracle's, as a set (geoms exact;
    dist, pos 2e-5; normal 2e-5), the two contacts of a plane-capsule pair matched by nearest position."""
    m, sys_ = system(name)
    states = states_of(name) + ([_lying(m)] if name == "full" else [])
    d = _load(sys_, states, m)
    c = mjx.forward_contacts(sys_, d)
    ncon, geom, dist, pos, frame = (x.cpu().numpy() for x in (c.ncon, c.geom, c.dist, c.pos, c.frame))
    orc = Oracle(m)
    total = 0
    for i, st in enumerate(states):
        a = state_arrays(m, orc.forward(orc.new_state(*st)))
        assert ncon[i] == a["ncon"]
        left = list(range(a["ncon"]))  # each oracle contact takes the nearest unused GPU contact of its geom pair
        for w in range(a["ncon"]):
            same = [g for g in left if tuple(geom[i][g]) == tuple(a["con_geom"][w])]
            assert same, f"{name} state {i}: no contact of geoms {tuple(a['con_geom'][w])}"
            g = min(same, key=lambda k: np.abs(pos[i][k] - a["con_pos"][w]).max())
            left.remove(g)
            _abs_close(name, "contact dist", dist[i][g], a["con_dist"][w], 2e-5)
            _abs_close(name, "contact pos", pos[i][g], a["con_pos"][w], 2e-5)
            _abs_close(name, "contact normal", frame[i][g][0], a["con_frame"][w][:3], 2e-5)
        total += a["ncon"]
    assert total > 0


def test_body_data_cfrc_on_full():
    """body_data_kernel<DGen> with more than 17 bodies (the serial subtree loop): cfrc_int, cfrc_ext, subtree_com
    and cvel against tests/bodydata_ref.py on the oracle's forward outputs. cfrc values inherit the forward's
    qacc / efc_force error: 2e-3 * (1 + max|ref|); subtree_com 2e-5; cvel 2e-5 * (1 + max|ref|)."""
    m, sys_ = system("full")
    states = states_of("full") + [_lying(m)]
    d = _load(sys_, states, m)
    bd = mjx.body_data(sys_, d, fields=("subtree_com", "cvel", "cfrc_ext", "cfrc_int"))
    orc = Oracle(m)
    for i, st in enumerate(states):
        o = state_arrays(m, orc.forward(orc.new_state(*st)))
        ref = br.body_data(m, o)
        _abs_close("full", "body subtree_com", bd.subtree_com[i].cpu().numpy(), ref["subtree_com"], 2e-5)
        _close("full", "body cvel", bd.cvel[i].cpu().numpy(), ref["cvel"], 2e-5)
        _close("full", "body cfrc_ext", bd.cfrc_ext[i].cpu().numpy(), ref["cfrc_ext"], 2e-3)
        _close("full", "body cfrc_int", bd.cfrc_int[i].cpu().numpy(), ref["cfrc_int"], 2e-3)


@pytest.mark.parametrize("name", ["full", "tail"])
def test_applied_forces(name):
    """The applied instantiation on DGen, an xfrc_applied wrench on a body of index > 17 and a qfrc_applied:
    qacc_smooth moves by M^-1 (qfrc_applied + sum_b J_b(xipos_b)' [f_b; t_b]) with the compiler's numpy M and
    Jacobians, on top of the oracle's qacc_smooth: 2e-3 * s. (tests/applied_ref.py restates only the push rule
    of mjl_env_push, its timers and draws; it has no reference for the forces' effect on the dynamics, and the
    oracle takes no applied forces, hence this one.) The wrench moves qacc_smooth by more than 100 x that bound
    in every state, so a kernel that dropped part of it cannot pass."""
    m, sys_ = system(name)
    states = states_of(name)
    B = len(states)
    rng = np.random.default_rng(3)
    bodies = sorted({m.nbody - 1, 18, 3})
    xfrc = np.zeros((B, m.nbody, 6), np.float32)
    for b in bodies:
        xfrc[:, b] = rng.uniform(20, 60, (B, 6)) * rng.choice([-1.0, 1.0], (B, 6))
    qfrc = np.float32(rng.uniform(-1, 1, (B, m.nv)))
    d = _load(sys_, states, m)
    d.attach_applied(torch.tensor(qfrc, device="cuda"), torch.tensor(xfrc, device="cuda"))
    mjx.forward(sys_, d)
    got = d.get("qacc_smooth").cpu().numpy()
    orc = Oracle(m)
    for i, st in enumerate(states):
        a = state_arrays(m, orc.forward(orc.new_state(*st)))
        kin = mjcf._fk_and_mass(m, st[0])
        gen = qfrc[i].astype(np.float64)
        for b in bodies:
            jp, jr = mjcf.body_jacobian(m, kin, b, kin["xipos"][b])
            gen = gen + jp.T @ xfrc[i, b, :3].astype(np.float64) + jr.T @ xfrc[i, b, 3:].astype(np.float64)
        want = a["qacc_smooth"] + np.linalg.solve(kin["M"], gen)
        assert np.abs(want - a["qacc_smooth"]).max() > 100 * 2e-3 * (1 + np.abs(a["qacc_smooth"]).max())
        _close(name, "applied qacc_smooth", got[i], want, 2e-3)


def test_sensors_readout_on_tail():
    """mjx.sensors on `tail` with an IMU site on body 19 and a few sensors of each stage, against
    tests/sensors_ref.py on the oracle's forward outputs, with tests/test_sensors_gpu.py's rule for the bounds
    (8 x the float32-vs-float64 yardstick of the reference on these states, plus the forward's inherited
    tolerance for the acc-stage values) and its accelerometer check on the stored qacc."""
    import test_sensors_gpu as ts
    m = gm.tail_sensors()
    sys_ = mjx.put_model(m)
    states = states_of("tail")[:4]   # the same bodies, joints and geoms as `tail`
    jn = m.names["joint"]
    q, v, w, c = (x.copy() for x in states[1])   # a fall again, two sensed joints held past their range
    for j, side, push in (("tail1", 1, 1.0), ("knee_left", 0, -1.0)):
        k = jn.index(j)
        q[int(m.jnt_qposadr[k])] = m.jnt_range[k][side] + (0.05 if side else -0.05)
        v[int(m.jnt_dofadr[k])] = 0.0
        c[m.names["actuator"].index(j)] = push
    states = states + [_f32(q, 0.5 * v, w, c)]
    for i, st in enumerate(states):
        assert_decided(m, st, f"tail_sensors state {i}")
    outs, r64, r32 = ts.reference(m, states)
    tol, inh = ts.tolerances(m, states, outs, r64, r32)
    T = mjcf.SENSOR_TYPES
    sl = {n: m.sensor_slice(n) for n in m.names["sensor"]}
    assert abs(r64[4, sl["jl_tail1"]][0]) > 1.0  # the tail's forced limit carries force
    assert np.abs(r64[:, sl["touch_foot_left"]]).max() + np.abs(r64[:, sl["touch_foot_right"]]).max() > 0
    d = _load(sys_, states, m)
    assert _uses_generic(d)
    got = mjx.sensors(sys_, d).cpu().numpy()
    ts._check_rows(m, got, r64, tol, inh, range(len(states)), "tail_sensors")
    ts.accel_on_stored_qacc(m, states, outs, got, d.get("qacc").cpu().numpy(), tol, "tail_sensors")
    for s_, (sname, t, slc) in enumerate(ts._slots(m)):
        if t != T["framequat"]:
            for e in range(len(states)):
                _note("tail", f"sensor {sname}", np.abs(got[e, slc] - r64[e, slc]).max(), tol[t]["bound"] + inh[e][s_])


def _substituted(m, params, i):
    """tests/model_params_ref.py's `substituted` for a model that is not a built-in one: env i's float32 values in
    the descriptor fields, nothing else recomputed."""
    from mjx_amd.randomize import FIELDS
    A = {k: np.array(v, copy=True) for k, v in m.arrays.items()}
    for k in FIELDS:
        v = np.asarray(params[k][i], np.float32).astype(np.float64)
        if k == "pair_friction":
            A[k] = np.array(A[k], np.float64).reshape(-1, 5)
            A[k][:, 0] = A[k][:, 1] = v
        else:
            A[k] = v.reshape(np.shape(A[k]))
    return dataclasses.replace(m, arrays=A)


@pytest.mark.parametrize("name", ["full", "tail"])
def test_per_env_model_params(name):
    """The per-env instantiation on DGen: d.set_model_params with tests/model_params_ref.py's draw (every env its
    own masses, inertias, damping, armature, gear and friction; one env without damping). Env i of the batch
    against the fp64 oracle on the model with env i's values substituted, forward and one step, at the stated
    tolerances (tests/test_model_params_gpu.py test_against_the_fp64_oracle)."""
    import model_params_ref as mpr
    m, sys_ = system(name)
    states = states_of(name)
    B = len(states)
    p = mpr.draw(m, B)
    d = _load(sys_, states, m)
    d.enable_model_params()
    d.set_model_params(**{k: torch.tensor(v, device="cuda") for k, v in p.items()})
    mjx.forward(sys_, d)
    G = {f: d.get(f).cpu().numpy() for f in FWD}
    d2 = _load(sys_, states, m)
    d2.enable_model_params()
    d2.set_model_params(**{k: torch.tensor(v, device="cuda") for k, v in p.items()})
    mjx.step(sys_, d2)
    q1, v1 = (d2.get(f).cpu().numpy() for f in ("qpos", "qvel"))
    plain = _load(sys_, states, m)
    mjx.forward(sys_, plain)
    assert np.abs(G["qacc"] - plain.get("qacc").cpu().numpy()).max() > 0.1  # the values reach the dynamics
    tag = "per-env "
    for i, st in enumerate(states):
        sub = _substituted(m, p, i)
        assert_decided(sub, st, f"{name} env {i}")
        orc = Oracle(sub)
        a = state_arrays(sub, orc.forward(orc.new_state(*st)))
        assert (G["stats"][i][0], G["stats"][i][1]) == (a["ncon"], a["nefc"]), f"{name} env {i}: counts"
        for f in ("qfrc_bias", "qfrc_passive", "qfrc_actuator"):
            _close(name, tag + f, G[f][i], a[f], 2e-5)
        for f in ("qacc_smooth", "qacc", "qfrc_constraint"):
            _close(name, tag + f, G[f][i], a[f], 2e-3)
        a = state_arrays(sub, orc.step(orc.new_state(*st)))
        _abs_close(name, tag + "step qpos", q1[i], a["qpos"], 2e-5)
        _close(name, tag + "step qvel", v1[i], a["qvel"], 2e-3)


def test_rays_on_full():
    """mjx.ray on `full` (32 geoms: the ray path past the humanoid's 20) against tests/rays_ref.py, with
    tests/test_rays_gpu.py's comparison: geomid exact and dist within profiles/rays/tolerances.json on the
    non-marginal rays. 3 poses, 70 rays each (more than one wavefront): one straight down beside the root, one up,
    the rest from a 1.5 m box around the root towards random bodies; all geoms, then without the static floor."""
    import render_ref as rr
    import rays_ref as rf
    from test_rays_gpu import _tol, compare
    m, sys_ = system("full")
    Q = np.array([st[0] for st in states_of("full")[:3]])
    rng = np.random.default_rng(9)
    nray = 70
    P, V = np.zeros((len(Q), nray, 3)), np.zeros((len(Q), nray, 3))
    for e, q in enumerate(Q):
        xpos = mjcf._fk_and_mass(m, q)["xpos"]
        P[e] = q[:3] + rng.uniform(-0.75, 0.75, (nray, 3)) + [0, 0, 0.8]
        tgt = xpos[rng.integers(1, m.nbody, nray)] + rng.uniform(-0.03, 0.03, (nray, 3))
        V[e] = tgt - P[e]
        P[e, 0], V[e, 0] = q[:3] + [1.0, 0.3, 0.5], [0, 0, -1.0]
        V[e, 1] = [0, 0, 1.0]
        V[e] /= np.linalg.norm(V[e], axis=1, keepdims=True)
    P, V = np.float32(P).astype(np.float64), np.float32(V).astype(np.float64)
    d = mjx.make_data(sys_, len(Q))
    d.set("qpos", torch.tensor(Q, dtype=torch.float32))
    t = lambda x: torch.tensor(x, dtype=torch.float32, device="cuda")
    seen = set()
    for label, kw in (("all", {}), ("nostatic", {"flg_static": False})):
        dist, gid = mjx.ray(sys_, d, t(P), t(V), **kw)
        dist, gid = dist.cpu().numpy(), gid.cpu().numpy()
        for e in range(len(Q)):
            dref, gref, keep = compare(m, f"full {label} env {e}", Q[e], P[e], V[e], kw, dist[e], gid[e], None, _tol())
            assert keep.mean() >= 0.9
            seen |= set(gref[keep].tolist())
            if label == "all":
                assert gid[e, 0] == 0 and gid[e, 1] == -1
    assert len({g for g in seen if g > 20}) >= 3, "no ray hits a geom past the humanoid's 20"



# ------------------------------------------------------------------------------------------------
# env step and record
# ------------------------------------------------------------------------------------------------
def _env(B, seed=3):
    m = gm.tail()
    sys_ = mjx.put_model(m)
    cfg = resolve_ids(m, reference_ppo_config().env_config)
    env = HumanoidEnv(sys_, cfg, B, seed=seed, store_derived=True)
    return m, env, abi.env_config_c(cfg, m, env.obs_dim)


def test_env_step_parity_on_tail():
    """mjl_env_step on `tail` with the reference env config resolved on it, 3 steps of 2 envs against the oracle
    env: test_env_step_parity's tolerances (reward, obs 5e-3 relative; flags and counts exact). The reset stands
    the humanoid with its feet within 1e-4 of the floor's activation distance, which is no decided state, so
    every root is lowered by 4 mm after the reset (feet in the floor); the noise / action seed is the first
    whose oracle trajectories stay decided, and the compared trajectories, which start from the GPU's own
    float32 reset state, are asserted to be."""
    B, T, DROP = 2, 3, 0.004
    m, env, cfg_c = _env(B)
    nq, nv = m.nq, m.nv
    nd = nq - 7 + nv + 2
    orc = Oracle(m)

    def run(ost, acts, check):
        ref = []
        for t in range(T):
            row = []
            for i in range(B):
                a = state_arrays(m, ost[i][0])
                st = (a["qpos"], a["qvel"], a["qacc_warmstart"], np.clip(acts[t, i].astype(np.float64), -1, 1))
                if not check(st, t, i):
                    return None
                s, oa, oo, r, te, tr = orc.env_step(cfg_c, ost[i][0], ost[i][1], acts[t, i].astype(np.float64))
                ost[i] = [s, oa]
                sa = state_arrays(m, s)
                row.append((oa, oo, r, te, tr, sa["ncon"], sa["nefc"]))
            ref.append(row)
        return ref

    for seed in range(300, 340):
        rng = np.random.default_rng(seed)
        noise = rng.uniform(0, 1, (B, nd)).astype(np.float32)
        acts = rng.uniform(-1.2, 1.2, (T, B, m.nu)).astype(np.float32)
        ost = [list(orc.env_reset(cfg_c, noise[i].astype(np.float64))[:2]) for i in range(B)]
        for o in ost:
            o[0].qpos[2] -= DROP
        if run(ost, acts, lambda st, t, i: decided(m, st)) is not None:
            break
    else:
        raise AssertionError("no seed in 300..339 keeps the oracle env trajectories decided")
    env.reset(noise=torch.tensor(noise))
    state = env.get_state().clone()
    state[:, 2] -= DROP
    env.set_state(state)
    st0 = env.get_state().cpu().numpy().astype(np.float64)
    ost = [[orc.new_state(r[:nq], r[nq:nq + nv], r[nq + nv:nq + 2 * nv], time=r[-1]),
            r[nq + 2 * nv:nq + 2 * nv + abi.AUX_DIM].copy()] for r in st0]

    def must(st, t, i):
        assert_decided(m, st, f"step {t} env {i}")
        return True
    ref = run(ost, acts, must)
    for t in range(T):
        obs, rew, term, trunc = (x.cpu().numpy() for x in env.step(torch.tensor(acts[t]), auto_reset=False))
        aux, st = env.aux.cpu().numpy(), env.data.get("stats").cpu().numpy()
        for i in range(B):
            oa, oo, r, te, tr, ncon, nefc = ref[t][i]
            assert (te, tr) == (term[i], trunc[i]) and (aux[i][[0, 4, 5, 8]] == oa[[0, 4, 5, 8]]).all()
            assert (st[i][0], st[i][1]) == (ncon, nefc), f"step {t} env {i}: counts"
            assert ncon > 0
            _abs_close("tail", "env reward", rew[i], r, 5e-3 * (1 + abs(r)))
            _abs_close("tail", "env obs", obs[i], oo[:obs.shape[1]], 5e-3 * (1 + np.abs(oo).max()))


def test_nan_env_is_flagged_and_isolated_on_tail():
    """tests/test_gpu_parity.py test_non_finite_env_is_flagged_and_isolated on `tail`'s env step."""
    B, bad = 8, 3
    m, env, _ = _env(B, seed=5)
    _, env2, _ = _env(B, seed=5)
    env.reset()
    env2.set_state(env.get_state())
    qv = env.data.get("qvel").clone()
    qv[bad, 0] = float("nan")
    env.data.set("qvel", qv)
    act = torch.zeros((B, m.nu), device="cuda")
    r1 = [x.clone() for x in env.step(act, auto_reset=False)]
    r2 = [x.clone() for x in env2.step(act, auto_reset=False)]
    flags = env.data.get("stats")[:, 3].cpu().numpy()
    assert flags[bad] == 1.0 and (np.delete(flags, bad) == 0.0).all()
    assert (env2.data.get("stats")[:, 3] == 0).all()
    keep = [i for i in range(B) if i != bad]
    for x, y in list(zip(r1, r2)) + [(env.data.get("qpos"), env2.data.get("qpos"))]:
        assert torch.equal(x[keep], y[keep])


@pytest.mark.parametrize("solver,vjp", [("model", "implicit"), ("cg44", "unrolled")])
def test_record_equals_env_step_and_replay_equals_recompute(solver, vjp):
    """tests/test_vjp_tape.py on the DGen tape layout: over 6 steps of 16 envs of `tail` the recorded step is
    the env step bit for bit, and the replayed VJP's cotangents are the recomputing VJP's bit for bit.
    The unrolled CG 4/4 values have no independent reference on these dims: tests/unrolled_solver_ref.py restates
    the solver's reverse sweep for the humanoid tests' fixed inputs, and only the implicit VJP is compared with
    the oracle's dual-number Jacobian (test_step_vjp_matches_dual_jacobian); replay against recompute would
    pass if both were wrong alike.
    (Before build_rows wrote a contact row's pad columns this was not stable: the record keeps its rows in the
    tape slot's global slab, whose stale content reached the row dots.)"""
    m = dataclasses.replace(gm.tail())
    if solver == "cg44":
        m = dataclasses.replace(m, solver=mjcf.SOLVER_CG, iterations=4, ls_iterations=4)
    ecfg = resolve_ids(m, reference_ppo_config().env_config)
    B, H = 16, 6
    plain, taped = (apg.HumanoidAPGEnv(HumanoidEnv(mjx.put_model(m), ecfg, B, seed=9), vjp) for _ in range(2))
    assert _uses_generic(plain.env.data)
    taped.enable_vjp_tape(H)
    for e in (plain, taped):
        e.reset()
    g = torch.Generator(device="cuda").manual_seed(1)
    acts, pre = [], []
    for t in range(H):
        a = torch.rand((B, m.nu), generator=g, device="cuda") * 2 - 1
        acts.append(a)
        pre.append(plain.get_state())
        o1 = [x.clone() for x in plain.step(a)]
        o2 = [x.clone() for x in taped.step_record(t, a)]
        for x, y, k in zip(o1, o2, ("obs", "rew", "term", "trunc")):
            assert torch.equal(x, y), f"step {t}: {k}"
        for f in ("qpos", "qvel", "qacc_warmstart", "ctrl", "time", "aux"):
            assert torch.equal(plain.env.data.get(f), taped.env.data.get(f)), f"step {t}: {f}"
    gws_on = vjp == "unrolled"
    for t in range(H - 1, -1, -1):
        gq = torch.randn((B, m.nq), generator=g, device="cuda")
        gv = torch.randn((B, m.nv), generator=g, device="cuda")
        gw = torch.randn((B, m.nv), generator=g, device="cuda") if gws_on else None
        gr = torch.randn(B, generator=g, device="cuda")
        gx = torch.randn((B, abi.AUX_DIM), generator=g, device="cuda")
        plain.env.set_state(pre[t])
        if gws_on:
            r1 = plain.step_vjp_full(acts[t], gq, gv, gw, gr, gx)
        else:
            oq, ov, oa, ox = plain.step_vjp(acts[t], gq, gv, gr, gx)
            r1 = (oq, ov, None, oa, ox)
        r2 = taped.step_vjp_replay(t, acts[t], gq, gv, gw, gr, gx)
        for x, y, k in zip(r1, r2, ("qpos", "qvel", "ws", "act", "aux")):
            if x is None:
                assert y is None
                continue
            assert torch.isfinite(x).all()
            assert torch.equal(x, y), f"step {t}: {k} cotangent ({(x - y).abs().max().item():.3g})"


def test_step_vjp_matches_dual_jacobian():
    """vjp_kernel<DGen>: mjx.step_vjp on `tail` against the oracle's dual-number step Jacobian, exactly as
    tests/test_adjoint.py's test_step_vjp_matches_dual_jacobian: max|got - ref| / (max|ref| + scale) <= 2e-3 with
    scale = 1e-3 max|u| max|J|."""
    m, sys_ = system("tail")
    states = states_of("tail")[:4]
    nq, nv = m.nq, m.nv
    rng = np.random.default_rng(5)
    gq = np.float32(rng.normal(size=(len(states), nq)))
    gv = np.float32(rng.normal(size=(len(states), nv)))
    d = _load(sys_, states, m)
    got = [x.cpu().numpy().astype(np.float64) for x in mjx.step_vjp(sys_, d, torch.tensor(gq), torch.tensor(gv))]
    orc = Oracle(m)
    for i, st in enumerate(states):
        J = orc.step_jacobian(orc.new_state(*st))
        u = np.concatenate([gq[i], gv[i]]).astype(np.float64)
        ref = u @ J
        scale = 1e-3 * np.abs(u).max() * np.abs(J).max()
        for k, (lo, hi, what) in enumerate(((0, nq, "vjp qpos"), (nq, nq + nv, "vjp qvel"), (nq + nv, len(ref), "vjp ctrl"))):
            err = np.abs(got[k][i] - ref[lo:hi]).max() / (np.abs(ref[lo:hi]).max() + scale)
            _note("tail", what, err, 2e-3)
            assert err <= 2e-3, f"state {i} {what}: relative VJP error {err:.3e}"
