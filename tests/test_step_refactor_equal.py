"""The env step's shared pieces, on the two paths the other suites reach only by chance: the action
flip / clip of the step prologue across mjl_env_step and mjl_env_step_record (src/envs.py:335-344), and
every MJL_FIELD_* entry of the batch's and the reset pool's field tables through one pooled reset."""
import dataclasses

import pytest
import torch

import mjx_amd
from mjx_amd import abi, apg, mjx
from mjx_amd._lib import check, lib
from mjx_amd.config import reference_ppo_config
from mjx_amd.envs import HumanoidEnv, resolve_ids
from mjx_amd.mjx import _ptr, _stream

pytestmark = pytest.mark.gpu

STATE = ("qpos", "qvel", "qacc_warmstart", "ctrl", "time", "aux")


def test_step_and_record_agree_with_flip_on_off_and_clip():
    """3 envs of humanoid_mjx over 4 steps, env step against the implicit record: env 0 at the reset
    pose (model qpos0, at rest, flip off), env 1 with aux[0] = 1 (its action flipped), env 2 with two
    action components outside [-1, 1] (clipped). Outputs and the six state fields are equal bit for
    bit; the stored ctrl shows that the flip and the clip were in fact taken."""
    m = mjx_amd.load_model("humanoid_mjx")
    ecfg = resolve_ids(m, reference_ppo_config().env_config)
    B, H = 3, 4
    plain, taped = (apg.HumanoidAPGEnv(HumanoidEnv(mjx.put_model(m), ecfg, B, seed=9), "implicit") for _ in range(2))
    taped.enable_vjp_tape(H)
    for e in (plain, taped):
        e.reset()
    st = plain.get_state()  # [qpos | qvel | qacc_warmstart | aux | time]
    nq, nv = m.nq, m.nv
    st[0, :nq] = torch.tensor(m.qpos0, dtype=torch.float32, device="cuda")
    st[0, nq:nq + 2 * nv] = 0.0
    st[:, nq + 2 * nv] = torch.tensor([0.0, 1.0, 0.0], device="cuda")  # aux[0]: the flip
    for e in (plain, taped):
        e.env.set_state(st)
    g = torch.Generator(device="cuda").manual_seed(4)
    for t in range(H):
        a = torch.rand((B, m.nu), generator=g, device="cuda") * 2 - 1
        a[2, 0], a[2, m.nu - 1] = 1.7, -2.3
        o1 = [x.clone() for x in plain.step(a)]
        o2 = [x.clone() for x in taped.step_record(t, a)]
        for x, y, k in zip(o1, o2, ("obs", "rew", "term", "trunc")):
            assert torch.equal(x, y), f"step {t}: {k}"
        for f in STATE:
            assert torch.equal(plain.env.data.get(f), taped.env.data.get(f)), f"step {t}: {f}"
        ctrl, clipped = plain.env.data.get("ctrl"), a.clamp(-1, 1)
        assert torch.equal(ctrl[0], clipped[0]) and torch.equal(ctrl[2], clipped[2])
        assert not torch.equal(ctrl[1], clipped[1]), "env 1's action was not flipped"
        assert torch.equal(plain.env.aux[:, 0], st[:, nq + 2 * nv])


def test_pooled_reset_round_trip_covers_every_field():
    """2 envs, 2 pooled slots, max_episode_steps 1 (every step finishes), derived fields stored: after
    each merging step all 16 MJL_FIELD_* fields equal those of mjl_env_reset at the slot's counter on a
    second batch (stats: its first three columns -- the fourth is the step's NaN flag on one side and
    the reset's active-row count on the other)."""
    m = mjx_amd.load_model("humanoid_mjx")
    cfg = resolve_ids(m, dataclasses.replace(reference_ppo_config().env_config, max_episode_steps=1))
    B, slots = 2, 2
    env, ref = (HumanoidEnv(mjx.put_model(m), cfg, B, seed=5, store_derived=True) for _ in range(2))
    env.enable_reset_pool(slots)
    env.reset()
    c0 = env.counter
    env.fill_reset_pool(torch.tensor([slots], dtype=torch.int32, device="cuda"))
    act = torch.zeros((B, m.nu), device="cuda")
    assert len(abi.FIELD) == 16
    for j in range(slots):
        obs, _, term, trunc = (x.clone() for x in env.step(act))
        assert bool(torch.all(torch.maximum(term, trunc) == 1))
        counter = ((c0 + (j << 48)) % (1 << 64)) ^ (1 << 63)  # the pool's counter domain, slot in bits 48..55
        check(lib().mjl_env_reset(ref.data.handle, None, ref.seed, counter, None, _ptr(ref.obs), _stream()))
        assert torch.equal(obs, ref.obs), f"slot {j}: obs"
        for f in abi.FIELD:
            x, y = env.data.get(f), ref.data.get(f)
            if f == "stats":  # column 3: no NaN in the step; the reset's mean active rows per Newton Hessian
                assert bool(torch.all(x[:, 3] == 0)), f"slot {j}: stats[3] of the step"
                assert bool(torch.all((y[:, 3] >= 0) & (y[:, 3] <= y[:, 1]))), f"slot {j}: stats[3] of the reset"
                x, y = x[:, :3], y[:, :3]
            assert torch.equal(x, y), f"slot {j}: {f}"
