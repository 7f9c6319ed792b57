"""Exponent-carried cotangents in the APG reverse sweep (APGTrainer scale_cotangents, mjx_amd/apg.py
CotangentScale; CPU, differentiable stand-in envs, so the torch form of the rule the VJP kernel applies):
a forced rescale changes no bit of the gradient; a rollout whose chained step Jacobians leave fp32
range keeps every env and gives the fp64 gradient; the clip is unchanged where nothing is scaled;
data-parallel ranks stay identical through the exponent's MAX-reduce."""
import os

import torch
import torch.distributed as tdist
import torch.multiprocessing as mp

from mjx_amd import apg
from test_apg import DiffPointEnv, _cfg, _port


class PointEnvF32(DiffPointEnv):
    """DiffPointEnv in float32 (same step, reward and termination). Its resets start x and y six times
    wider, so the state cotangents (2 q disc / B per step) pass 1 within the horizon: an exponent only
    leaves 0 for a magnitude of 1 or more, whatever the threshold."""

    def reset(self):
        super().reset()
        self.q = (self.q * torch.tensor([6.0, 6.0, 1.0], dtype=torch.float64)).float()
        self.v = self.v.float()

    def step(self, act, auto_reset=False):
        self.q, self.v, r = self.f(self.q, self.v, act.float())
        term = (self.q[:, 2].abs() > 1.5).float()
        return None, r, term, torch.zeros_like(term)

    def step_vjp(self, act, gq, gv, grew, gaux, nonfinite=None):
        q = self.q.clone().requires_grad_(True)
        v = self.v.clone().requires_grad_(True)
        a = act.float().clone().requires_grad_(True)
        q2, v2, r = self.f(q, v, a)
        torch.autograd.backward([q2, v2, r], [gq.float(), gv.float(), grew.float()])
        return q.grad, v.grad, a.grad, None


GAIN, EPS = 16.0, 2.0 ** -60


class GainEnv:
    """float32 stand-in whose step multiplies the state by GAIN: q' = GAIN q + EPS (a0, a1, a0 - a1) from
    |q_0| <= EPS / 2, reward = sum(q) - 0.1 |a|^2, no termination; v, of order 1, turns by a fixed rotation
    (the policy's input differs from step to step and env to env while q is still ~EPS). The state stays in fp32 range over the horizon
    (|q_H| ~ EPS GAIN^H = 2^(4 H - 60)) and so does every action cotangent (EPS times the state cotangent),
    but the state cotangent itself, ~GAIN^(H - t) / B, leaves it once 4 (H - t) - 3 > 127."""

    dtype = torch.float32

    def __init__(self, num_envs, seed=0):
        self.num_envs, self.act_dim, self.nq, self.nv = num_envs, 2, 3, 3
        self.g = torch.Generator().manual_seed(seed)
        self.q = torch.zeros(num_envs, 3, dtype=self.dtype)
        self.v = torch.zeros(num_envs, 3, dtype=self.dtype)

    ROT = torch.tensor([[0.8, -0.6, 0.0], [0.6, 0.8, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64)

    @staticmethod
    def f(q, v, a):
        q2 = GAIN * q + EPS * torch.stack([a[:, 0], a[:, 1], a[:, 0] - a[:, 1]], 1)
        return q2, v @ GainEnv.ROT.to(v.dtype), q.sum(1) - 0.1 * (a * a).sum(1)

    def reset(self):
        self.q = ((torch.rand((self.num_envs, 3), generator=self.g, dtype=torch.float64) - 0.5) * EPS).to(self.dtype)
        self.v = (torch.rand((self.num_envs, 3), generator=self.g, dtype=torch.float64) * 2 - 1).to(self.dtype)

    def step(self, act, auto_reset=False):
        self.q, self.v, r = self.f(self.q, self.v, act.to(self.dtype))
        z = torch.zeros(self.num_envs, dtype=self.dtype)
        return None, r, z, z.clone()

    def qpos_qvel(self):
        return torch.cat([self.q, self.v], 1)

    def get_state(self):
        return (self.q.clone(), self.v.clone())

    def set_state(self, st, warm_from=None):
        self.q, self.v = st[0].clone(), st[1].clone()

    def step_vjp(self, act, gq, gv, grew, gaux, nonfinite=None):
        q = self.q.clone().requires_grad_(True)
        v = self.v.clone().requires_grad_(True)
        a = act.to(self.dtype).clone().requires_grad_(True)
        q2, v2, r = self.f(q, v, a)
        torch.autograd.backward([q2, v2, r], [gq.to(self.dtype), gv.to(self.dtype), grew.to(self.dtype)])
        return q.grad, v.grad, a.grad, None


def _gain_cfg(H, **kw):
    return _cfg(horizon=H, diverge_qvel=None, normalize_observations=False, **kw)


def _gain_trainer(cfg, seed=0, **kw):
    """APGTrainer on GainEnv with every policy parameter drawn at random (the initial policy's output
    layer is ~0: every action, and so every row of the parameter gradient, would be the same)."""
    tr = apg.APGTrainer(cfg, GainEnv(cfg.batch_size, seed), device="cpu", **kw)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in tr.policy.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.5)
    return tr


def _clip(g, clip):
    g = g.double()
    return g * torch.clamp(clip / (torch.linalg.vector_norm(g) + 1e-16), max=1.0)


def _fp64_clipped_gradient(tr, H):
    """The clipped gradient of the GainEnv rollout loss by fp64 autograd through the whole rollout, under
    tr's policy (its fp32 parameters, exactly, in fp64)."""
    import copy
    pol = copy.deepcopy(tr.policy).double()
    B, cfg = tr.env.num_envs, tr.cfg
    env = GainEnv(B, 0)
    env.reset()
    q, v = env.q.double(), env.v.double()
    ret, disc = torch.zeros(B, dtype=torch.float64), 1.0
    for _ in range(H):
        a = pol(torch.cat([q, v], 1))
        q, v, r = GainEnv.f(q, v, a)
        ret = ret + disc * r
        disc *= cfg.gamma
    (-ret.mean()).backward()
    return _clip(torch.cat([p.grad.reshape(-1) for p in pol.parameters()]), cfg.grad_clip)


def _sweep_clipped_gradient(H, scale):
    """(clipped gradient of the trainer's sweep on GainEnv, its trainer, envs the reverse guard cut)."""
    cfg = _gain_cfg(H)
    tr = _gain_trainer(cfg, scale_cotangents=scale)
    out = tr.loss_and_grad(use_norm=False)
    g = torch.cat([p.grad.reshape(-1) for p in tr.policy.parameters()]).double()
    if scale:
        g = g * apg._pow2(tr.last_scale[0])
    return _clip(g, cfg.grad_clip), tr, int(out[3][1])


def _rel_err(a, b):
    return float((a - b).abs().max() / b.abs().max())


def test_forced_rescale_is_exact():
    """Threshold 0: every env whose cotangents reach 1 rescales at every step from then on; the parameter
    gradient, brought back from 2^-E, is the unscaled sweep's bit for bit."""
    cfg = _cfg()
    trs = [apg.APGTrainer(cfg, PointEnvF32(cfg.batch_size, 0), device="cpu", **kw)
           for kw in ({}, {"scale_cotangents": True, "scale_threshold_log2": 0})]
    outs = [tr.loss_and_grad(use_norm=False) for tr in trs]
    assert torch.equal(outs[0][0], outs[1][0])
    E, scaled = trs[1].last_scale
    assert int(E) > 0 and int(scaled) > 0, "no exponent left 0: the comparison shows nothing"
    assert trs[0].last_scale is None
    for p, q in zip(trs[0].policy.parameters(), trs[1].policy.parameters()):
        assert p.grad.dtype == torch.float32 and bool(p.grad.abs().max() > 0)
        assert torch.equal(p.grad, apg._ldexp(q.grad, E))


def test_overflowing_rollout_keeps_every_env_and_matches_fp64():
    """GainEnv, 8 envs, H = 40: GAIN^H = 2^160 is outside fp32 and inside fp64. The unscaled sweep cuts
    every env and is left with a wrong gradient; the scaled one cuts none, and its clipped gradient is the
    clipped gradient of fp64 autograd through the same rollout.

    Tolerance (relative to the clipped gradient's largest entry): the fp32-vs-fp64 disagreement of the
    UNSCALED sweep on the same env at H0, the longest horizon at which it cuts no env, times H / H0 (the
    rounding accumulates per step) times 2. Measured: H0 = 33, disagreement 1.237e-07 there, so the bound
    at H = 40 is 2.998e-07; the scaled sweep's disagreement at H = 40: 1.645e-07 (the unscaled sweep's
    there: 2.0e-01, and it has to miss the bound a thousandfold for the case to show anything)."""
    H = 40
    B = _gain_cfg(H).batch_size
    g_u, tr_u, cut_u = _sweep_clipped_gradient(H, False)
    # (the guard zeroes an env's cotangent chain at the step where it overflows; the steps behind it keep
    # their small contributions, so what is left is a wrong gradient rather than a zero one)
    err_u = _rel_err(g_u, _fp64_clipped_gradient(tr_u, H))
    H0 = max(h for h in range(24, H) if _sweep_clipped_gradient(h, False)[2] == 0)
    g0, tr0, _ = _sweep_clipped_gradient(H0, False)
    err0 = _rel_err(g0, _fp64_clipped_gradient(tr0, H0))
    tol = err0 * (H / H0) * 2
    g_s, tr_s, cut_s = _sweep_clipped_gradient(H, True)
    ref = _fp64_clipped_gradient(tr_s, H)
    err = _rel_err(g_s, ref)
    print(f"H0 = {H0}, unscaled fp32-vs-fp64 at H0: {err0:.3e}, bound at H = {H}: {tol:.3e}, scaled at H: {err:.3e}, "
          f"unscaled at H: {err_u:.3e}, E = {int(tr_s.last_scale[0])}")
    assert cut_u == B and err_u > 1000 * tol
    assert cut_s == 0 and bool(torch.isfinite(g_s).all()) and float(g_s.abs().max()) > 0
    assert int(tr_s.last_scale[0]) > 0 and int(tr_s.last_scale[1]) == B
    assert 0 < err0 and err <= tol
    tr_c = _gain_trainer(_gain_cfg(H), scale_cotangents=True)
    m = tr_c.update(0)  # the trainer's own clip reaches the same gradient, and reports the true norm
    g_upd = torch.cat([p.grad.reshape(-1) for p in tr_c.policy.parameters()]).double()
    assert _rel_err(g_upd, ref) <= tol
    assert m["reverse_nonfinite_envs"] == 0 and m["scaled_envs"] == B and m["cotangent_exp_max"] > 0
    assert 2.0 ** 64 < m["grad_norm"] < float("inf")


def test_clip_unchanged_where_nothing_is_scaled():
    """E = 0 (DiffPointEnv's cotangents stay far below the threshold): update() with scaling on leaves
    the clipped gradient, and so the parameters, of the update with it off, bit for bit -- clipping
    (grad_clip 1e-3) and not clipping (1e3), in fp64 (DiffPointEnv) and fp32 (its float32 copy)."""
    for clip in (1e-3, 1e3):
        for dbl in (False, True):
            cfg = _cfg(grad_clip=clip)
            trs = [apg.APGTrainer(cfg, (DiffPointEnv if dbl else PointEnvF32)(cfg.batch_size, 1), device="cpu",
                                  scale_cotangents=s) for s in (False, True)]
            if dbl:
                for tr in trs:
                    tr.policy.double()
            ms = [tr.update(0) for tr in trs]
            assert ms[1]["cotangent_exp_max"] == 0 and ms[1]["scaled_envs"] == 0
            assert ms[0]["grad_norm"] == ms[1]["grad_norm"] and (ms[0]["grad_norm"] > clip) == (clip < 1)
            for p, q in zip(trs[0].policy.parameters(), trs[1].policy.parameters()):
                assert torch.equal(p.grad, q.grad) and torch.equal(p, q)


def _dp_worker(rank, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    tdist.init_process_group("gloo", rank=rank, world_size=2)
    # rank 1 discounts harder, so its cotangents grow less over the horizon than rank 0's
    cfg = _gain_cfg(40, gamma=0.99 if rank == 0 else 0.5)
    tr = _gain_trainer(cfg, seed=10 + rank, dist=tdist, scale_cotangents=True)
    ms = tr.train(3, verbose=False)
    torch.save({"p": torch.cat([p.detach().reshape(-1) for p in tr.policy.parameters()]),
                "E": torch.tensor([m["cotangent_exp_max"] for m in ms]),
                "own_E": int(tr.last_scale[0])}, out[rank])
    tdist.destroy_process_group()


def test_data_parallel_ranks_stay_identical_with_scaling(tmp_path):
    """Two gloo ranks on the exploding stand-in, scaling on: the ranks' sweeps end at different exponents
    (rank 1 discounts harder), the exponent is MAX-reduced before the gradients are summed, and the
    parameters stay identical across ranks, finite, and move."""
    out = [str(tmp_path / "r0.pt"), str(tmp_path / "r1.pt")]
    mp.spawn(_dp_worker, args=(_port(), out), nprocs=2, join=True)
    a, b = torch.load(out[0], weights_only=True), torch.load(out[1], weights_only=True)
    torch.testing.assert_close(a["p"], b["p"], rtol=0, atol=0)
    assert bool(torch.isfinite(a["p"]).all())
    assert torch.equal(a["E"], b["E"]) and int(a["E"].min()) > 0
    assert a["own_E"] != b["own_E"] and max(a["own_E"], b["own_E"]) == int(a["E"][-1])
    ref = _gain_trainer(_gain_cfg(40))
    assert not torch.equal(a["p"], torch.cat([p.detach().reshape(-1) for p in ref.policy.parameters()]))
