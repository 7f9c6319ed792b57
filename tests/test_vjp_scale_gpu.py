"""Exponent-carried cotangents on the GPU (mjl_vjp_scale_attach, csrc/adjoint.hip vjp_kernel's output stage;
APGTrainer scale_cotangents): the kernel's rescale is an exact power-of-two homogeneity of the VJP in every
guarded entry, the guard still cuts what is non-finite, a detached batch is untouched; the scaled trainer
reproduces the unscaled one bit for bit where nothing overflows, eager, graphed and unfused, and keeps the
envs of a rollout whose cotangents leave fp32 range."""
import pytest
import torch

from mjx_amd import apg
from test_apg import _cfg

pytestmark = pytest.mark.gpu


def _model(solver):
    import mjx_amd
    from mjx_amd import mjcf
    m = mjx_amd.load_model("humanoid_mjx")
    if solver == "cg44":
        m.solver, m.iterations, m.ls_iterations = mjcf.SOLVER_CG, 4, 4
    return m


def _humanoid(m, B, vjp, seed):
    from mjx_amd import mjx
    from mjx_amd.config import reference_ppo_config
    from mjx_amd.envs import HumanoidEnv, resolve_ids
    env = HumanoidEnv(mjx.put_model(m), resolve_ids(m, reference_ppo_config().env_config), B, seed=seed)
    return apg.HumanoidAPGEnv(env, vjp)


def _p2(n):
    return apg._pow2(torch.as_tensor(n, device="cuda"))


def _true(outs, e, shift=0):
    """The cotangents a call left, as fp64 true values: stored * 2^(e + shift) per env."""
    return [o.double() * _p2(e.long() + shift)[:, None] for o in outs]


@pytest.mark.parametrize("entry", ["recompute", "replay", "replay_policy"])
@pytest.mark.parametrize("unrolled", [0, 1])
def test_kernel_rescale_is_an_exact_homogeneity(unrolled, entry):
    """humanoid_mjx, 8 envs after five random steps; OPT_VJP_UNROLLED 0 (the MJCF's Newton) and 1 (CG 4/4);
    the recompute entries (mjl_env_step_vjp_guarded / _vjp_full), the replay and the replay with the
    policy's backward.

    The randn * 2^100 inputs also exercise the kernel's input stage: the unrolled CG reverse pass takes unit
    cotangents through intermediates more than 2^28 above them (with only the outputs rescaled, 5 of these
    8 envs left fp32 range inside the step and were cut), so inputs at or past the threshold are brought
    down to order 1 before the reverse passes."""
    from mjx_amd import abi
    from mjx_amd.ppo import APGPolicy, RunningMeanStd
    B, T = 8, abi.VJP_SCALE_THRESHOLD_LOG2
    m = _model("cg44" if unrolled else "model")
    aenv = _humanoid(m, B, "unrolled" if unrolled else "implicit", seed=2)
    env, dev = aenv.env, "cuda"
    env.reset()
    g = torch.Generator(device=dev).manual_seed(0)
    for _ in range(5):
        env.step(torch.rand((B, m.nu), generator=g, device=dev) * 2 - 1, auto_reset=False)
    st = env.get_state().clone()
    w = m.nq + m.nv
    policy = APGPolicy(w, m.nu, 32, 2, None, torch.Generator().manual_seed(1)).to(dev)
    with torch.no_grad():  # (the initial output layer is ~0)
        for p in policy.parameters():
            p.copy_(torch.randn(p.shape, generator=g, device=dev) * 0.3)
    nat = apg.NativeAPGPolicy(policy)
    rms = RunningMeanStd(w, torch.device(dev))
    o, on = torch.empty((B, w), device=dev), torch.empty((B, w), device=dev)
    snap = torch.empty(B, dtype=torch.uint8, device=dev)
    alive = torch.ones(B, dtype=torch.uint8, device=dev)
    ys = [torch.empty((B, n), device=dev) for n in nat.widths]
    act = nat.forward_obs(aenv, alive, rms, False, o, on, snap, ys).clone()
    if entry != "recompute":
        aenv.enable_vjp_tape(1)
        aenv.step_record(0, act)
    env.set_state(st)
    r = lambda *s: torch.randn(s, generator=g, device=dev)  # noqa: E731
    gq, gv, gr, gaux = r(B, m.nq), r(B, m.nv), r(B), r(B, abi.AUX_DIM)
    gws = r(B, m.nv) if unrolled else None

    def call(gq, gv, gws, gr, gaux):
        cnt = torch.zeros(1, device=dev)
        if entry == "replay_policy":
            out = nat.replay_bwd(aenv, 0, act, gq, gv, gws, gr, gaux, cnt, ys, o, snap, rms, False)
        elif entry == "replay":
            out = aenv.step_vjp_replay(0, act, gq, gv, gws, gr, gaux, cnt)
        elif unrolled:
            out = aenv.step_vjp_full(act, gq, gv, gws, gr, gaux, cnt)
        else:
            out = aenv.step_vjp(act, gq, gv, gr, gaux, cnt)
        return [x for x in out if x is not None], float(cnt)

    big = lambda x, k: None if x is None else x * float(2.0 ** k)  # noqa: E731
    before, n0 = call(gq, gv, gws, gr, gaux)
    small, _ = call(gq, gv, gws, big(gr, -100), gaux)  # detached: the state cotangents with g_rew * 2^-100
    lo, _ = call(gq, gv, gws, big(gr, -7), gaux)
    assert n0 == 0 and all(bool(torch.isfinite(x).all()) for x in before + small + lo)
    e = torch.zeros(B, dtype=torch.int32, device=dev)
    aenv.attach_vjp_scale(e, T)
    try:
        # below the threshold: the detached call bit for bit, exponents untouched
        out, n = call(gq, gv, gws, gr, gaux)
        assert n == 0 and int(e.abs().max()) == 0
        for a, b in zip(out, before):
            assert torch.equal(a, b)
        # exponent 7 in with the unscaled g_rew = exponent 0 in with g_rew * 2^-7 (true values * 2^-7)
        e.fill_(7)
        out, n = call(gq, gv, gws, gr, gaux)
        assert n == 0
        for a, b in zip(_true(out, e, -7), lo):
            assert torch.equal(a, b.double())
        # an env with a NaN input cotangent: zeroed, counted, exponent 0; the others as without it
        e.fill_(7)
        gq2 = gq.clone()
        gq2[3, 0] = float("nan")
        bad, n = call(gq2, gv, gws, gr, gaux)
        keep = torch.arange(B, device=dev) != 3
        assert n == 1 and int(e[3]) == 0
        for a, b in zip(bad, out):
            assert bool(torch.all(a[3] == 0)) and torch.equal(a[keep], b[keep])
        # all-zero input cotangents: the early return, exponent back to 0
        e.fill_(7)
        z = torch.zeros_like
        out, n = call(z(gq), z(gv), None if gws is None else z(gws), z(gr), z(gaux))
        assert n == 0 and int(e.abs().max()) == 0 and all(float(x.abs().max()) == 0 for x in out)
        from mjx_amd._lib import MjlError
        with pytest.raises(MjlError):
            aenv.attach_vjp_scale(e, 500)
    finally:
        aenv.attach_vjp_scale(None, T)
    out, n = call(gq, gv, gws, gr, gaux)  # detached again: as before attaching
    for a, b in zip(out, before):
        assert torch.equal(a, b)
    e.zero_()
    aenv.attach_vjp_scale(e, T)
    try:
        # state cotangents * 2^100 at exponent 0: finite outputs at a positive exponent, and exactly
        # 2^100 times the detached call on the unscaled cotangents
        out, n = call(big(gq, 100), big(gv, 100), big(gws, 100), gr, big(gaux, 100))
        print(f"unrolled {unrolled} {entry}: cut at 2^100: {n}, exponents {e.tolist()}, detached outputs' largest "
              f"magnitude {float(max(x.abs().max() for x in before)):.3e}")
        assert n == 0 and all(bool(torch.isfinite(x).all()) for x in out) and int(e.min()) > 0
        assert float(max(x.abs().max() for x in out)) < 2.0
        for a, b in zip(_true(out, e), small):
            assert torch.equal(a, b.double() * float(2.0 ** 100))
    finally:
        aenv.attach_vjp_scale(None, T)


def _trainers(solver, vjp, B, H, specs, seed=3, **cfg_kw):
    m = _model(solver)
    cfg = _cfg(batch_size=B, horizon=H, hidden_size=32, **cfg_kw)
    return [apg.APGTrainer(cfg, _humanoid(m, B, vjp, seed), device="cuda", **kw) for kw in specs]


def _same_update(ms, trs, step):
    for k in ("loss", "grad_norm", "mean_reward", "nonfinite_envs"):
        assert all(m[k] == ms[0][k] or (m[k] != m[k] and ms[0][k] != ms[0][k]) for m in ms), f"update {step}: {k}"
    for tr in trs[1:]:
        for p, q in zip(trs[0].policy.parameters(), tr.policy.parameters()):
            assert torch.equal(p.grad, q.grad), f"update {step}: gradient"
            assert torch.equal(p, q), f"update {step}: parameters"


@pytest.mark.parametrize("solver,vjp", [("model", "implicit"), ("cg44", "unrolled")])
def test_trainer_forced_rescale_bit_identical(solver, vjp):
    """64 envs x 8 steps, threshold 1 (an env rescales once a cotangent reaches 2): the scaled trainer's
    clipped gradients and parameters are the unscaled trainer's bit for bit over 4 updates, eager and as
    a hipGraph replay (through the warm-up call, the capture and the replays of both normalisation graphs)."""
    on = {"scale_cotangents": True, "scale_threshold_log2": 1}
    trs = _trainers(solver, vjp, 64, 8, [{"use_graph": False}, {"use_graph": False, **on}, {"use_graph": True, **on}])
    scaled = 0
    for step in range(4):
        ms = [tr.update(step) for tr in trs]
        _same_update(ms, trs, step)
        assert ms[0]["scaled_envs"] == 0 and ms[1]["scaled_envs"] == ms[2]["scaled_envs"]
        assert ms[1]["cotangent_exp_max"] == ms[2]["cotangent_exp_max"]
        assert (ms[1]["scaled_envs"] > 0) == (ms[1]["cotangent_exp_max"] > 0)
        scaled += ms[1]["scaled_envs"]
    assert scaled > 0, "no exponent left 0: the comparison shows nothing"
    assert set(trs[2]._graphs) == {True} and trs[1]._graphs == {}


@pytest.mark.parametrize("solver,vjp", [("model", "implicit"), ("cg44", "unrolled")])
def test_trainer_forced_rescale_unfused_backward(monkeypatch, solver, vjp):
    """MJL_APG_FUSED_BWD=0 (the policy's backward as its own launch, added to the state cotangents behind
    the kernel's rescale): the gradients of the fused path."""
    on = {"scale_cotangents": True, "scale_threshold_log2": 1, "use_graph": False}
    trs = _trainers(solver, vjp, 64, 8, [on, on])
    scaled = 0
    for step in range(2):
        ms = []
        for tr, fused in zip(trs, ("1", "0")):
            monkeypatch.setenv("MJL_APG_FUSED_BWD", fused)
            ms.append(tr.update(step))
        _same_update(ms, trs, step)
        scaled += min(m["scaled_envs"] for m in ms)
    assert scaled > 0


def test_trainer_keeps_envs_whose_cotangents_overflow():
    """256 envs x 128 steps, CG 4/4 with the unrolled VJP (the reference's train_apg.py at an eighth of its
    batch), two updates, seed 3. Unscaled, the reverse guard cuts envs (their cotangents leave fp32
    range); scaled, at most 5 (2 % of 256) remain cut, the forward is the same, and the gradient norm -- the
    true one -- and the parameters are finite."""
    B, H = 256, 128
    res = []
    for on in (False, True):
        tr, = _trainers("cg44", "unrolled", B, H, [{"scale_cotangents": on}])
        ms = [tr.update(step) for step in range(2)]
        res.append(ms)
        print("scale_cotangents", on, [{k: m[k] for k in ("reverse_nonfinite_envs", "forward_dropped_envs", "scaled_envs",
                                                          "cotangent_exp_max", "grad_norm")} for m in ms])
        assert all(bool(torch.isfinite(p).all()) for p in tr.policy.parameters()) or not on
        del tr
        torch.cuda.empty_cache()
    for mu, ms in zip(*res):
        assert mu["reverse_nonfinite_envs"] >= 1
        assert ms["reverse_nonfinite_envs"] <= 5
        assert ms["grad_norm"] == ms["grad_norm"] and ms["grad_norm"] < float("inf")
        assert ms["cotangent_exp_max"] > 0 and ms["scaled_envs"] > 0
    # the first update's forward is the same rollout; the second's follows each run's own parameters
    assert res[0][0]["forward_dropped_envs"] == res[1][0]["forward_dropped_envs"]
    assert res[0][0]["loss"] == res[1][0]["loss"]
