"""What a control step of k physics steps costs: mjl_step_n / mjl_env_step_n(k) against the k single-step launches
it stands for (k - 1 mjl_step and, for the env step, one mjl_env_step), each side captured as one hipGraph so
that neither pays host launch gaps. This is the measurement that decided between a fused kernel and host-issued
launches (DESIGN.md "Substeps": the recorded JSON is the fused kernel's); with the entries issuing the launches
themselves the two sides differ by the env step's control kernel only.

humanoid_mjx at 2048 and 4096 envs, k in {2, 4, 5, 8}, rollout-like states: 64 random-action env steps from a
reset (pooled auto-reset on). Every timed replay starts from the same saved state (restored outside the timed
interval), so both sides solve the same k substeps. The two sides alternate replay by replay; the medians of
REPS replays each are reported in us per control step with their ratio, and the spread (p10..p90) of each side.
Writes profiles/substeps/substep_cost.json (or the path given) and prints it."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mujoco-mjx-lab_amd"))
import torch  # noqa: E402

import mjx_amd  # noqa: E402
from mjx_amd import _lib, abi, mjx  # noqa: E402
from mjx_amd.config import reference_ppo_config  # noqa: E402
from mjx_amd.envs import HumanoidEnv, resolve_ids  # noqa: E402

KS, SIZES, REPS, WARM = (2, 4, 5, 8), (2048, 4096), 40, 5


def capture(fn, stream):
    with torch.cuda.stream(stream):
        fn()
        stream.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            fn()
    stream.synchronize()
    return g


def main(out_path):
    m = mjx_amd.load_model("humanoid_mjx")
    sys_ = mjx.put_model(m)
    cfg = resolve_ids(m, reference_ppo_config().env_config)
    res = {"model": "humanoid_mjx", "reps": REPS, "unit": "us per control step (HIP events around one graph replay)",
           "build": _lib.build_info(), "results": []}
    stream = torch.cuda.Stream()
    for B in SIZES:
        env = HumanoidEnv(sys_, cfg, B, seed=1)
        env.enable_reset_pool(4)
        env.reset()
        env.fill_reset_pool(torch.tensor([4], dtype=torch.int32, device="cuda"))
        g = torch.Generator(device="cuda").manual_seed(0)
        for _ in range(64):
            env.step(torch.rand((B, m.nu), generator=g, device="cuda") * 2 - 1)
        act = torch.rand((B, m.nu), generator=g, device="cuda") * 2 - 1
        perm, sign, _, _ = abi.flip_tables(cfg, m.nu, env.obs_dim)
        flipped = act[:, torch.tensor(perm, device="cuda")] * torch.tensor(sign, device="cuda")
        ctrl = torch.where(env.aux[:, :1] > 0.5, flipped, act).clamp(-1, 1).contiguous()
        saved = env.get_state().clone()
        torch.cuda.synchronize()
        for k in KS:
            def seq_step():
                for _ in range(k):
                    mjx.step(sys_, env.data, ctrl)

            def seq_env():
                for _ in range(k - 1):
                    mjx.step(sys_, env.data, ctrl)
                env.n_frames = 1
                env.step(act, counter=1)

            def fused_env():
                env.n_frames = k
                env.step(act, counter=1)

            sides = {"step": (lambda: mjx.step(sys_, env.data, ctrl, nstep=k), seq_step), "env_step": (fused_env, seq_env)}
            for entry, fns in sides.items():
                graphs = [capture(f, stream) for f in fns]
                t = ([], [])
                with torch.cuda.stream(stream):
                    for r in range(WARM + REPS):
                        for side in (0, 1):
                            env.set_state(saved)
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record(stream)
                            graphs[side].replay()
                            e1.record(stream)
                            e1.synchronize()
                            if r >= WARM:
                                t[side].append(e0.elapsed_time(e1) * 1e3)
                q = lambda x, p: sorted(x)[int(p * (len(x) - 1))]  # noqa: E731
                med = [statistics.median(x) for x in t]
                row = {"envs": B, "k": k, "entry": entry, "fused_us": round(med[0], 2), "sequential_us": round(med[1], 2),
                       "fused_over_sequential": round(med[0] / med[1], 4),
                       "fused_p10_p90": [round(q(t[0], .1), 2), round(q(t[0], .9), 2)],
                       "sequential_p10_p90": [round(q(t[1], .1), 2), round(q(t[1], .9), 2)]}
                res["results"].append(row)
                print(json.dumps(row), flush=True)
        env.n_frames = 1
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "substeps", "substep_cost.json"))
