"""Cost of attached applied forces: pooled env step and mjl_step at 2048 envs, attached (random nonzero,
and all-zero: the same dynamics) vs detached, device events, warm-up, median of windows, the variants
alternating. Usage: python tools/applied_bench.py [out.json]  (DESIGN.md "Applied forces")."""
import json, os, sys, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))  # tools/ -> repository root
sys.path.insert(0, os.path.join(ROOT, "mujoco-mjx-lab_amd"))
import torch
import mjx_amd
from mjx_amd import mjx
from mjx_amd.config import reference_ppo_config
from mjx_amd.envs import HumanoidEnv, resolve_ids

B, WIN, NWIN = 2048, 200, 9
m = mjx_amd.load_model("humanoid_mjx")
sys_ = mjx.put_model(m)
g = torch.Generator(device="cuda").manual_seed(0)
qfrc = (torch.rand((B, m.nv), generator=g, device="cuda") * 2 - 1) * 5
xfrc = (torch.rand((B, m.nbody, 6), generator=g, device="cuda") * 2 - 1) * 20
acts = torch.rand((WIN, B, m.nu), generator=g, device="cuda") * 2 - 1

def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for t in range(WIN):
        fn(t)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / WIN  # us per call

def make_env():
    env = HumanoidEnv(sys_, resolve_ids(m, reference_ppo_config().env_config), B, seed=1)
    env.enable_reset_pool(16)
    env.reset()
    return env

res = {}
envs = {"detached": make_env(), "attached": make_env(), "attached_zero": make_env()}
envs["attached"].attach_applied(qfrc, xfrc)
envs["attached_zero"].attach_applied(torch.zeros_like(qfrc), torch.zeros_like(xfrc))
n16 = torch.tensor([16], dtype=torch.int32, device="cuda")
samples = {k: [] for k in envs}
for w in range(NWIN + 2):
    for k, env in envs.items():
        env.fill_reset_pool(n16)
        us = window(lambda t: env.step(acts[t]))
        if w >= 2:
            samples[k].append(us)
res["pooled_env_step_us"] = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in samples.items()}
datas = {"detached": mjx.make_data(sys_, B), "attached": mjx.make_data(sys_, B), "attached_zero": mjx.make_data(sys_, B)}
datas["attached"].attach_applied(qfrc, xfrc)
datas["attached_zero"].attach_applied(torch.zeros_like(qfrc), torch.zeros_like(xfrc))
samples = {k: [] for k in datas}
ctrl = acts[0].contiguous()
for w in range(NWIN + 2):
    for k, d in datas.items():
        d.set("qpos", torch.tensor(m.qpos0, dtype=torch.float32).repeat(B, 1))
        d.set("qvel", torch.zeros((B, m.nv)))
        us = window(lambda t: mjx.step(sys_, d, ctrl))
        if w >= 2:
            samples[k].append(us)
res["mjl_step_us"] = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in samples.items()}
res["nenv"], res["window_calls"], res["windows"] = B, WIN, NWIN
print(json.dumps(res))
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "applied", "applied_cost.json")
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
json.dump(res, open(out, "w"), indent=1)
