"""Cost of per-env model parameters: pooled env step and mjl_step at 2048 envs for the plain batch, per-env
blocks holding the model's values (the cost of private model reads: nenv x sizeof(ModelF) no longer shared in
cache) and per-env blocks holding random values; plus set_model_params alone. Device events, warm-up, median of
windows, the variants alternating. Usage: python tools/randomize_bench.py [out.json]  (DESIGN.md "Per-env model
parameters")."""
import json, os, sys, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))  # tools/ -> repository root
sys.path.insert(0, os.path.join(ROOT, "mujoco-mjx-lab_amd"))
import torch
import mjx_amd
from mjx_amd import mjx
from mjx_amd.config import reference_ppo_config
from mjx_amd.envs import HumanoidEnv, resolve_ids
from mjx_amd.randomize import draw_model_params

B, WIN, NWIN = 2048, 200, 9
RANGES = {"mass": (0.5, 1.5), "friction": (0.3, 1.5), "damping": (0.5, 2.0), "armature": (0.5, 2.0), "gear": (0.7, 1.3)}
m = mjx_amd.load_model("humanoid_mjx")
sys_ = mjx.put_model(m)
g = torch.Generator(device="cuda").manual_seed(0)
acts = torch.rand((WIN, B, m.nu), generator=g, device="cuda") * 2 - 1
params = {k: v.cuda() for k, v in draw_model_params(m, B, RANGES, seed=0).items()}
VARIANTS = ("plain", "per_env_nominal", "per_env_random")

def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for t in range(WIN):
        fn(t)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / WIN  # us per call

def prepare(data, variant):
    if variant != "plain":
        data.enable_model_params()
    if variant == "per_env_random":
        data.set_model_params(**params)

def make_env(variant):
    env = HumanoidEnv(sys_, resolve_ids(m, reference_ppo_config().env_config), B, seed=1)
    prepare(env.data, variant)
    env.enable_reset_pool(16)
    env.reset()
    return env

def stats(samples):
    return {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in samples.items()}

res = {}
envs = {k: make_env(k) for k in VARIANTS}
n16 = torch.tensor([16], dtype=torch.int32, device="cuda")
samples = {k: [] for k in envs}
for w in range(NWIN + 2):
    for k, env in envs.items():
        env.fill_reset_pool(n16)
        us = window(lambda t: env.step(acts[t]))
        if w >= 2:
            samples[k].append(us)
res["pooled_env_step_us"] = stats(samples)
datas = {k: mjx.make_data(sys_, B) for k in VARIANTS}
for k, d in datas.items():
    prepare(d, k)
samples = {k: [] for k in datas}
ctrl = acts[0].contiguous()
for w in range(NWIN + 2):
    for k, d in datas.items():
        d.set("qpos", torch.tensor(m.qpos0, dtype=torch.float32).repeat(B, 1))
        d.set("qvel", torch.zeros((B, m.nv)))
        us = window(lambda t: mjx.step(sys_, d, ctrl))
        if w >= 2:
            samples[k].append(us)
res["mjl_step_us"] = stats(samples)
d = datas["per_env_random"]
samples = {"all_six_fields": [], "body_mass_only": []}
for w in range(NWIN + 2):
    for k, kw in (("all_six_fields", params), ("body_mass_only", {"body_mass": params["body_mass"]})):
        us = window(lambda t: d.set_model_params(**kw))
        if w >= 2:
            samples[k].append(us)
res["set_model_params_us"] = stats(samples)
res["nenv"], res["window_calls"], res["windows"] = B, WIN, NWIN
print(json.dumps(res))
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "randomize", "randomize_cost.json")
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
json.dump(res, open(out, "w"), indent=1)
