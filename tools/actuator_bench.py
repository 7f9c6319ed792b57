"""Cost of general (PD) actuators: the pooled env step at 2048 envs on humanoid_mjx, its motors against the same
model with pd_actuators (kp 30, kv 2, action scale 0.5), plus a PD model without velocity term (b2 = 0: the
actuation branch alone, no integrator addend). Every window of every variant starts from the same packed state
and runs the same actions; device events, warm-up, median of windows, the variants alternating.
Usage: python tools/actuator_bench.py [out.json]  (DESIGN.md "Actuators")."""
import json, os, sys, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))  # tools/ -> repository root
sys.path.insert(0, os.path.join(ROOT, "mujoco-mjx-lab_amd"))
import torch
import mjx_amd
from mjx_amd import mjx
from mjx_amd.actuators import pd_actuators
from mjx_amd.config import reference_ppo_config
from mjx_amd.envs import HumanoidEnv, resolve_ids

B, WIN, NWIN = 2048, 200, 9
m = mjx_amd.load_model("humanoid_mjx")
models = {"motor": m, "pd": pd_actuators(m, 30.0, 2.0, 0.5), "pd_no_velocity_term": pd_actuators(m, 30.0, 0.0, 0.5)}
g = torch.Generator(device="cuda").manual_seed(0)
acts = torch.rand((WIN, B, m.nu), generator=g, device="cuda") * 2 - 1

def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for t in range(WIN):
        fn(t)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / WIN  # us per call

def make_env(model):
    env = HumanoidEnv(mjx.put_model(model), resolve_ids(model, reference_ppo_config().env_config), B, seed=1)
    env.enable_reset_pool(16)
    env.reset(counter=0)
    return env

envs = {k: make_env(v) for k, v in models.items()}
start = envs["motor"].get_state().clone()  # one start state for every variant and window
n16 = torch.tensor([16], dtype=torch.int32, device="cuda")
samples = {k: [] for k in envs}
for w in range(NWIN + 2):
    for k, env in envs.items():
        env.set_state(start)
        env.fill_reset_pool(n16)
        us = window(lambda t: env.step(acts[t]))
        if w >= 2:
            samples[k].append(us)
res = {"pooled_env_step_us": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in samples.items()}}
med = {k: v["median"] for k, v in res["pooled_env_step_us"].items()}
res["ratio_to_motor"] = {k: med[k] / med["motor"] for k in med}
res["nenv"], res["window_calls"], res["windows"] = B, WIN, NWIN
print(json.dumps(res))
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "actuators", "actuator_cost.json")
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
json.dump(res, open(out, "w"), indent=1)
