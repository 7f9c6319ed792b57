"""What a range scan costs: us per call of mjl_ray_scan (yaw-aligned grids on the torso, the carrying body left
out) at 2048 envs of humanoid_mjx for 1, 35 (5 x 7) and 187 (11 x 17) rays, in both kernel layouts: "chunks"
(one wavefront per env and 64 rays: the kinematics is repeated per chunk) and "per_env" (one wavefront per env
strides over all its rays: kinematics once per env), chosen with MJL_OPT_RAY_CHUNK; "default" is the library's
choice. Beside them mjl_sensors with stages = pos on a frame-sensor model and the env step, measured in the
same run. States: 30 env steps of random actions in. HIP events on the launch stream, 200 calls after 20, three
interleaved rounds per variant, medians. Writes profiles/rays/ray_cost.json (or the path given) and prints it."""
import dataclasses
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mujoco-mjx-lab_amd"))
import torch  # noqa: E402

from mjx_amd import _lib, abi, mjcf, mjx, rays  # noqa: E402
from mjx_amd.config import reference_ppo_config  # noqa: E402
from mjx_amd.envs import HumanoidEnv, resolve_ids  # noqa: E402

B, CALLS, WARMUP, ROUNDS = 2048, 200, 20, 3
PATTERNS = {1: rays.grid_pattern(1, 1, 0.1, 0.1, 0.5), 35: rays.grid_pattern(5, 7, 0.1, 0.1, 0.5),
            187: rays.grid_pattern(11, 17, 0.1, 0.1, 0.5)}
LAYOUTS = {"chunks": 64, "per_env": 65535, "default": 0}


def model():
    text = open(os.path.join(ROOT, "tests", "golden", "humanoid_mjx.xml")).read()
    s = ['<framepos name="p" objtype="xbody" objname="torso"/>', '<framequat name="q" objtype="xbody" objname="torso"/>',
         '<touch name="touch_foot_right" site="site_foot_right"/>', '<touch name="touch_foot_left" site="site_foot_left"/>']
    text = re.sub(r"<sensor>.*?</sensor>", "<sensor>\n" + "\n".join(s) + "\n</sensor>", text, count=1, flags=re.S)
    return mjcf.compile_xml_string(text, "humanoid_mjx")


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(CALLS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / CALLS * 1e3  # us


def main(out_path):
    m = model()
    sys_ = mjx.put_model(m)
    cfg = resolve_ids(m, dataclasses.replace(reference_ppo_config().env_config))
    env = HumanoidEnv(sys_, cfg, B, seed=0)
    env.reset()
    g = torch.Generator(device="cuda").manual_seed(0)
    act = lambda: torch.rand((B, m.nu), generator=g, device="cuda") * 2 - 1
    for _ in range(30):
        env.step(act())
    a = act()
    sens = torch.zeros((B, sys_.nrsensordata), device="cuda")

    def scan(n, chunk):
        def fn():
            env.data.set_option(abi.OPT_RAY_CHUNK, chunk)
            env.scan("torso", PATTERNS[n], align="yaw")
        return fn
    variants = {"env_step": lambda: env.step(a),
                "sensors_pos": lambda: env.sensors(stages=abi.SENSOR_STAGE["pos"], out=sens)}
    for n in PATTERNS:
        for name, chunk in LAYOUTS.items():
            variants[f"scan_{n}_{name}"] = scan(n, chunk)
    runs = {k: [] for k in variants}
    for _ in range(ROUNDS):  # interleaved
        for k, fn in variants.items():
            runs[k].append(timed(fn))
    env.data.set_option(abi.OPT_RAY_CHUNK, 0)
    res = {"envs": B, "model": "humanoid_mjx", "calls": CALLS, "warmup": WARMUP, "rounds": ROUNDS,
           "unit": "us per call (HIP events)", "layouts": {k: f"MJL_OPT_RAY_CHUNK = {v}" for k, v in LAYOUTS.items()},
           "build": _lib.build_info(),
           "us": {k: {"median": round(statistics.median(v), 2), "runs": [round(x, 2) for x in v]} for k, v in runs.items()}}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "rays", "ray_cost.json"))
