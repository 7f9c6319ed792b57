"""What the sensor readout costs: us per call of mjl_sensors with POS | VEL (one launch) and with
POS | VEL | ACC (a forward pass, then the readout) at 2048 envs of humanoid_mjx carrying the full humanoid
sensor set (jointpos, jointvel and jointlimitfrc on its 21 hinges, an IMU on the torso: gyro, accelerometer,
framequat, and the two touch sensors: 68 sensors), beside mjl_forward and the env step measured in the same
run. States: the normal_stand keyframe with joint noise and random velocities, 30 env steps of random actions
in. HIP events on the launch stream, 200 calls after 20, three interleaved rounds per variant, medians.
Writes profiles/sensors/sensor_cost.json (or the path given) and prints it."""
import dataclasses
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mujoco-mjx-lab_amd"))
import torch  # noqa: E402

import mjx_amd  # noqa: E402
from mjx_amd import _lib, abi, mjcf, mjx  # noqa: E402
from mjx_amd.config import reference_ppo_config  # noqa: E402
from mjx_amd.envs import HumanoidEnv, resolve_ids  # noqa: E402

B, CALLS, WARMUP, ROUNDS = 2048, 200, 20, 3


def full_sensor_model():
    text = open(os.path.join(ROOT, "tests", "golden", "humanoid_mjx.xml")).read()
    hinges = mjx_amd.load_model("humanoid_mjx").names["joint"][1:]
    text = re.sub(r'(<body name="torso"[^>]*>)', r'\1\n<site name="imu" pos="0 0 0.1" quat="0.7 0.1 -0.5 0.5" size="0.01"/>',
                  text, count=1)
    s = [f'<{t} name="{t}_{j}" joint="{j}"/>' for t in ("jointpos", "jointvel", "jointlimitfrc") for j in hinges]
    s += ['<gyro name="gyro" site="imu"/>', '<accelerometer name="accel" site="imu"/>',
          '<framequat name="orientation" objtype="site" objname="imu"/>',
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
    m = full_sensor_model()
    sys_ = mjx.put_model(m)
    cfg = resolve_ids(m, dataclasses.replace(reference_ppo_config().env_config))
    env = HumanoidEnv(sys_, cfg, B, seed=0)
    env.reset()
    g = torch.Generator(device="cuda").manual_seed(0)
    act = lambda: torch.rand((B, m.nu), generator=g, device="cuda") * 2 - 1
    for _ in range(30):
        env.step(act())
    a = act()
    out = torch.zeros((B, sys_.nrsensordata), device="cuda")
    st = abi.SENSOR_STAGE
    variants = {
        "env_step": lambda: env.step(a),
        "sensors_pos_vel": lambda: env.sensors(stages=st["pos"] | st["vel"], out=out),
        "forward": lambda: mjx.forward(sys_, env.data),
        "sensors_pos_vel_acc": lambda: env.sensors(out=out),
    }
    runs = {k: [] for k in variants}
    for _ in range(ROUNDS):  # interleaved
        for k, fn in variants.items():
            runs[k].append(timed(fn))
    res = {"envs": B, "model": "humanoid_mjx", "nrsensor": m.nrsensor, "nrsensordata": m.nrsensordata, "calls": CALLS,
           "warmup": WARMUP, "rounds": ROUNDS, "unit": "us per call (HIP events)", "build": _lib.build_info(),
           "us": {k: {"median": round(statistics.median(v), 2), "runs": [round(x, 2) for x in v]} for k, v in runs.items()}}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sensors", "sensor_cost.json"))
