"""Times mjl_body_data beside mjl_sensors (pos | vel) at 2048 envs with HIP events: per launch one event pair,
50 warm-up launches, 300 timed, the median in microseconds. DESIGN.md "Body data" quotes the output.

    python tools/body_data_bench.py [--envs 2048]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mujoco-mjx-lab_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))  # tests/test_sensors_gpu.py imports it

import mjx_amd  # noqa: E402
from mjx_amd import abi, mjcf, mjx  # noqa: E402


def median_us(fn, warm=50, n=300):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=2048)
    args = ap.parse_args()
    from test_sensors_gpu import sensor_xml  # the humanoid with the full sensor set (127 sensors)
    m = mjcf.compile_xml_string(sensor_xml("humanoid_mjx"), "humanoid_mjx")
    sys_ = mjx.put_model(m)
    d = mjx.make_data(sys_, args.envs)
    rng = np.random.default_rng(0)
    q = np.tile(m.qpos0, (args.envs, 1))
    q[:, 7:] += rng.uniform(-0.3, 0.3, (args.envs, m.nq - 7))
    d.set("qpos", torch.tensor(q, dtype=torch.float32))
    d.set("qvel", torch.tensor(rng.uniform(-1, 1, (args.envs, m.nv)), dtype=torch.float32))
    posvel = tuple(mjx.BODY_FIELDS)[:7]
    full = mjx.body_data(sys_, d, posvel)
    one = mjx.body_data(sys_, d, ("subtree_com",))
    sens = mjx.sensors(sys_, d, stages=abi.SENSOR_STAGE["pos"] | abi.SENSOR_STAGE["vel"])
    st = abi.SENSOR_STAGE["pos"] | abi.SENSOR_STAGE["vel"]
    res = {"envs": args.envs,
           "sensors_pos_vel_us": median_us(lambda: mjx.sensors(sys_, d, stages=st, out=sens)),
           "body_data_pos_vel_us": median_us(lambda: mjx.body_data(sys_, d, posvel, out=full)),
           "body_data_subtree_com_us": median_us(lambda: mjx.body_data(sys_, d, ("subtree_com",), out=one))}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
