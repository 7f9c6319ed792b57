"""Times mjl_jac_dot beside mjl_jac on the same 4 local points, and mjl_centroidal (the whole model) beside
mjl_body_data's vel outputs, at 2048 envs with HIP events: per launch one event pair, 50 warm-up launches, 300
timed, the median in microseconds. Writes profiles/taskspace/cost.json (DESIGN.md "Task-space dynamics" quotes it).

    python tools/taskspace_bench.py [--envs 2048] [--out profiles/taskspace/cost.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mujoco-mjx-lab_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mjx_amd  # noqa: E402
from mjx_amd import mjx  # noqa: E402
from mjx_amd._lib import build_info  # noqa: E402

from dyn_bench import median_us  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "taskspace", "cost.json"))
    args = ap.parse_args()
    m = mjx_amd.load_model("humanoid_mjx")
    sys_ = mjx.put_model(m)
    n = args.envs
    d = mjx.make_data(sys_, n)
    rng = np.random.default_rng(0)
    q = np.tile(m.qpos0, (n, 1))
    q[:, 7:] += rng.uniform(-0.3, 0.3, (n, m.nq - 7))
    d.set("qpos", torch.tensor(q, dtype=torch.float32))
    d.set("qvel", torch.tensor(rng.uniform(-1, 1, (n, m.nv)), dtype=torch.float32))
    dev = d.device
    res = {"envs": n, "model": "humanoid_mjx", "nv": m.nv, "src_hash": build_info()["tree_src_hash"],
           "method": "HIP events around one launch, 50 warm-up, median of 300, microseconds"}
    frames = [("xbody", 1 + k % (m.nbody - 1)) for k in range(4)]
    bodies, local = mjx.jac_frames(sys_, frames, [0.05, 0.0, 0.1])
    tabs = (torch.tensor(bodies, dtype=torch.int32, device=dev), torch.tensor(local, device=dev))
    jo = mjx.jac_local(sys_, d, frames, _dev=tabs)
    res["jac_local_4_points_us"] = median_us(lambda: mjx.jac_local(sys_, d, frames, out=jo, _dev=tabs))
    jd = mjx.jac_dot_local(sys_, d, frames, _dev=tabs)
    res["jac_dot_4_points_all_us"] = median_us(lambda: mjx.jac_dot_local(sys_, d, frames, out=jd, _dev=tabs))
    only = (None, None, jd[2])
    res["jac_dot_4_points_jdotv_us"] = median_us(lambda: mjx.jac_dot_local(sys_, d, frames, out=only, _dev=tabs))
    vel = ("cvel", "subtree_linvel", "subtree_angmom")
    bd = mjx.body_data(sys_, d, vel)
    res["body_data_vel_us"] = median_us(lambda: mjx.body_data(sys_, d, vel, out=bd))
    root = torch.zeros(1, dtype=torch.int32, device=dev)
    ce = mjx.centroidal(sys_, d, 0, _dev=root)
    res["centroidal_whole_model_us"] = median_us(lambda: mjx.centroidal(sys_, d, 0, out=ce, _dev=root))
    res["jac_dot_all_over_jac"] = res["jac_dot_4_points_all_us"] / res["jac_local_4_points_us"]
    res["jac_dot_jdotv_over_jac"] = res["jac_dot_4_points_jdotv_us"] / res["jac_local_4_points_us"]
    res["centroidal_over_body_data_vel"] = res["centroidal_whole_model_us"] / res["body_data_vel_us"]
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
