"""Times mjl_jac and mjl_mass_matrix beside the pos-only mjl_body_data launch at 2048 envs with HIP events: per
launch one event pair, 50 warm-up launches, 300 timed, the median in microseconds. Writes profiles/dyn/cost.json
(DESIGN.md "Jacobians and mass matrix" quotes it).

    python tools/dyn_bench.py [--envs 2048] [--out profiles/dyn/cost.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mujoco-mjx-lab_amd"))

import mjx_amd  # noqa: E402
from mjx_amd import mjx  # noqa: E402
from mjx_amd._lib import build_info  # noqa: E402


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dyn", "cost.json"))
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
    pos = ("xipos", "ximat", "subtree_com", "cinert")
    bd = mjx.body_data(sys_, d, pos)
    res["body_data_pos_us"] = median_us(lambda: mjx.body_data(sys_, d, pos, out=bd))
    for npt in (4, 32):
        frames = [("xbody", 1 + k % (m.nbody - 1)) for k in range(npt)]
        bodies, local = mjx.jac_frames(sys_, frames, [0.05, 0.0, 0.1])
        tabs = (torch.tensor(bodies, dtype=torch.int32, device=dev), torch.tensor(local, device=dev))
        out = mjx.jac_local(sys_, d, frames, _dev=tabs)
        res[f"jac_local_{npt}_points_us"] = median_us(lambda: mjx.jac_local(sys_, d, frames, out=out, _dev=tabs))
    M = mjx.full_m(sys_, d)
    res["full_m_us"] = median_us(lambda: mjx.full_m(sys_, d, out=M))
    for nvec in (1, 8):
        v = torch.tensor(rng.uniform(-1, 1, (n, nvec, m.nv)), dtype=torch.float32, device=dev)
        x = torch.empty_like(v)
        res[f"solve_m_{nvec}_vec_us"] = median_us(lambda: mjx.solve_m(sys_, d, v, out=x))
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
