"""Times mjl_inverse (continuous and discrete) beside mjl_forward on the same batch at 2048 envs with HIP events: per
launch one event pair, 50 warm-up launches, 300 timed, the median in microseconds. The states are random joint
angles and velocities with the pelvis lowered by 0 to 0.3 m, so a good part of the envs carry contact and limit
rows (the mean row count is reported). Writes profiles/inverse/cost.json (DESIGN.md "Inverse dynamics" quotes it).

    python tools/inverse_bench.py [--envs 2048] [--out profiles/inverse/cost.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inverse", "cost.json"))
    args = ap.parse_args()
    n = args.envs
    res = {"envs": n, "src_hash": build_info()["tree_src_hash"],
           "method": "HIP events around one launch, 50 warm-up, median of 300, microseconds"}
    for name in mjx_amd.BUILTIN_MODELS:
        m = mjx_amd.load_model(name)
        sys_ = mjx.put_model(m)
        d = mjx.make_data(sys_, n)
        rng = np.random.default_rng(0)
        q = np.tile(m.qpos0, (n, 1))
        q[:, 7:] += rng.uniform(-0.3, 0.3, (n, m.nq - 7))
        q[:, 2] -= rng.uniform(0.0, 0.3, n)
        d.set("qpos", torch.tensor(q, dtype=torch.float32))
        d.set("qvel", torch.tensor(rng.uniform(-1, 1, (n, m.nv)), dtype=torch.float32))
        d.set("ctrl", torch.tensor(rng.uniform(-1, 1, (n, m.nu)), dtype=torch.float32))
        mjx.forward(sys_, d)
        qacc = d.get("qacc").clone()
        out = (torch.empty_like(qacc), torch.empty_like(qacc))
        r = {"nv": m.nv, "mean_nefc": float(d.get("stats")[:, 1].mean())}
        # interleaved: forward, continuous, discrete, forward again
        r["forward_us"] = median_us(lambda: mjx.forward(sys_, d))
        r["inverse_us"] = median_us(lambda: mjx.inverse(sys_, d, qacc, out=out, with_constraint=True))
        r["inverse_discrete_us"] = median_us(lambda: mjx.inverse(sys_, d, qacc, discrete=True, out=out, with_constraint=True))
        r["forward_again_us"] = median_us(lambda: mjx.forward(sys_, d))
        res[name] = r
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
