"""Times mjl_ik beside the same algorithm composed from torch ops (per iteration: Data.set of the iterate,
mjx.jac_local, the normal equations by einsum, torch.linalg.solve, the quaternion update), on the humanoid with 4
position tasks (the two foot sites and two points fixed in the hands: the model has two sites) and 20 iterations, at
64 and 2048 envs, with HIP events: 5 warm-up solves, the median of 30 (torch loop) / 50 warm-up, 300 timed (mjl_ik),
in microseconds per solve. Also the largest difference between the two solutions. Writes profiles/ik/cost.json
(DESIGN.md "Inverse kinematics" quotes it).

    python tools/ik_bench.py [--envs 64 2048] [--out profiles/ik/cost.json]
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

ITERATIONS, DAMPING = 20, 1e-3


def torch_ik(sys_, scratch, frames, tabs, jout, target, start, iterations, damping):
    """mjl_ik's iteration (position tasks, unit weights, no posture, no step bound, no limits) from torch ops."""
    q = start.clone()
    eye = damping * torch.eye(sys_.nv, device=q.device)
    for _ in range(iterations):
        scratch.set("qpos", q)
        jp, _, x = mjx.jac_local(sys_, scratch, frames, out=jout, _dev=tabs)
        J = jp.reshape(q.shape[0], -1, sys_.nv)
        e = (target - x).reshape(q.shape[0], -1)
        H = torch.einsum("erv,erw->evw", J, J) + eye
        g = torch.einsum("erv,er->ev", J, e)
        dq = torch.linalg.solve(H, g)
        w = dq[:, 3:6]
        nrm = w.norm(dim=1, keepdim=True)
        half = 0.5 * nrm
        qr = torch.cat([torch.cos(half), torch.sin(half) * w / nrm.clamp_min(1e-30)], dim=1)
        quat = mjx._qmul_t(q[:, 3:7], qr)
        q = torch.cat([q[:, :3] + dq[:, :3], quat / quat.norm(dim=1, keepdim=True), q[:, 7:] + dq[:, 6:]], dim=1)
    return q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[64, 2048])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ik", "cost.json"))
    args = ap.parse_args()
    m = mjx_amd.load_model("humanoid_mjx")
    sys_ = mjx.put_model(m)
    frames = [("site", 0), ("site", 1), "hand_right", "hand_left"]
    offset = np.array([[0, 0, 0], [0, 0, 0], [0.05, 0, 0.02], [0.05, 0, 0.02]], np.float64)
    res = {"model": "humanoid_mjx", "nv": m.nv, "tasks": 4, "iterations": ITERATIONS, "damping": DAMPING,
           "src_hash": build_info()["tree_src_hash"],
           "method": "HIP events around one solve, median, microseconds; position tasks, limits off"}
    for n in args.envs:
        rng = np.random.default_rng(0)
        qstar = np.tile(m.qpos0, (n, 1))
        qstar[:, 7:] += rng.uniform(-0.3, 0.3, (n, m.nq - 7))
        start = qstar.copy()
        start[:, :3] += rng.uniform(-0.03, 0.03, (n, 3))
        start[:, 7:] += rng.uniform(-0.1, 0.1, (n, m.nq - 7))
        d, scratch = mjx.make_data(sys_, n), mjx.make_data(sys_, n)
        dev = d.device
        d.set("qpos", torch.tensor(qstar, dtype=torch.float32))
        bodies, local, conj, _ = mjx.ik_tables(sys_, frames, offset)
        tabs = (torch.tensor(bodies, dtype=torch.int32, device=dev), torch.tensor(local, device=dev))
        itabs = tabs + (None if conj is None else torch.tensor(conj, device=dev), None)
        jout = mjx.jac_local(sys_, d, frames, _dev=tabs)
        target = jout[2].clone()
        q0 = torch.tensor(start, dtype=torch.float32, device=dev)
        out = mjx.ik(sys_, d, frames, target, qpos_start=q0, iterations=ITERATIONS, damping=DAMPING, limits=False, _dev=itabs)
        run = lambda: mjx.ik(sys_, d, frames, target, qpos_start=q0, iterations=ITERATIONS, damping=DAMPING, limits=False,
                             out=out, _dev=itabs)
        ref = torch_ik(sys_, scratch, frames, tabs, jout, target, q0, ITERATIONS, DAMPING)
        r = {"mjl_ik_us": median_us(run),
             "torch_loop_us": median_us(lambda: torch_ik(sys_, scratch, frames, tabs, jout, target, q0, ITERATIONS, DAMPING),
                                        warm=5, n=30),
             "max_abs_qpos_difference": float((out.qpos - ref).abs().max()),
             "max_residual_m": float(out.err[:, :, :3].norm(dim=2).max())}
        r["torch_loop_over_mjl_ik"] = r["torch_loop_us"] / r["mjl_ik_us"]
        res[f"envs_{n}"] = r
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
