"""Times mjl_ik_wb beside mjl_ik with the frame tasks alone and beside the same whole-body iteration composed from
the readouts (per iteration: Data.set of the iterate, mjx.jac_local, mjx.body_data's subtree_com, mjx.jac_subtree_com,
mjx.geom_distance with its gradient, the normal equations by einsum, torch.linalg.solve, the quaternion update), on
the humanoid with tools/ik_bench.py's 4 position tasks, the whole-model CoM in xy and the model's foot - floor and
arm - torso pairs (12 pairs), 20 iterations, at 64 and 2048 envs, with HIP events: the median in microseconds per
solve (50 warm-up, 300 timed for the kernels; 5 and 30 for the composed loop). Also how far the kernel and the
composed loop agree. Writes profiles/ik/wb_cost.json (DESIGN.md "Whole-body IK" quotes it).

    python tools/ik_wb_bench.py [--envs 64 2048] [--out profiles/ik/wb_cost.json]
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
FEET = ["foot1_right", "foot2_right", "foot1_left", "foot2_left"]
ARMS = ["lower_arm_right", "hand_right", "lower_arm_left", "hand_left"]
TORSO = ["torso", "waist_upper"]
FLOOR_MIN, BODY_MIN = 0.005, 0.02  # m


def composed(sys_, scratch, frames, tabs, jout, target, com_target, pairs, cmin, start, iterations, damping):
    """mjl_ik_wb's iteration (unit weights, CoM in xy, no posture, no step bound, no limits) from the readouts."""
    q = start.clone()
    eye = damping * torch.eye(sys_.nv, device=q.device)
    for _ in range(iterations):
        scratch.set("qpos", q)
        jp, _, x = mjx.jac_local(sys_, scratch, frames, out=jout, _dev=tabs)
        com = mjx.body_data(sys_, scratch, fields=("subtree_com",)).subtree_com[:, 0]
        jc = mjx.jac_subtree_com(sys_, scratch, 0)[:, 0, :2]
        gd = mjx.geom_distance(sys_, scratch, None, None, with_jac=True, _dev=pairs)
        on = (gd.dist < cmin).float()
        J = torch.cat([jp.reshape(q.shape[0], -1, sys_.nv), jc, gd.jac * on.unsqueeze(2)], dim=1)
        e = torch.cat([(target - x).reshape(q.shape[0], -1), (com_target - com)[:, :2], (cmin - gd.dist) * on], dim=1)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ik", "wb_cost.json"))
    args = ap.parse_args()
    m = mjx_amd.load_model("humanoid_mjx")
    sys_ = mjx.put_model(m)
    frames = [("site", 0), ("site", 1), "hand_right", "hand_left"]
    offset = np.array([[0, 0, 0], [0, 0, 0], [0.05, 0, 0.02], [0.05, 0, 0.02]], np.float64)
    g1 = ["floor"] * len(FEET) + [t for t in TORSO for _ in ARMS]
    g2 = FEET + ARMS * len(TORSO)
    cmin_host = [FLOOR_MIN] * len(FEET) + [BODY_MIN] * (len(ARMS) * len(TORSO))
    res = {"model": "humanoid_mjx", "nv": m.nv, "tasks": 4, "pairs": len(g1), "com": "whole model, weights (1, 1, 0)",
           "iterations": ITERATIONS, "damping": DAMPING, "src_hash": build_info()["tree_src_hash"],
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
        wtabs = mjx.ik_wb_tables(sys_, 0, [1, 1, 0], (g1, g2), cmin_host)
        pairs = tuple(torch.tensor(x, dtype=torch.int32, device=dev) for x in wtabs[2:4])
        cmin = torch.tensor(wtabs[4], device=dev)
        jout = mjx.jac_local(sys_, d, frames, _dev=tabs)
        target = jout[2].clone()
        com_target = mjx.body_data(sys_, d, fields=("subtree_com",)).subtree_com[:, 0].clone()
        q0 = torch.tensor(start, dtype=torch.float32, device=dev)
        kw = dict(qpos_start=q0, iterations=ITERATIONS, damping=DAMPING, limits=False)
        out = mjx.ik(sys_, d, frames, target, _dev=itabs, **kw)
        wout = mjx.ik_wb(sys_, d, frames, target, com_target=com_target, _dev=(itabs, wtabs), **kw)
        ref = composed(sys_, scratch, frames, tabs, jout, target, com_target, pairs, cmin, q0, ITERATIONS, DAMPING)
        r = {"mjl_ik_wb_us": median_us(lambda: mjx.ik_wb(sys_, d, frames, target, com_target=com_target, out=wout,
                                                         _dev=(itabs, wtabs), **kw)),
             "mjl_ik_us": median_us(lambda: mjx.ik(sys_, d, frames, target, out=out, _dev=itabs, **kw)),
             "composed_loop_us": median_us(lambda: composed(sys_, scratch, frames, tabs, jout, target, com_target, pairs, cmin,
                                                            q0, ITERATIONS, DAMPING), warm=5, n=30),
             "max_abs_qpos_difference_kernel_vs_composed": float((wout.qpos - ref).abs().max()),
             "envs_within_1e-4_of_composed": int(((wout.qpos - ref).abs().amax(dim=1) < 1e-4).sum()),
             "max_residual_m": float(wout.err[:, :, :3].norm(dim=2).max()),
             "max_com_err_m": float(wout.com_err.abs().max()),
             "min_clearance_minus_clear_min_m": float((wout.clearance - cmin).min()),
             "pairs_active_at_start": float((mjx.ik_wb(sys_, d, frames, target, com_target=com_target, _dev=(itabs, wtabs),
                                                       **dict(kw, iterations=0)).clearance < cmin).float().sum(dim=1).mean())}
        r["mjl_ik_wb_over_mjl_ik"] = r["mjl_ik_wb_us"] / r["mjl_ik_us"]
        r["composed_loop_over_mjl_ik_wb"] = r["composed_loop_us"] / r["mjl_ik_wb_us"]
        res[f"envs_{n}"] = r
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
