"""Times mjl_step_jacobian (tangent layout, A and B) for every candidate number of row groups per env, and beside it
what the library offered before: nq + nv launches of mjl_step_vjp with one-hot cotangents resident on the device,
writing into preallocated outputs. Both run in this process on the same batch of contact states (random joint angles
and velocities, the pelvis lowered by 0 to 0.3 m; the mean row count is reported) of humanoid_mjx at 64, 512 and
2048 envs. HIP events around each whole call (the loop: around all its launches), warm-up first, the median in
microseconds; the candidates and the loop are interleaved round by round. Writes profiles/linearize/cost.json
(DESIGN.md "Linearization" quotes it).

    python tools/linearize_bench.py [--envs 64 512 2048] [--resource-usage FILE] [--out profiles/linearize/cost.json]

--resource-usage: the text `make -C mujoco-mjx-lab_amd/csrc resource-usage` prints; the linearize kernels' register,
LDS and scratch figures are copied from it into the JSON.
"""
import argparse
import json
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mujoco-mjx-lab_amd"))

import mjx_amd  # noqa: E402
from mjx_amd import abi, mjx  # noqa: E402
from mjx_amd._lib import build_info, check, lib  # noqa: E402

GROUPS = (1, 2, 4, 8, 16)
RULE = "G = clamp(floor(SIMDs / nenv), 1, 16), SIMDs = 4 x CUs of the device"


def timed_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def resource_usage(path):
    """{kernel dims: {VGPRs, AGPRs, ...}} of the linearize kernels out of hipcc's kernel-resource-usage remarks."""
    out, cur = {}, None
    for line in open(path):
        k = re.search(r"Function Name: (\S+)", line)
        if k:
            name = k.group(1)
            cur = None
            if "linearize_kernel" in name:
                cur = out.setdefault("DGen" if "Li32ELi32ELi32ELi32E" in name else "DHumV", {})
            continue
        f = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass", line)
        if cur is not None and f:
            cur[f.group(1).strip()] = f.group(2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[64, 512, 2048])
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--resource-usage", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linearize", "cost.json"))
    args = ap.parse_args()
    m = mjx_amd.load_model("humanoid_mjx")
    sys_ = mjx.put_model(m)
    nq, nv, nu = m.nq, m.nv, m.nu
    res = {"model": "humanoid_mjx", "nq": nq, "nv": nv, "nu": nu, "src_hash": build_info()["tree_src_hash"],
           "device": torch.cuda.get_device_name(0), "rule": RULE, "groups_tried": list(GROUPS),
           "method": "HIP events around one whole call (the baseline: around its nq + nv launches), 3 warm-up rounds, "
                     f"median of {args.rounds} interleaved rounds, microseconds",
           "baseline": f"{nq + nv} launches of mjl_step_vjp, one-hot cotangents and outputs resident on the device",
           "sizes": {}}
    if args.resource_usage:
        res["resource_usage"] = resource_usage(args.resource_usage)
    L = lib()
    for n in args.envs:
        d = mjx.make_data(sys_, n)
        rng = np.random.default_rng(0)
        q = np.tile(m.qpos0, (n, 1))
        q[:, 7:] += rng.uniform(-0.3, 0.3, (n, nq - 7))
        q[:, 2] -= rng.uniform(0.0, 0.3, n)
        d.set("qpos", torch.tensor(q, dtype=torch.float32))
        d.set("qvel", torch.tensor(rng.uniform(-1, 1, (n, nv)), dtype=torch.float32))
        d.set("ctrl", torch.tensor(rng.uniform(-1, 1, (n, nu)), dtype=torch.float32))
        mjx.forward(sys_, d)
        r = {"mean_nefc": float(d.get("stats")[:, 1].mean())}
        A = torch.empty((n, 2 * nv, 2 * nv), device="cuda")
        B = torch.empty((n, 2 * nv, nu), device="cuda")
        # the baseline's inputs and outputs: row i of `hot` is cotangent i for every env
        hot = torch.eye(nq + nv, device="cuda").unsqueeze(1).expand(-1, n, -1)
        gq, gv = hot[:, :, :nq].contiguous(), hot[:, :, nq:].contiguous()
        oq, ov = torch.empty((nq + nv, n, nq), device="cuda"), torch.empty((nq + nv, n, nv), device="cuda")
        oc = torch.empty((nq + nv, n, nu), device="cuda")
        P, st = mjx._ptr, mjx._stream()

        def loop():
            for i in range(nq + nv):
                check(L.mjl_step_vjp(d.handle, P(gq[i]), P(gv[i]), P(oq[i]), P(ov[i]), P(oc[i]), st))

        def lin(g):
            d.set_option(abi.OPT_LINEARIZE_GROUPS, g)
            mjx.transition(sys_, d, out=(A, B))

        cands = [("loop", loop)] + [(f"G{g}", (lambda g=g: lin(g))) for g in GROUPS + (0,)]
        ts = {k: [] for k, _ in cands}
        for rnd in range(3 + args.rounds):
            for k, fn in cands:
                t = timed_us(fn)
                if rnd >= 3:
                    ts[k].append(t)
        med = {k: float(np.median(v)) for k, v in ts.items()}
        r["step_vjp_loop_us"] = med["loop"]
        r["step_jacobian_us"] = {str(g): med[f"G{g}"] for g in GROUPS}
        r["step_jacobian_rule_us"] = med["G0"]
        r["rule_groups"] = max(1, min(16, 4 * torch.cuda.get_device_properties(0).multi_processor_count // n))
        r["best_groups"] = int(min(GROUPS, key=lambda g: med[f"G{g}"]))
        r["loop_over_rule"] = med["loop"] / med["G0"]
        r["rule_ns_per_env_row"] = 1e3 * med["G0"] / (n * 2 * nv)
        # the same matrices by both routes (raw layout, where the loop's rows are the entry's)
        Jr = mjx.step_jacobian(sys_, d)
        loop()
        torch.cuda.synchronize()
        ref = torch.cat([oq, ov, oc], 2).transpose(0, 1)
        r["max_abs_diff_vs_loop"] = float((Jr - ref).abs().max())
        r["max_abs_loop"] = float(ref.abs().max())
        res["sizes"][str(n)] = r
        print(n, json.dumps(r), flush=True)
    res["faster_than_loop"] = {k: v["loop_over_rule"] > 1.0 for k, v in res["sizes"].items()}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
