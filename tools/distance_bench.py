"""What the geom distance readout costs: microseconds per mjl_geom_distance launch on humanoid_mjx at 64 and 2048
envs (states: random joint angles around qpos0), written to profiles/distance/cost.json:

    collision_pairs          the model's own collision pairs, dist / fromto / normal
    all_pairs, all_pairs_jac all 190 geom pairs, without and with the gradient
    composed_jac             the gradient rows of the 190 pairs as a user composes them today, in float32: two mjl_jac
                             launches (the `from` points on geom1's bodies, the `to` points on geom2's, 190 world
                             points each) and torch for normal' (jacp_to - jacp_from). The witness points and normals
                             are taken as given (this readout's), so the figure leaves out the closed forms a user
                             would also have to write in torch: a lower bound of the composed cost
    chunk_sweep              all_pairs and all_pairs_jac under MJL_OPT_DISTANCE_CHUNK = 16, 32, 64, 128, 65535 (one
                             wavefront per env), the measurement behind the library's default

Timing: each variant is captured in a graph of 10 calls; HIP events around one replay, 10 warm-up replays, the median of
50, divided by 10.

    python tools/distance_bench.py [--out profiles/distance/cost.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mujoco-mjx-lab_amd"))

import mjx_amd  # noqa: E402
from mjx_amd import abi, mjx  # noqa: E402
from mjx_amd._lib import build_info, check, lib  # noqa: E402

CALLS, WARM, REPLAYS = 10, 10, 50
CHUNKS = (16, 32, 64, 128, 65535)


def graph_us(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(CALLS):
            fn()
    for _ in range(WARM):
        g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPLAYS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / CALLS)
    return round(float(np.median(ts)), 2)


def bench(m, sys_, n):
    d = mjx.make_data(sys_, n)
    rng = np.random.default_rng(0)
    q = np.tile(m.qpos0, (n, 1))
    q[:, 7:] += rng.uniform(-0.3, 0.3, (n, m.nq - 7))
    d.set("qpos", torch.tensor(q, dtype=torch.float32))
    dev, nv = d.device, m.nv
    ids = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)

    def launch(g1, g2, with_jac):
        tabs = (ids(g1), ids(g2))
        p = len(g1)
        out = (torch.zeros((n, p), device=dev), torch.zeros((n, p, 6), device=dev), torch.zeros((n, p, 3), device=dev),
               torch.zeros((n, p, nv), device=dev) if with_jac else None)
        return (lambda: mjx.geom_distance(sys_, d, None, None, out=out, _dev=tabs)), out

    c1, c2 = mjx.collision_pairs(sys_)
    g1, g2 = zip(*[(a, b) for a in range(m.ngeom) for b in range(a + 1, m.ngeom)])
    res = {"npair_collision": len(c1), "npair_all": len(g1)}
    res["collision_pairs_us"] = graph_us(launch(c1, c2, False)[0])
    res["all_pairs_us"] = graph_us(launch(g1, g2, False)[0])
    fn, out = launch(g1, g2, True)
    res["all_pairs_jac_us"] = graph_us(fn)

    # the gradient composed from mjl_jac and torch, the witness points and normals given
    gb = m.arrays["geom_bodyid"]
    b1, b2 = ids([int(gb[g]) for g in g1]), ids([int(gb[g]) for g in g2])
    p = len(g1)
    frm, to, nrm = out[1][..., :3].contiguous(), out[1][..., 3:].contiguous(), out[2]
    jf, jt = torch.zeros((n, p, 3, nv), device=dev), torch.zeros((n, p, 3, nv), device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def composed():
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(lib().mjl_jac(d.handle, None, p, ptr(b1), abi.JAC_FRAME["world"], ptr(frm), ptr(jf), None, None, st))
        check(lib().mjl_jac(d.handle, None, p, ptr(b2), abi.JAC_FRAME["world"], ptr(to), ptr(jt), None, None, st))
        return torch.einsum("epi,epiv->epv", nrm, jt - jf)
    err = float((composed() - out[3]).abs().max())
    res["composed_jac_us"] = graph_us(composed)
    res["composed_jac_max_abs_diff"] = err
    sweep = {}
    for chunk in CHUNKS:
        d.set_option(abi.OPT_DISTANCE_CHUNK, chunk)
        sweep[str(chunk)] = {"all_pairs_us": graph_us(launch(g1, g2, False)[0]),
                             "all_pairs_jac_us": graph_us(launch(g1, g2, True)[0]),
                             "collision_pairs_us": graph_us(launch(c1, c2, False)[0])}
    d.set_option(abi.OPT_DISTANCE_CHUNK, 0)
    res["chunk_sweep"] = sweep
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distance", "cost.json"))
    args = ap.parse_args()
    m = mjx_amd.load_model("humanoid_mjx")
    sys_ = mjx.put_model(m)
    res = {"model": "humanoid_mjx", "nv": m.nv, "ngeom": m.ngeom, "src_hash": build_info()["tree_src_hash"],
           "method": f"graphs of {CALLS} calls, HIP events around one replay, {WARM} warm-up replays, median of "
                     f"{REPLAYS}, microseconds per call",
           "default_chunk": "MJL_OPT_DISTANCE_CHUNK = 0 (kDistChunk, csrc/capi.hip)",
           "envs": {str(n): bench(m, sys_, n) for n in (64, 2048)}}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
