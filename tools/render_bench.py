"""Throughput of mjl_render_qpos (both launches: frame set-up + ray cast), timed with device events.

    python tools/render_bench.py [--out profiles/r11/render_bench.json] [--iters 20] [--repeats 5]

Two shapes, each with and without shadows, on humanoid_mjx through `side_view`, all three outputs:
    pixel observations   2048 frames of 64 x 64
    video                64 frames of 640 x 480
Poses: qpos0 with every hinge moved by a seeded uniform draw inside +-0.3 rad, a different one per frame.
Reports per case the median time of a call over `repeats` windows of `iters` calls (after a warm-up of
the same shape), primary rays per second, and the share of the FP32 vector peak (157.3 TFLOP/s) that
the counted arithmetic amounts to. The count (operations per ray-geom test, read off
csrc/render_kernels.hip's ray_geom, one per add / multiply / compare-select, divide and sqrt as one):
    plane     3 (offset) + 5 + 5 + 2 (two dot products, negate, divide) + 2 (range)               = 17
    sphere    3 + 6 (closest approach) + 6 (offset there) + 7 (r^2 - |q|^2) + 3 (sqrt, roots) + 2 = 27
    capsule   3 + 54 (axial split 22, side quadratic 27, axial test 3, range 2) + 2 x 31 (caps)   = 119
A primary ray runs one test per geom; with shadows every pixel that hits a geom runs a second loop.
Set-up, shading and stores are not counted, so the share is a lower bound of the arithmetic done.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mujoco-mjx-lab_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import mjx_amd  # noqa: E402
from mjx_amd import _lib, mjcf, mjx  # noqa: E402
from mjx_amd.render import Renderer  # noqa: E402

FLOPS_PER_TEST = {mjcf.GEOM_PLANE: 17, mjcf.GEOM_SPHERE: 27, mjcf.GEOM_CAPSULE: 119}
PEAK_FP32 = 157.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "render_bench.json"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("render_bench needs a GPU: timings are not taken on the CPU")
    m = mjx_amd.load_model("humanoid_mjx")
    sys_ = mjx.put_model(m)
    flops_ray = int(sum(FLOPS_PER_TEST[int(t)] for t in m.arrays["geom_type"]))
    rng = np.random.default_rng(11)
    cases = []
    for label, n, W, H in (("pixel_obs", 2048, 64, 64), ("video", 64, 640, 480)):
        q = np.tile(m.qpos0, (n, 1))
        q[:, 7:] += rng.uniform(-0.3, 0.3, (n, m.nq - 7))
        q = torch.tensor(q, dtype=torch.float32, device="cuda")
        r = Renderer(sys_, n)
        for shadows in (False, True):
            run = lambda: r.render(q, "side_view", W, H, shadows=shadows, depth=True, seg=True)  # noqa: E731
            out = run()
            hit_share = float((out.seg >= 0).float().mean())
            for _ in range(3):
                run()
            torch.cuda.synchronize()
            ms = []
            for _ in range(a.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    run()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1) / a.iters)
            t = float(np.median(ms)) * 1e-3
            rays = n * W * H
            flops = rays * flops_ray * (1.0 + (hit_share if shadows else 0.0))
            cases.append({"case": label, "frames": n, "width": W, "height": H, "shadows": shadows,
                          "ms_per_call_median": round(t * 1e3, 4), "ms_per_call_min": round(min(ms), 4),
                          "ms_per_call_max": round(max(ms), 4), "rays_per_s": round(rays / t, 1),
                          "hit_pixel_share": round(hit_share, 4), "counted_flops_per_primary_ray": flops_ray,
                          "counted_tflops": round(flops / t / 1e12, 3),
                          "fp32_vector_peak_share": round(flops / t / PEAK_FP32, 4)})
    line = {"bench": "render_qpos", "model": "humanoid_mjx", "camera": "side_view", "ngeom": int(m.ngeom),
            "outputs": "rgb+depth+seg", "iters": a.iters, "repeats": a.repeats, "timing": "device events, includes the "
            "output allocation of Renderer.render", "device": torch.cuda.get_device_name(0),
            "lib_src_hash": _lib.build_info()["lib_src_hash"], "cases": cases}
    s = json.dumps(line)
    print(s)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(s + "\n")


if __name__ == "__main__":
    main()
