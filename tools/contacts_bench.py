"""What the contact readout costs: mjl_forward against mjl_forward_contacts (every output on, max_con =
ncon_max, caller-owned buffers) at 2048 envs of humanoid_mjx, on two kinds of state:

  standing   every env at the normal_stand keyframe
  contacts   the mix of the parity tests' states: a stand with joint noise, a height offset and random
             velocities, then env % 60 steps of random controls (landing, stumbling and falling
             bodies, 0 to 8 contacts per env; the counts are recorded)

Also timed, to split the difference: mjl_forward with MJL_OPT_FORCE_GLOBAL_ROWS (the forward launch
mjl_forward_contacts makes), so readout kernel = forward_contacts - forward_global_rows.
HIP events on the launch stream, 200 calls after 20, three interleaved rounds per variant, medians
reported. Every call starts from the qacc_warmstart the call before it left (a forward pass stores its
solution there), so all variants time the same warm-started solve. Writes
profiles/contacts/contacts_bench.json (or the path given) and prints it."""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mujoco-mjx-lab_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mjx_amd  # noqa: E402
from mjx_amd import _lib, abi, mjx  # noqa: E402

B, CALLS, WARMUP, ROUNDS = 2048, 200, 20, 3


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
    m = mjx_amd.load_model("humanoid_mjx")
    sys_ = mjx.put_model(m)
    L, mc = _lib.lib(), sys_.ncon_max
    stand = torch.tensor(np.tile(m.key_qpos[m.names["key"].index("normal_stand")], (B, 1)), dtype=torch.float32)
    res = {"envs": B, "model": "humanoid_mjx", "max_con": mc, "calls": CALLS, "warmup": WARMUP, "rounds": ROUNDS,
           "unit": "us per call (HIP events)", "build": _lib.build_info(), "states": {}}
    for kind in ("standing", "contacts"):
        d = mjx.make_data(sys_, B)
        d.set("qpos", stand)
        if kind == "contacts":
            g = torch.Generator(device="cuda").manual_seed(0)
            rand = lambda n, lo, hi: torch.rand((B, n), generator=g, device="cuda") * (hi - lo) + lo
            q = stand.cuda()
            q[:, 7:] += rand(m.nq - 7, -0.3, 0.3)
            q[:, 2:3] += rand(1, -0.25, 0.05)
            d.set("qpos", q)
            d.set("qvel", rand(m.nv, -1, 1))
            keep = {f: d.get(f) for f in ("qpos", "qvel", "qacc_warmstart")}
            nstep = (torch.arange(B, device="cuda") % 60).unsqueeze(1)
            for t in range(1, 60):  # env e keeps its state after e % 60 steps
                mjx.step(sys_, d, rand(m.nu, -1, 1))
                for f in keep:
                    keep[f] = torch.where(nstep == t, d.get(f), keep[f])
            for f in keep:
                d.set(f, keep[f])
        dev = d.device
        i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
        f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
        bufs = [i32(B), i32(B, mc, 2), i32(B, mc), i32(B, mc), f32(B, mc), f32(B, mc, 3), f32(B, mc, 9), f32(B, mc, 3),
                f32(B, sys_.nbody, 3)]
        ptrs = [C.c_void_p(t.data_ptr()) for t in bufs]
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def forward(global_rows):
            d.set_option(abi.OPT_FORCE_GLOBAL_ROWS, global_rows)
            t = timed(lambda: _lib.check(L.mjl_forward(d.handle, None, stream)))
            d.set_option(abi.OPT_FORCE_GLOBAL_ROWS, 0)
            return t

        def contacts():
            return timed(lambda: _lib.check(L.mjl_forward_contacts(d.handle, None, mc, *ptrs, stream)))

        variants = {"forward": lambda: forward(0), "forward_global_rows": lambda: forward(1), "forward_contacts": contacts}
        runs = {k: [] for k in variants}
        for _ in range(ROUNDS):  # interleaved
            for k, fn in variants.items():
                runs[k].append(fn())
        ncon = bufs[0].cpu().numpy()
        nefc = d.get("stats").cpu().numpy()[:, 1]
        r = {k: {"median": round(statistics.median(v), 2), "runs": [round(x, 2) for x in v]} for k, v in runs.items()}
        r["ncon_mean"], r["ncon_max"] = round(float(ncon.mean()), 2), int(ncon.max())
        r["nefc_mean"] = round(float(nefc.mean()), 2)
        res["states"][kind] = r
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "contacts", "contacts_bench.json"))
