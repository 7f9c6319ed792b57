"""Writes profiles/rays/tolerances.json (needs a GPU): the largest |dist - reference| and |hitpos - reference| of
the built kernel over the non-marginal rays of every case of tests/test_rays_gpu.py, against the float64 reference
tests/rays_ref.py, and the test bounds: four times the maxima, rounded up to one significant digit. Marginal rays
are taken at the distance bound, so the measurement is repeated once with the bound it found. Prints the file."""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "oracle", "mujoco-mjx-lab_amd", ""):
    sys.path.insert(0, os.path.join(ROOT, p))

import test_rays_gpu as tg  # noqa: E402


def up1(x):
    e = math.floor(math.log10(x))
    return math.ceil(x / 10 ** e - 1e-9) * 10 ** e


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "rays", "tolerances.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    for _ in range(2):
        meas = tg.measure()
        doc = {"note": "written by tools/ray_tolerances.py; see its docstring and tests/test_rays_gpu.py",
               "unit": "m", "measured_max": {k: {"dist": v[0], "hitpos": v[1]} for k, v in meas.items()},
               "dist_tol": up1(4 * max(v[0] for v in meas.values())),
               "hitpos_tol": up1(4 * max(v[1] for v in meas.values()))}
        with open(out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    print(json.dumps(doc))
