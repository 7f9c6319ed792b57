"""Writes profiles/distance/tolerances.json (needs a GPU): the largest |dist|, witness point, normal and jac errors of
the built kernel against the float64 reference tests/distance_ref.py over the cases of
tests/test_distance_gpu.py::test_all_pairs_against_the_reference (its `measure`: both humanoids, 3 poses, all 190
pairs, uncapped and capped at 0.3 m; dist on every pair not within 1e-4 m of the cap, the rest on the non-degenerate
pairs), and the test bounds: four times the maxima, rounded up to one significant digit. Prints the file.

    python tools/distance_tolerances.py [profiles/distance/tolerances.json]
"""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "oracle", "mujoco-mjx-lab_amd", ""):
    sys.path.insert(0, os.path.join(ROOT, p))

import test_distance_gpu as tg  # noqa: E402


def up1(x):
    e = math.floor(math.log10(x))
    return math.ceil(x / 10 ** e - 1e-9) * 10 ** e


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "distance", "tolerances.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    meas = tg.measure()
    doc = {"note": "written by tools/distance_tolerances.py; see its docstring and tests/test_distance_gpu.py",
           "unit": "m (dist, point), 1 (normal), m per unit of qvel (jac)", "measured_max": meas}
    for k in tg.KEYS:
        doc[k + "_tol"] = up1(4 * max(v[k] for v in meas.values()))
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))
