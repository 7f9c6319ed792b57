"""Writes profiles/sensors/tolerances.json: the tolerances of tests/test_sensors_gpu.py, computed on the CPU
from the test's own models, states and reference (tests/sensors_ref.py on the oracle). Per model and sensor
type: yardstick = max |reference formulas in numpy float32 - float64| over the test states, scale = max |value|
(at least 1), bound = max(8 x yardstick, 1e-6 x scale), inherited_max = the largest forward-pass term added
for an acc-stage value. tests/test_sensors.py compares the file with a fresh computation."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "oracle", "mujoco-mjx-lab_amd", ""):
    sys.path.insert(0, os.path.join(ROOT, p))

import test_sensors_gpu as tg  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sensors", "tolerances.json")
    doc = {"note": "written by tools/sensor_tolerances.py; see its docstring and tests/test_sensors_gpu.py",
           "models": tg.tolerance_table()}
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(out)
