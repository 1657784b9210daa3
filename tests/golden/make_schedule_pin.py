"""Pin of what the planner and the step scheduler do: the cases of tests/schedule_pin_cases.py as the build BEFORE the knob table
and the split of the host scheduler into units of its own runs them.  Calls only this package; needs a GPU.
Written once, on that build:  python tests/golden/make_schedule_pin.py
(The file lives in a directory of its own: every *.npz directly under tests/golden is a matrix fixture of the suites.)"""
import importlib
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from schedule_pin_cases import CASES, run_case  # noqa: E402

pkg = importlib.import_module("stm-multifrontal-qr-factorization-empowered-by-gcn_amd")
out = {}
for fixture, setting in CASES:
    out[f"{fixture}/{setting}"] = rec = run_case(pkg, fixture, setting)
    print(fixture, setting, *(f"{k}={rec[0][k]}/{rec[1][k]}" for k in ("nlaunch", "nsteps", "reschedules", "device_bytes")), flush=True)
dst = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "tests" / "golden" / "schedule_pin" / "schedule_pin_parent.json"
dst.parent.mkdir(parents=True, exist_ok=True)
dst.write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")
