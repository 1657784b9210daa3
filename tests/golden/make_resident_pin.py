"""Pin of the resident-factor operations: the cases of tests/resident_pin_cases.py as the build BEFORE the resident host layer was
split into units of its own computes them.  Calls only this package; needs a GPU.
Written once, on that build:  python tests/golden/make_resident_pin.py
Every case runs twice; an entry that does not reproduce is left out of the pin and named on the way, and nothing is written when an
entry is missing from one of the two runs."""
import importlib
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from resident_pin_cases import CASES, pack, run_case  # noqa: E402

pkg = importlib.import_module("stm-multifrontal-qr-factorization-empowered-by-gcn_amd")
out, dropped = {}, []
for name in CASES:
    a, b = run_case(pkg, name), run_case(pkg, name)
    if sorted(a) != sorted(b):
        sys.exit(f"{name}: the two runs produced different entries; nothing written")
    dropped += [f"{name}/{k}" for k in a if not np.array_equal(a[k], b[k])]
    out.update(pack(name, {k: v for k, v in a.items() if np.array_equal(v, b[k])}))
    print(name, len(a), "entries, rank", int(a["rank"]), "device bytes", float(a["device_bytes/factorized"]), float(a["device_bytes/after"]))
for k in dropped:
    print("NOT REPRODUCIBLE, left out:", k)
dst = ROOT / "tests" / "golden" / "resident_pin" / "resident_pin_parent.npz"
dst.parent.mkdir(exist_ok=True)
np.savez_compressed(dst, **out)
print("wrote", dst, dst.stat().st_size, "bytes,", len(dropped), "entries left out")
