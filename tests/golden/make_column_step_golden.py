"""Pin of the column pipeline's results: qr_front on the fronts of tests/column_step_cases.py (GOLDEN), as the build
BEFORE the column step lost its memory waits and row masks computes them.  Calls only this package; needs a GPU.
Written once, on that build:  python tests/golden/make_column_step_golden.py
(The file lives in a directory of its own: every *.npz directly under tests/golden is a matrix fixture of the suites.)
Kept per case: Tau, Stair, Rdead, the first rows of F and one SHA-256 digest per column of its other in-staircase entries."""
import importlib
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from column_step_cases import GOLDEN, golden_case, pin, run_front  # noqa: E402

pkg = importlib.import_module("stm-multifrontal-qr-factorization-empowered-by-gcn_amd")
out = {}
for name in GOLDEN:
    (F0, St0), npiv, tol, ntol, dbg = golden_case(name)
    if dbg is not None:
        os.environ["STMMQR_DBG"] = str(dbg)
    try:
        r, Tau, Rdead, fl, F, St = run_front(pkg, F0, St0, npiv, tol, ntol)
    finally:
        os.environ.pop("STMMQR_DBG", None)
    head, dig = pin(F, St0, St)
    out[name + "_rank"], out[name + "_flops"] = r, fl
    out[name + "_Tau"], out[name + "_Stair"], out[name + "_Rdead"] = Tau, St, Rdead
    out[name + "_head"], out[name + "_digest"] = head, dig
    print(name, "rank", r, "flops", fl)
dst = ROOT / "tests" / "golden" / "column_step" / "column_step_parent.npz"
dst.parent.mkdir(exist_ok=True)
np.savez_compressed(dst, **out)
