"""The byte offsets compiled into the library for the reference's sparse_common equal offsetof() in the real header, and the
library's mirrors of sparse_csc / qr_symbolic / qr_numeric have the real header's sizes.  The real header's layout is recorded
in tests/golden/api/abi_layout.json (generator: tests/golden/make_abi_golden.py, run on a checkout of the reference)."""
import ctypes as C
import importlib
import json
import subprocess
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
GOLD = json.loads((ROOT / "tests" / "golden" / "api" / "abi_layout.json").read_text())

FIELDS = ["status", "malloc_count", "memory_usage", "memory_inuse", "blas_ok", "SPQR_grain", "SPQR_small",
          "SPQR_shrink", "SPQR_flopcount", "SPQR_flopcount_bound"]


def test_common_layout_matches_reference_header():
    pkg = importlib.import_module("stm-multifrontal-qr-factorization-empowered-by-gcn_amd")

    class L(C.Structure):
        _fields_ = [(f, C.c_size_t) for f in FIELDS]
    lay = L()
    pkg.lib.stmmqr_get_common_layout(C.byref(lay))
    assert [getattr(lay, f) for f in FIELDS] == [GOLD["offsetof_sparse_common"][f] for f in FIELDS]

    src = '#include <stdio.h>\n#include "stmmqr_hip.h"\nint main(){printf("%zu %zu %zu\\n", sizeof(stm_sparse_csc),' \
          ' sizeof(stm_qr_symbolic), sizeof(stm_qr_numeric));return 0;}\n'
    with tempfile.TemporaryDirectory() as td:
        (Path(td) / "t.c").write_text(src)
        subprocess.check_call(["gcc", "-I", str(ROOT / "include"), str(Path(td) / "t.c"), "-o", str(Path(td) / "t")])
        out = subprocess.check_output([str(Path(td) / "t")]).decode().split()
    assert [int(x) for x in out] == [GOLD["sizeof"][s] for s in ("sparse_csc", "qr_symbolic", "qr_numeric")] == [88, 272, 192]
