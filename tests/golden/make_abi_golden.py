#!/usr/bin/env python3
"""Generate tests/golden/api/abi_layout.json: offsetof() of the sparse_common fields the library reads and writes, and
sizeof() of sparse_csc / qr_symbolic / qr_numeric, as the REFERENCE's own header SparseQR.h lays them out on x86-64
(gcc -DDLONG, the flags of oracle/Makefile).  Needs a checkout of the reference's STMMQR directory:
    python tests/golden/make_abi_golden.py PATH/TO/STMMQR
tests/test_abi_layout.py compares the library's compiled-in layout with this record."""
import json
import subprocess
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parent
OUT = HERE / "api" / "abi_layout.json"
FIELDS = ["status", "malloc_count", "memory_usage", "memory_inuse", "blas_ok", "SPQR_grain", "SPQR_small",
          "SPQR_shrink", "SPQR_flopcount", "SPQR_flopcount_bound"]
STRUCTS = ["sparse_csc", "qr_symbolic", "qr_numeric"]


def main():
    if len(sys.argv) != 2 or not (Path(sys.argv[1]) / "include" / "SparseQR.h").exists():
        sys.exit("usage: make_abi_golden.py PATH/TO/STMMQR (the directory holding include/SparseQR.h)")
    ref = Path(sys.argv[1]).resolve()
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"SparseQR.h\"\nint main(){\n" + \
          "".join(f'printf("%zu\\n", offsetof(sparse_common,{f}));\n' for f in FIELDS) + \
          "".join(f'printf("%zu\\n", sizeof({s}));\n' for s in STRUCTS) + "return 0;}\n"
    with tempfile.TemporaryDirectory() as td:
        (Path(td) / "p.c").write_text(src)
        subprocess.check_call(["gcc", "-std=gnu99", "-fcommon", "-w", "-DDLONG", f"-I{ref}/include", f"-I{ref}/include/tpsm",
                               str(Path(td) / "p.c"), "-o", str(Path(td) / "p")])
        out = [int(x) for x in subprocess.check_output([str(Path(td) / "p")]).decode().split()]
    rec = {"offsetof_sparse_common": dict(zip(FIELDS, out[:len(FIELDS)])), "sizeof": dict(zip(STRUCTS, out[len(FIELDS):]))}
    OUT.write_text(json.dumps(rec, indent=1) + "\n")
    print("wrote", OUT, rec)


if __name__ == "__main__":
    main()
