"""The index arithmetic of the resident-factor operations (csrc/stmmqr_restables.cpp) alone, as a stand-alone program under
AddressSanitizer + UBSan (tests/restables_selftest.cpp): level tables, live panel counts, the row map, the transpose of Rj, the
carried view, the layout of the selected inverse and the resolution of covariance pairs, on hand-written trees.  No GPU, no HIP call:
the HIP headers are needed only for the types of csrc/stmmqr_device.h."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "stm-multifrontal-qr-factorization-empowered-by-gcn_amd" / "csrc"


def test_resident_tables_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    rocm = Path(os.environ.get("ROCM_PATH", "/opt/rocm"))
    if not (rocm / "include" / "hip" / "hip_runtime.h").exists():
        pytest.skip("no hip/hip_runtime.h")
    exe = tmp_path / "restables_selftest"
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-isystem", str(rocm / "include"), "-I", str(CSRC), "-o", str(exe),
           str(ROOT / "tests" / "restables_selftest.cpp"), str(CSRC / "stmmqr_restables.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and "asan" in b.stderr.lower() and "cannot find" in b.stderr.lower():
        pytest.skip("the sanitizer runtimes are not installed")
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60,
                       env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1", "PATH": "/usr/bin:/bin"})
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.strip().splitlines()[-1].endswith(" 0 failures")


def test_the_pure_part_makes_no_hip_call():
    """stmmqr_restables.* include stmmqr_device.h and the standard library only, and name neither the plan nor a device buffer"""
    for name in ("stmmqr_restables.h", "stmmqr_restables.cpp"):
        text = (CSRC / name).read_text()
        includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
        assert all(i.startswith("<") or i in ('"stmmqr_device.h"', '"stmmqr_restables.h"') for i in includes), includes
        code = "\n".join(ln.split("//")[0] for ln in text.splitlines())
        assert not any(w in code for w in ("hipMalloc", "hipMemcpy", "hipStream", "DevBuf", "stmmqr_plan")), name
