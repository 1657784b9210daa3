"""The planner (csrc/stmmqr_schedule.cpp, csrc/stmmqr_sched.h) alone, as a stand-alone program under AddressSanitizer + UBSan
(tests/schedule_selftest.cpp): schedules built as values from hand-written trees and from the symbolic analyses of golden fixtures,
under every grouping and setting that sends the builder down another path.  No GPU, no HIP call: the HIP headers are needed only for
the types of csrc/stmmqr_device.h."""
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from stmmqr_testlib import Symbolic, load_golden

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "stm-multifrontal-qr-factorization-empowered-by-gcn_amd" / "csrc"
FIXTURES = ("syn_grid3d", "grid20_standin", "epb1", "lns_3937", "dwt_992")


def write_tree(path, name):
    """the symbolic arrays the planner reads, as "key count values..." records"""
    S = Symbolic(load_golden(name))
    nf, n = S.sc["nf"], S.sc["n"]
    recs = {"nf": [nf], "n": [n], "maxstack": [max(S.sc["maxstack"], 0)], "do_rank": [S.sc["do_rank_detection"]], "keep_h": [S.sc.get("keepH", 1)],
            "Sleft": S.arr["Sleft"][:n + 2], "Super": S.arr["Super"][:nf + 1], "Rp": S.arr["Rp"][:nf + 1], "Hip": S.arr["Hip"][:nf + 1],
            "Child": S.arr["Child"][:nf + 1], "Childp": S.arr["Childp"][:nf + 2], "Post": S.arr["Post"][:nf], "Fm": S.arr["Fm"][:nf],
            "Rj": S.arr["Rj"][:S.sc["rjsize"]]}
    with open(path, "w") as fh:
        fh.write(f"name 0 {name}\n")
        for k, v in recs.items():
            v = np.asarray(v, dtype=np.int64).reshape(-1)
            fh.write(f"{k} {v.size} " + " ".join(map(str, v.tolist())) + "\n")


def test_schedules_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    rocm = Path(os.environ.get("ROCM_PATH", "/opt/rocm"))
    if not (rocm / "include" / "hip" / "hip_runtime.h").exists():
        pytest.skip("no hip/hip_runtime.h")
    exe = tmp_path / "schedule_selftest"
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-isystem", str(rocm / "include"), "-I", str(CSRC), "-o", str(exe),
           str(ROOT / "tests" / "schedule_selftest.cpp"), str(CSRC / "stmmqr_schedule.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and "asan" in b.stderr.lower() and "cannot find" in b.stderr.lower():
        pytest.skip("the sanitizer runtimes are not installed")
    assert b.returncode == 0, b.stderr[-3000:]
    files = []
    for name in FIXTURES:
        files.append(str(tmp_path / f"{name}.txt"))
        write_tree(files[-1], name)
    r = subprocess.run([str(exe)] + files, capture_output=True, text=True, timeout=120,
                       env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1", "PATH": "/usr/bin:/bin"})
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.strip().splitlines()[-1] == f"{4 + len(FIXTURES)} trees, 0 failures"


def test_the_planner_is_pure():
    """stmmqr_sched.h / stmmqr_schedule.cpp include stmmqr_device.h, stmmqr_knobs.h, stmmqr_recover.h, their own header and the standard
    library only, and name neither the plan, a device buffer, a HIP call, the options global, the environment nor `fail`"""
    allowed = ('"stmmqr_device.h"', '"stmmqr_knobs.h"', '"stmmqr_recover.h"', '"stmmqr_sched.h"')
    for name in ("stmmqr_sched.h", "stmmqr_schedule.cpp"):
        text = (CSRC / name).read_text()
        includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
        assert all(i.startswith("<") or i in allowed for i in includes), includes
        code = "\n".join(ln.split("//")[0] for ln in text.splitlines())
        bad = ("hipMalloc", "hipMemcpy", "hipMemset", "hipStream", "hipFree", "DevBuf", "stmmqr_plan", "g_opt", "getenv", "fail(", "knobs::once", "knobs::num",
               "knobs::value", "knobs::on(", "BuildKnobs::read")
        assert not any(w in code for w in bad), (name, [w for w in bad if w in code])
