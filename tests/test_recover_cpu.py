"""The recovery policy of the factorization driver (csrc/stmmqr_recover.h) alone, as a stand-alone program under AddressSanitizer +
UBSan (tests/recover_selftest.cpp): the classification of a finished pass, what the whole call, the phased begin,
stmmqr_plan_set_early_end and the group retry do after each outcome, and that the whole call's loop always ends.  No GPU, no HIP header."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "stm-multifrontal-qr-factorization-empowered-by-gcn_amd" / "csrc"


def test_recovery_policy_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "recover_selftest"
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", str(CSRC), "-o", str(exe), str(ROOT / "tests" / "recover_selftest.cpp")]
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


def test_the_policy_is_pure():
    """stmmqr_recover.h includes the standard library only and names neither HIP, the plan nor a device buffer"""
    text = (CSRC / "stmmqr_recover.h").read_text()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert all(i.startswith("<") and not i.startswith("<hip") for i in includes), includes
    code = "\n".join(ln.split("//")[0] for ln in text.splitlines())
    assert not any(w in code for w in ("hip", "DevBuf", "stmmqr_plan")), "stmmqr_recover.h"


def test_the_driver_keeps_no_recovery_flag_of_its_own():
    """the loose flags that the one outcome replaced stay gone from every unit, and the plan has no whole_call member
    (it is an argument of the driver's two internal entry points)"""
    for p in CSRC.iterdir():
        if p.suffix not in (".cpp", ".h", ".hip"):
            continue
        code = "\n".join(ln.split("//")[0] for ln in p.read_text().splitlines())
        for gone in ("panel_wait_failed", "early_end_failed", "arena_overflow", ".whole_call", "->whole_call"):
            assert gone not in code, (p.name, gone)
