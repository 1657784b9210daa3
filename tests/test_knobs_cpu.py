"""The table of environment knobs (csrc/stmmqr_knobs.h) alone, as a stand-alone program under AddressSanitizer + UBSan
(tests/knobs_selftest.cpp): every row's default and override, the reading rules, and the hipGraph key of RunKnobs, which must move
with every knob that a run of the schedule reads.  And: the table is the only place of the library that reads STMMQR_* variables."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "stm-multifrontal-qr-factorization-empowered-by-gcn_amd" / "csrc"
# stmmqr_qrtest.cpp is a program of its own (STMMQR_REFERENCE_LIB, STMMQR_QRTEST_VERBOSE); stmmqr_multi.cpp looks up the name of
# the RCCL library where it loads it (STMMQR_RCCL_LIB)
ELSEWHERE = {"stmmqr_knobs.h": None, "stmmqr_qrtest.cpp": None, "stmmqr_multi.cpp": ['getenv("STMMQR_RCCL_LIB")']}


def test_knob_table_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "knobs_selftest"
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", str(CSRC), "-o", str(exe), str(ROOT / "tests" / "knobs_selftest.cpp")]
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


def test_only_the_table_reads_the_environment():
    hits = {}
    for p in sorted(CSRC.iterdir()):
        if p.suffix not in (".cpp", ".hip", ".h") or ELSEWHERE.get(p.name, ()) is None:
            continue
        text = p.read_text()
        for allowed in ELSEWHERE.get(p.name, ()):
            text = text.replace(allowed, "")
        if 'getenv("STMMQR_' in text:
            hits[p.name] = text.count('getenv("STMMQR_')
    assert not hits, hits
