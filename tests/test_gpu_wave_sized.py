"""The sized eight-sum butterfly of the panel kernels (csrc/stmmqr_wave.h, wave_reduce8<NV>), compiled as a stand-alone HIP
program on the GPU box: for NV = 1 .. 8 the lanes and broadcasts a caller may read hold the bytes of the unsized form, on
non-integer data whose sums round differently in another order (tests/wave_sized_selftest.hip)."""
import pathlib
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
PKG = ROOT / "stm-multifrontal-qr-factorization-empowered-by-gcn_amd"


def test_sized_butterfly_same_bits(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "wave_sized_selftest"
    subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-I", str(PKG / "csrc"), str(ROOT / "tests" / "wave_sized_selftest.hip"),
                    "-o", str(exe)], check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bad=0" in r.stdout
