"""The yardstick of tests/test_gpu_nullspace.py, checked without a GPU: tests/nullspace_reference.py on factors the CPU oracle made.
Asserted, because it can be derived: the basic solution through the factors, projected by the yardstick, is the minimum-norm
least-squares solution, so it equals numpy.linalg.lstsq(A_in, b, rcond=1e-10) -- A_in the matrix actually factorized -- within
solve_tol(cond), cond = the ratio of the largest singular value of A_in to the smallest one above the gap; N_ref has the identity on
the dead columns and R N_ref = 0 to rounding.  Printed, not asserted: |W|_2, cond(R11) and what one and two passes of the float64
emulation of the device's projector (Gram matrix, Cholesky factor) leave of N'x, so the GPU test's expectations are on record."""
import numpy as np
import pytest
import scipy.linalg as sla

import nullspace_reference as nr
from minnorm_reference import dense_of, qfill_of
from resident_reference import LD, Factors
from stmmqr_testlib import EPS, Symbolic, load_golden, scalar, solve_tol

NAMES = ["syn_dupcol", "syn_rankdef_grid", "syn_wide5x8", "dwt_992"]


def gap_cond(A):
    """(cond, rank): largest singular value over the smallest one above the gap rcond = 1e-10"""
    s = np.linalg.svd(A, compute_uv=False)
    keep = s > 1e-10 * s[0]
    return float(s[0] / s[keep][-1]), int(keep.sum())


def emulated_passes(N, x):
    """|N'x| / (|N|_F |x|) after one and after two passes of x -= N (L L')^-1 N'x in float64"""
    N, x = np.asarray(N, float), np.array(x, float)
    c = sla.cho_factor(N.T @ N, lower=True)
    scale = np.linalg.norm(N) * np.linalg.norm(x)
    out = []
    for _ in range(2):
        x = x - N @ sla.cho_solve(c, N.T @ x)
        out.append(float(np.linalg.norm(N.T @ x) / scale))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_projected_basic_solution_is_the_minimum_norm_one(oracle, name):
    g = load_golden(name)
    S = Symbolic(g)
    N0 = oracle.factorize(S, g["in_Ap"], g["in_Ai"], g["in_Ax"], scalar(g, "in_tol"), int(scalar(g, "in_ntol")))
    Fa = Factors(S, N0)
    m, n = S.m, S.n
    A = dense_of(m, n, g["in_Ap"], g["in_Ai"], g["in_Ax"])
    q = qfill_of(S)
    R11, R12, pc, jd = nr.blocks(Fa)
    d = jd.size
    assert d == n - Fa.rank and d > 0
    Nref = nr.nullspace_ref(Fa)
    # the identity on the dead columns, R N = 0 to rounding
    assert np.array_equal(np.asarray(Nref[jd], float), np.eye(d))
    res = nr.rn_residual(R11, R12, Nref[pc])
    fro = float(np.sqrt((np.asarray(R11, float) ** 2).sum()))
    assert np.all(np.asarray(res, float) <= (Fa.rank + 2) * EPS * fro * np.asarray(nr.colnorm(Nref), float))
    # basic solution through the factors, projected, against lstsq on A itself
    B = np.random.default_rng(11).standard_normal((m, 3))
    xb = Fa.rsolve(Fa.qtx(B))                                # R's column order, zero on dead columns
    assert not np.any(np.asarray(xb[jd], float))
    xm = nr.project_ref(Nref, xb)
    X = np.zeros((n, 3), LD)
    X[q] = xm                                                # X[Qfill[k]] = x[k]
    want = np.linalg.lstsq(A, B, rcond=1e-10)[0]
    cond, rank = gap_cond(A)
    assert rank == Fa.rank
    err = float(np.max(np.linalg.norm(np.asarray(X, float) - want, axis=0) / np.linalg.norm(want, axis=0)))
    shrink = float(np.max(np.asarray(nr.colnorm(xm), float) / np.asarray(nr.colnorm(xb), float)))
    one, two = emulated_passes(Nref, np.asarray(xb[:, 0], float))
    print(f"\n[nullspace cpu] {name}: n {n}, d {d}, |W|_2 {nr.norm2(Nref[pc]):.2e}, cond(R11) {nr.cond2(R11):.2e}, cond(A_in) above the gap {cond:.2e}; "
          f"|x_min - lstsq| / |lstsq| {err:.1e} (allowed {solve_tol(cond):.1e}), |x_min| / |x_basic| {shrink:.3f}; "
          f"float64 projector |N'x| / (|N| |x|): one pass {one:.1e}, two passes {two:.1e}")
    assert err <= solve_tol(cond)
    # a projection: idempotent, orthogonal to N, never longer than its input
    assert np.all(np.asarray(nr.colnorm(xm), float) <= np.asarray(nr.colnorm(xb), float) * (1 + 8 * (d + 2) * EPS))
    assert float(np.max(np.asarray(nr.colnorm(Nref.T @ xm), float))) <= 8 * (d + 2) * EPS * float(np.sqrt((np.asarray(Nref, float) ** 2).sum())) * float(
        np.max(np.asarray(nr.colnorm(xb), float)))


def test_index_helpers():
    class Fake:
        n, rank = 7, 4
        pivot_col = np.array([0, 2, 3, 6])
    pc, jd = nr.split(Fake)
    assert pc.tolist() == [0, 2, 3, 6] and jd.tolist() == [1, 4, 5]
    pc, jd = nr.split(Fake, 5)                               # a view that ends at column 5
    assert pc.tolist() == [0, 2, 3] and jd.tolist() == [1, 4]
    T = np.triu(np.arange(1.0, 10.0).reshape(3, 3)) + 3 * np.eye(3)
    B = np.arange(6.0).reshape(3, 2)
    assert np.allclose(nr.back_substitute(T, B), np.linalg.solve(T, B), rtol=1e-14)
    assert nr.project_ref(np.zeros((3, 0), LD), np.ones(3)).shape == (3, 1)


def test_transposed_reference_basis_without_the_basis(oracle):
    """nref_t_apply: N_ref' X by one forward substitution equals N_ref' X with N_ref formed"""
    g = load_golden("dwt_992")
    S = Symbolic(g)
    Fa = Factors(S, oracle.factorize(S, g["in_Ap"], g["in_Ai"], g["in_Ax"], scalar(g, "in_tol"), int(scalar(g, "in_ntol"))))
    R11, R12, pc, jd = nr.blocks(Fa)
    Nref = nr.nullspace_ref(Fa)
    X = np.random.default_rng(4).standard_normal((S.n, 2))
    a, b = nr.nref_t_apply(R11, R12, pc, jd, X), Nref.T @ np.asarray(X, LD)
    scale = float(np.sqrt((np.asarray(Nref, float) ** 2).sum())) * np.linalg.norm(X, axis=0)
    assert np.all(np.asarray(nr.colnorm(a - b), float) <= 1e-3 * EPS * nr.cond2(R11) * scale)      # long double: 2^-11 of float64's eps cond


def test_index_work_under_asan_ubsan(tmp_path):
    """restab::null_* of csrc/stmmqr_restables.cpp as a stand-alone program (tests/nullspace_selftest.cpp), the recipe of
    tests/test_restables_cpu.py"""
    import os
    import shutil
    import subprocess
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    csrc = root / "stm-multifrontal-qr-factorization-empowered-by-gcn_amd" / "csrc"
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    rocm = Path(os.environ.get("ROCM_PATH", "/opt/rocm"))
    if not (rocm / "include" / "hip" / "hip_runtime.h").exists():
        pytest.skip("no hip/hip_runtime.h")
    exe = tmp_path / "nullspace_selftest"
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-isystem", str(rocm / "include"), "-I", str(csrc), "-o", str(exe),
           str(root / "tests" / "nullspace_selftest.cpp"), str(csrc / "stmmqr_restables.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and "asan" in b.stderr.lower() and "cannot find" in b.stderr.lower():
        pytest.skip("the sanitizer runtimes are not installed")
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60,
                       env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1", "PATH": "/usr/bin:/bin"})
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.strip().splitlines()[-1] == "ok (0 failures)"
