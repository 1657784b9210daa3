"""Host-side pieces of bench.py that need no GPU: the --matrix workload builder (reader + own symbolic phase -> the same
qr_symbolic and the same matrix at the seam as the compiled reference recorded in the fixture) and the CPU-baseline legs."""
import importlib
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
PKG = "stm-multifrontal-qr-factorization-empowered-by-gcn_amd"


@pytest.mark.parametrize("name", ["epb1", "bcsstk14", "dwt_992", "cvxqp3"])
def test_matrix_workload_equals_the_fixture(tmp_path, name):
    """bench.py --matrix F.mtx: what it hands to the timed numeric factorization is what the reference's driver handed to
    qr_factorize on the same file (fixture = refdump's record): the matrix after singleton removal, ntol, the whole qr_symbolic;
    tol to the last bits of a 2-norm"""
    import bench
    from stmmqr_testlib import Symbolic, load_golden, scalar
    pkg = importlib.import_module(PKG)
    g0 = load_golden(name)
    p = tmp_path / f"{name}.mtx"
    bench._write_mtx(p, int(g0["A_m"][0]), int(g0["A_n"][0]), g0["A_p"], g0["A_i"], g0["A_x"])
    g, meta = bench.matrix_workload(pkg, p, "default")
    S, S0 = Symbolic(g), Symbolic(g0)
    assert S.sc == S0.sc
    for k, a in S0.arr.items():
        if a is None or k in ("Fm", "Cm"):
            continue
        np.testing.assert_array_equal(S.arr[k], a, err_msg=k)
    for k in ("Fm", "Cm"):
        np.testing.assert_array_equal(S.arr[k][:S.nf], S0.arr[k][:S.nf])
    for k in ("in_Ap", "in_Ai", "in_Ax"):
        np.testing.assert_array_equal(g[k], g0[k])
    assert scalar(g, "in_ntol") == scalar(g0, "in_ntol")
    assert abs(scalar(g, "in_tol") - scalar(g0, "in_tol")) <= 4e-16 * scalar(g0, "in_tol")
    assert meta["n1cols"] == scalar(g0, "n1cols")


def test_other_orderings_are_refused():
    import bench
    pkg = importlib.import_module(PKG)
    with pytest.raises(SystemExit, match="third-party"):
        bench.matrix_workload(pkg, "nowhere.mtx", "metis")


@pytest.mark.skipif(not (ROOT / "oracle" / "_ref" / "refdump").exists(), reason="oracle/_ref not built")
def test_cpu_baseline_legs():
    """every leg is either measured on THIS host (best of 3 below 20 s, sized from the host's own first run) or reported with the
    reason it failed -- the TPSM leg of the reference as compiled in place dies in TPSM_Numa_SearchNodeSequence on a host without
    the 4 NUMA nodes of its checked-in Numainfo.h and must say so rather than vanish"""
    import bench
    from stmmqr_testlib import load_golden
    g = load_golden("syn_grid3d")
    cb = bench.cpu_baseline("syn_grid3d", g)
    assert cb["kind"] == "reference" and cb["value"] > 0
    legs = cb["legs"]
    assert legs[0]["cores"] == 1 and legs[0]["best_of"] == 3 and legs[0]["seconds"] > 0
    if bench.host_cores() > 1:
        assert len(legs) == 3 and "TPSM" in legs[2]["mode"]
        assert ("value" in legs[2]) != ("error" in legs[2])
        for l in legs:
            assert ("FAILED" in cb["sample"]) == any("error" in x for x in legs)


def test_dump_outputs_is_the_download_within_64_mb(tmp_path, oracle):
    """--dump-outputs writes what plan.download() returns: float64 arrays that hold the integer arrays exactly, the whole packed
    R+H of a small factorization, the sum of squares of every front's block; an R+H longer than the sample is cut to a fixed sample,
    all files together stay within 64 MB, and the sample is the same in two runs."""
    import types
    import bench
    from stmmqr_testlib import Symbolic, load_golden, scalar
    g = load_golden("syn_grid3d")
    S = Symbolic(g)
    No = oracle.factorize(S, g["in_Ap"], g["in_Ai"], g["in_Ax"], scalar(g, "in_tol"), int(scalar(g, "in_ntol")))

    class Plan:
        def __init__(self, stack):
            self.stack = stack

        def download(self):
            return types.SimpleNamespace(Stack=self.stack, Rblock_off=No.Rblock_off, Rdead=No.Rdead, HStair=No.HStair, HTau=No.HTau,
                                         Hii=No.Hii, HPinv=No.HPinv, Hm=No.Hm, Hr=No.Hr, rank=No.c.rank, rank1=No.c.rank1,
                                         maxfrank=No.c.maxfrank, maxfm=No.c.maxfm, rh_total=self.stack.size)

    rh = No.c.rh_total
    bench.dump_outputs(tmp_path / "a", Plan(No.Stack[:rh]), S)
    out = {f.stem: np.load(f) for f in (tmp_path / "a").glob("*.npy")}
    assert all(a.dtype == np.float64 for a in out.values())
    np.testing.assert_array_equal(out["R_H_stack_sample"], No.Stack[:rh])
    np.testing.assert_array_equal(out["HStair"], No.HStair[:S.rjsize])
    np.testing.assert_array_equal(out["Rdead"], No.Rdead[:S.n])
    np.testing.assert_array_equal(out["info"], [No.c.rank, No.c.rank1, No.c.maxfrank, No.c.maxfm, rh])
    blocks = No.rh_blocks(S)
    np.testing.assert_allclose(out["R_H_front_sumsq"], [np.dot(blocks[f], blocks[f]) for f in range(S.nf)], rtol=1e-14)

    big = np.random.default_rng(0).standard_normal(3 * bench.DUMP_STACK_CAP)
    for d in ("b", "c"):
        bench.dump_outputs(tmp_path / d, Plan(big), S)
        assert sum(f.stat().st_size for f in (tmp_path / d).glob("*.npy")) <= 64 << 20
    b, c = np.load(tmp_path / "b" / "R_H_stack_sample.npy"), np.load(tmp_path / "c" / "R_H_stack_sample.npy")
    assert b.size == bench.DUMP_STACK_CAP and np.array_equal(b, c) and np.all(np.isin(b[:100], big))
