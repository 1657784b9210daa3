"""stmmqr_plan_r_sparse, the part that needs no GPU: the symbol is declared and exported, an object that holds the host half only
refuses with the library's message, and the fixtures have the property the compressed-row form's column order rests on.  (The
feature adds no function to the pure csrc/stmmqr_restables.{h,cpp} -- the counts, offsets and positions are computed by the kernels
--, so there is no stand-alone sanitizer program for it.)"""
import importlib
import re
from pathlib import Path

import numpy as np
import pytest

from stmmqr_testlib import Symbolic, load_golden
from test_refactor_cpu import full_matrix

ROOT = Path(__file__).resolve().parent.parent
PKG = "stm-multifrontal-qr-factorization-empowered-by-gcn_amd"
FIXTURES = ["syn_dense6x4", "syn_wide5x8", "syn_emptycol", "syn_dupcol", "syn_chain", "syn_star", "syn_rand60x40", "syn_grid2d",
            "syn_rankdef_grid", "syn_grid3d", "dwt_992", "bcsstk14", "lns_3937", "reorientation_8"]


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module(PKG)


def test_declared_and_exported(pkg):
    header = (ROOT / "include" / "stmmqr_hip.h").read_text()
    assert re.search(r"\bint stmmqr_plan_r_sparse\(stmmqr_plan \*plan, int form, stm_long ncol, stm_long econ,", header)
    assert re.search(r"#define STMMQR_RSPARSE_CSC 0\b", header) and re.search(r"#define STMMQR_RSPARSE_CSR 1\b", header)
    lib = pkg.capi.lib
    assert hasattr(lib, "stmmqr_plan_r_sparse") and hasattr(lib, "stmmqr_plan_device_index")
    assert pkg.capi.R_SPARSE_FORMS == {"csc": 0, "csr": 1}
    assert lib.stmmqr_plan_device_index(None) == -1


def test_host_only_object_refuses(pkg):
    m, n, Ap, Ai, Ax = full_matrix("syn_star")
    Q = pkg.SparseQR.lq(m, n, Ap, Ai, Ax, device=-2)
    try:
        for form in ("csc", "csr"):
            with pytest.raises(pkg.StmmqrError, match="no factorization held by the plan") as e:
                Q.r_sparse(form)
            assert e.value.code == -4
        with pytest.raises(pkg.StmmqrError, match="neither 'csc' nor 'csr'"):
            Q.r_sparse("coo")
    finally:
        Q.close()
    Q = pkg.SparseQR(m, n, Ap, Ai, Ax, symbolic_only=True)
    try:
        with pytest.raises(pkg.StmmqrError, match="no factorization held by the plan"):
            Q.r_sparse(device=True)                                          # (refused before torch is looked for)
    finally:
        Q.close()


@pytest.mark.parametrize("name", FIXTURES)
def test_rj_ascends_within_a_front(name):
    """a row of R lists its front's columns in front order; they ascend because Rj does: pivotal columns Super[f] .. first, then
    the non-pivotal ones, all larger and increasing"""
    S = Symbolic(load_golden(name))
    for f in range(S.nf):
        rj = np.asarray(S.Rj[int(S.Rp[f]):int(S.Rp[f + 1])])
        fp = int(S.Super[f + 1] - S.Super[f])
        assert np.array_equal(rj[:fp], np.arange(int(S.Super[f]), int(S.Super[f + 1])))
        assert np.all(np.diff(rj) > 0)
