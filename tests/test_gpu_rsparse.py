"""R of the resident factors as compressed sparse columns / rows made on the device (stmmqr_plan_r_sparse; kernels:
csrc/stmmqr_rsparse.hip).

Yardstick: the host export (SparseQR.export_r / stmmqr_plan_export_r: one download, qr_rcount + qr_rconvert on one host thread) of the
same object.  Both move data and count it, no arithmetic: "equal" is equality of bits.  The compressed rows are checked against the
compressed columns of the same object re-sorted on the host; the zero test against a numpy walk of the plan's own download.

Sizes: the fixtures hold columns of fewer than 64, more than 64 and more than 256 rows (a wave's trips and its four-trip loop),
fronts of more than 64 columns (column slabs) and of more than 256 rows (row slabs: reorientation_8), dead pivot columns, m < n."""
import importlib

import numpy as np
import pytest

from pack_window_cases import front_walk
from stmmqr_testlib import Symbolic, load_golden, scalar
from test_refactor_cpu import full_matrix, new_values

pytestmark = pytest.mark.gpu
PKG = "stm-multifrontal-qr-factorization-empowered-by-gcn_amd"
ERR_INVALID = -4
I64 = np.int64
FIXTURES = ["syn_dense6x4", "syn_wide5x8", "syn_emptycol", "syn_dupcol", "syn_chain", "syn_star", "syn_rand60x40", "syn_grid2d",
            "syn_rankdef_grid", "syn_grid3d", "dwt_992", "bcsstk14", "lns_3937", "reorientation_8"]
R_ONLY = ["syn_rankdef_grid", "bcsstk14"]
FILTERED = ["syn_wide5x8", "syn_dupcol", "syn_rankdef_grid", "dwt_992", "bcsstk14"]
ZEROS = ["syn_chain", "syn_grid2d", "syn_rankdef_grid"]
LAYOUTS = [dict(STMMQR_RECYCLE="2", STMMQR_RESIDENT_CACHE="0"), dict(STMMQR_RECYCLE="2", STMMQR_RESIDENT_CACHE="1"), dict(STMMQR_RECYCLE="0")]


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module(PKG)
    assert p.device_count() >= 1
    return p


@pytest.fixture(scope="module")
def capi():
    return importlib.import_module(PKG + ".capi")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(I64)


def make(pkg, name, Ax=None, keep_h=True):
    m, n, Ap, Ai, Ax0 = full_matrix(name)
    return pkg.SparseQR(m, n, Ap, Ai, Ax0 if Ax is None else Ax, relax=pkg.relax_for_qr(n, int(Ap[-1])), keep_h=keep_h)


@pytest.fixture(scope="module")
def exports(pkg):
    """per (fixture, keep_h): the host export, both device forms and the symbolic arrays of ONE object, made once and left unchanged"""
    cache = {}

    def get(name, keep_h=True):
        if (name, keep_h) not in cache:
            Q = make(pkg, name, keep_h=keep_h)
            try:
                cache[(name, keep_h)] = {"host": Q.export_r(with_h=False), "csc": Q.r_sparse("csc"), "csr": Q.r_sparse("csr"),
                                         "sym": Q.symbolic()}
            finally:
                Q.close()
        return cache[(name, keep_h)]
    return get


def assert_csc_is_host(got, host, what):
    assert np.array_equal(got["ptr"], host["Rp"]), f"{what}: ptr differs from Rp"
    assert np.array_equal(got["idx"], host["Ri"]), f"{what}: idx differs from Ri"
    assert np.array_equal(bits(got["val"]), bits(host["Rx"])), f"{what}: val differs from Rx in its bits"
    assert got["info"][0] == host["Rp"][-1] and got["info"][3] == 0


def csr_of_csc(ptr, idx, val, m):
    """the compressed rows of a matrix given by compressed columns (rows ascending within a column): (rptr, cols, vals)"""
    ncol = ptr.size - 1
    col = np.repeat(np.arange(ncol, dtype=I64), np.diff(ptr))
    order = np.lexsort((col, idx))
    rptr = np.zeros(m + 1, I64)
    np.cumsum(np.bincount(idx, minlength=m)[:m], out=rptr[1:])
    return rptr, col[order], val[order]


def assert_csr_is(got, want, what):
    assert got["ptr"].shape == want[0].shape and np.array_equal(got["ptr"], want[0]), f"{what}: row pointers differ"
    assert np.array_equal(got["idx"], want[1]), f"{what}: column indices differ"
    assert np.array_equal(bits(got["val"]), bits(want[2])), f"{what}: values differ in their bits"


def filtered(host, ncol, econ):
    """the leading ncol columns and the rows below econ of a host export -> (ptr, idx, val)"""
    Rp, Ri, Rx = host["Rp"], host["Ri"], host["Rx"]
    col = np.repeat(np.arange(Rp.size - 1, dtype=I64), np.diff(Rp))
    keep = (col < ncol) & (Ri < econ)
    ptr = np.zeros(ncol + 1, I64)
    np.cumsum(np.bincount(col[keep], minlength=ncol)[:ncol], out=ptr[1:])
    return ptr, Ri[keep], Rx[keep]


# ---- 1: compressed columns = the host export, bit for bit ----
@pytest.mark.parametrize("name", FIXTURES)
def test_csc_equals_host_export(exports, name):
    E = exports(name)
    m, n = int(E["sym"]["m"]), int(E["sym"]["n"])
    assert E["csc"]["shape"] == (m, n) and E["csc"]["ptr"].size == n + 1
    assert_csc_is_host(E["csc"], E["host"], name)


@pytest.mark.parametrize("name", R_ONLY)
def test_csc_of_an_r_only_object(exports, name):
    E = exports(name, keep_h=False)
    assert_csc_is_host(E["csc"], E["host"], name + " (R only)")
    H = exports(name)                                                       # the R of the object with H: the same bits
    assert_csc_is_host(E["csc"], H["host"], name + " (R only against the object with H)")
    assert_csr_is(E["csr"], csr_of_csc(E["csc"]["ptr"], E["csc"]["idx"], E["csc"]["val"], int(E["sym"]["m"])), name + " (R only)")


# ---- 2: compressed rows = the compressed columns of the same object, re-sorted ----
@pytest.mark.parametrize("name", FIXTURES)
def test_csr_equals_resorted_csc(exports, name):
    E = exports(name)
    m, n = int(E["sym"]["m"]), int(E["sym"]["n"])
    csc, csr = E["csc"], E["csr"]
    assert csr["shape"] == (m, n) and csr["ptr"].size == m + 1
    assert_csr_is(csr, csr_of_csc(csc["ptr"], csc["idx"], csc["val"], m), name)
    rows = int(csr["info"][2])
    assert rows == int(csc["info"][2]) and np.all(csr["ptr"][rows:] == csr["ptr"][-1]), "rows beyond the rows of R are not empty"
    assert np.array_equal(csr["info"], csc["info"])
    # Rj ascends within a front, so a row's columns come out ascending
    for i in range(m):
        assert np.all(np.diff(csr["idx"][csr["ptr"][i]:csr["ptr"][i + 1]]) > 0)


# ---- 3: econ and ncol ----
@pytest.mark.parametrize("name", FILTERED)
def test_econ_and_ncol(pkg, exports, name):
    full = exports(name)
    m, n = int(full["sym"]["m"]), int(full["sym"]["n"])
    rows = int(full["csc"]["info"][2])
    Q = make(pkg, name)
    try:
        for econ in (0, 1, rows // 2, rows, m + 5):
            host = Q.export_r(econ=econ, with_h=False)
            for ncol in (0, 1, int(full["sym"]["Super"][1]), n - 1, n):
                what = f"{name} econ={econ} ncol={ncol}"
                want = filtered(host, ncol, m + 5)
                assert np.array_equal(want[0], host["Rp"][:ncol + 1]), "(the leading columns of a CSC are a prefix)"
                csc = Q.r_sparse("csc", ncol=ncol, econ=econ)
                assert csc["shape"] == (m, ncol)
                assert np.array_equal(csc["ptr"], want[0]) and np.array_equal(csc["idx"], want[1]), what
                assert np.array_equal(bits(csc["val"]), bits(want[2])), what
                assert csc["info"][0] == want[0][-1] and csc["info"][2] == rows
                if econ >= rows:
                    assert np.array_equal(csc["ptr"], full["host"]["Rp"][:ncol + 1]), what + ": not the prefix of the full export"
                # the filtered FULL result, as compressed rows
                fptr, fidx, fval = filtered(full["host"], ncol, econ)
                csr = Q.r_sparse("csr", ncol=ncol, econ=econ)
                assert csr["shape"] == (m, ncol)
                assert_csr_is(csr, csr_of_csc(fptr, fidx, fval, m), what)
                assert np.all(csr["ptr"][min(econ, rows):] == csr["ptr"][-1]), what + ": rows >= min(econ, rows of R) are not empty"
                assert np.array_equal(csr["info"], csc["info"]), what
    finally:
        Q.close()


# ---- 4: zero dropping, counted on the device's own download ----
def golden_plan(pkg, name, keep_h=True):
    g = load_golden(name)
    S = Symbolic(g)
    sym = {**S.sc, **{k: v for k, v in S.arr.items() if v is not None}, "keepH": 1 if keep_h else 0}
    plan = pkg.HipQR(sym)
    plan.factorize(g["in_Ax"], scalar(g, "in_tol"), int(scalar(g, "in_ntol")), g["in_Ap"], g["in_Ai"])
    return g, S, plan


def stored_and_zero(S, N):
    """the walk of walk_packed (csrc/stmmqr_export.cpp, the branch with H) over a downloaded stack: the stored entries of R and the
    exact zeros among them"""
    stored = zeros = 0
    for f in range(S.nf):
        p = int(N.Rblock_off[f])
        fp, pr = int(S.Super[f + 1] - S.Super[f]), int(S.Rp[f])
        fn, fm = int(S.Rp[f + 1]) - pr, int(N.Hm[f])
        rm_k, clen = front_walk(N.HStair[pr:pr + fn], fp, fn, fm)      # column k: clen[k] entries, the first rm_k[k] are R's
        for k in range(fn):
            rm = int(rm_k[k])
            stored += rm
            zeros += int(np.count_nonzero(N.Stack[p:p + rm] == 0.0))
            p += int(clen[k])
    return stored, zeros


def test_zero_dropping(pkg):
    dropped = 0
    for name in ZEROS:
        g, S, plan = golden_plan(pkg, name)
        try:
            stored, zeros = stored_and_zero(S, plan.download())
            for form in ("csc", "csr"):
                info = plan.r_sparse(form)["info"]
                print(f"[r_sparse zeros] {name} {form}: visited {info[1]} (walk {stored}), dropped {info[1] - info[0]} (walk {zeros})")
                assert info[1] == stored and info[1] - info[0] == zeros
            dropped += zeros
        finally:
            plan.close()
    assert dropped > 0, "no exact zero among the stored entries of the three fixtures: the zero test went unexercised"


# ---- 5: device pointers ----
def on_device(pkg, capi, plan, form, nptr, nnz):
    """the fill call into sentinel-filled device buffers from device_alloc -> (ptr, idx, val, info)"""
    ptr, idx, val, info = np.full(nptr, -7, I64), np.full(max(nnz, 1), -7, I64), np.full(max(nnz, 1), -7.0), np.zeros(4, I64)
    dp, di, dv = pkg.device_alloc(ptr.nbytes), pkg.device_alloc(idx.nbytes), pkg.device_alloc(val.nbytes)
    try:
        for d, h in ((dp, ptr), (di, idx), (dv, val)):
            pkg.device_copy(d, h.ctypes.data, h.nbytes)
        assert capi.lib.stmmqr_plan_r_sparse(plan._h, capi.R_SPARSE_FORMS[form], plan.sym["n"], plan.sym["m"], dp, di, dv, nnz,
                                             info.ctypes.data_as(capi.c_long_p), 1) == 0, capi.last_error()
        for d, h in ((dp, ptr), (di, idx), (dv, val)):
            pkg.device_copy(h.ctypes.data, d, h.nbytes)
    finally:
        pkg.device_free(dp); pkg.device_free(di); pkg.device_free(dv)
    return ptr, idx[:nnz], val[:nnz], info


@pytest.mark.parametrize("name", ["syn_rankdef_grid", "dwt_992"])
def test_device_pointers(pkg, capi, name):
    g, S, plan = golden_plan(pkg, name)
    try:
        for form in ("csc", "csr"):
            want = plan.r_sparse(form)
            nnz = int(want["info"][0])
            ptr, idx, val, info = on_device(pkg, capi, plan, form, want["ptr"].size, nnz)
            assert np.array_equal(ptr, want["ptr"]) and np.array_equal(idx, want["idx"]) and np.array_equal(bits(val), bits(want["val"]))
            assert np.array_equal(info, want["info"])
            T = plan.r_sparse(form, device=True)
            assert tuple(T.shape) == (S.m, S.n) and T.is_cuda
            comp, plain = (T.ccol_indices(), T.row_indices()) if form == "csc" else (T.crow_indices(), T.col_indices())
            assert np.array_equal(comp.cpu().numpy(), want["ptr"]) and np.array_equal(plain.cpu().numpy(), want["idx"])
            assert np.array_equal(bits(T.values().cpu().numpy()), bits(want["val"]))
        n2 = S.n // 2
        T = plan.r_sparse("csc", ncol=n2, device=True)
        assert tuple(T.shape) == (S.m, n2) and np.array_equal(T.ccol_indices().cpu().numpy(), plan.r_sparse("csc", ncol=n2)["ptr"])
    finally:
        plan.close()


# ---- 6: the two-call protocol and the refusals ----
def test_protocol_and_refusals(pkg, capi):
    lib = capi.lib
    g = load_golden("syn_grid2d")
    S = Symbolic(g)
    sym = {**S.sc, **{k: v for k, v in S.arr.items() if v is not None}}
    m, n = S.m, S.n
    plan = pkg.HipQR(sym)
    ptr, info = np.full(n + 1, -7, I64), np.full(4, -7, I64)
    ip = lambda a: a.ctypes.data_as(capi.c_long_p)

    def call(form=0, ncol=n, econ=m, p=ptr, idx=None, val=None, cap=0, inf=info, h=None):
        return lib.stmmqr_plan_r_sparse(plan._h if h is None else h, form, ncol, econ, None if p is None else p.ctypes.data,
                                        None if idx is None else idx.ctypes.data, None if val is None else val.ctypes.data, cap,
                                        None if inf is None else ip(inf), 0)
    try:
        assert call() == ERR_INVALID and "no factorization" in capi.last_error()
        with pytest.raises(pkg.StmmqrError, match="no factorization") as e:
            plan.r_sparse()
        assert e.value.code == ERR_INVALID
        plan.factorize(g["in_Ax"], scalar(g, "in_tol"), int(scalar(g, "in_ntol")), g["in_Ap"], g["in_Ai"])
        x0 = plan.solve(np.ones(m))
        one = np.zeros(1, I64)
        for kw, word in ((dict(form=2), "form"), (dict(form=-1), "form"), (dict(ncol=-1), "ncol"), (dict(ncol=n + 1), "ncol"),
                         (dict(econ=-1), "econ"), (dict(cap=-1), "cap"), (dict(p=None), "ptr"), (dict(inf=None), "info"),
                         (dict(idx=one), "idx and val"), (dict(val=np.zeros(1)), "idx and val")):
            assert call(**kw) == ERR_INVALID and word in capi.last_error(), f"{kw}: {capi.last_error()}"
        assert lib.stmmqr_plan_r_sparse(None, 0, n, m, ptr.ctypes.data, None, None, 0, ip(info), 0) == ERR_INVALID
        assert np.all(ptr == -7) and np.all(info == -7)                      # no refusal wrote anything
        # the count call, a capacity one short, the full call
        assert call() == 0
        nnz = int(info[0])
        assert nnz > 1 and ptr[0] == 0 and ptr[-1] == nnz
        ptr0 = ptr.copy()
        ptr[:] = -7
        idx, val = np.full(nnz, -7, I64), np.full(nnz, -7.0)
        assert call(idx=idx, val=val, cap=nnz - 1) == ERR_INVALID
        assert str(nnz) in capi.last_error() and str(nnz - 1) in capi.last_error() and "cap" in capi.last_error()
        assert np.all(idx == -7) and np.all(val == -7.0) and np.array_equal(ptr, ptr0) and info[0] == nnz
        assert call(idx=idx, val=val, cap=nnz) == 0
        want = plan.r_sparse()
        assert np.array_equal(ptr, want["ptr"]) and np.array_equal(idx, want["idx"]) and np.array_equal(bits(val), bits(want["val"]))
        assert np.array_equal(plan.solve(np.ones(m)), x0)                    # the plan stays usable
    finally:
        plan.close()
    # groups set: not a whole-tree plan (the construction of tests/test_gpu_condest.py)
    parent = np.full(S.nf, -1)
    for f in range(S.nf):
        for q in range(int(S.Childp[f]), int(S.Childp[f + 1])):
            parent[int(S.Child[q])] = f
    group = np.zeros(S.nf, np.int32)
    f = int(parent[0])
    while f >= 0:
        group[f] = 1
        f = int(parent[f])
    assert group.any() and not group.all()
    plan = pkg.HipQR(sym)
    try:
        plan.set_groups(group)
        plan.factorize(g["in_Ax"], scalar(g, "in_tol"), int(scalar(g, "in_ntol")), g["in_Ap"], g["in_Ai"])
        with pytest.raises(pkg.StmmqrError, match="whole tree") as e:
            plan.r_sparse()
        assert e.value.code == ERR_INVALID
        assert plan.result_sizes()[1] == S.n                                 # the plan stays usable
    finally:
        plan.close()


# ---- 7: the scratch layouts, and a second factorization ----
@pytest.mark.parametrize("name", ["dwt_992", "bcsstk14"])
def test_scratch_layouts(pkg, exports, monkeypatch, name):
    want = exports(name)
    for layout in LAYOUTS:
        for k in ("STMMQR_RECYCLE", "STMMQR_RESIDENT_CACHE"):
            monkeypatch.delenv(k, raising=False)
        for k, v in layout.items():
            monkeypatch.setenv(k, v)
        Q = make(pkg, name)
        try:
            for form in ("csc", "csr"):
                got = Q.r_sparse(form)
                for k in ("ptr", "idx", "info"):
                    assert np.array_equal(got[k], want[form][k]), f"{name} {layout} {form}: {k} differs"
                assert np.array_equal(bits(got["val"]), bits(want[form]["val"])), f"{name} {layout} {form}: val differs"
        finally:
            Q.close()


@pytest.mark.parametrize("name", ["dwt_992", "bcsstk14"])
def test_after_refactorize(pkg, name):
    Ax2 = new_values(full_matrix(name)[4])
    Q, F = make(pkg, name), make(pkg, name, Ax2)
    try:
        first = Q.r_sparse("csc")
        Q.refactorize(Ax2)
        for form in ("csc", "csr"):
            got, want = Q.r_sparse(form), F.r_sparse(form)
            for k in ("ptr", "idx", "info"):
                assert np.array_equal(got[k], want[k]), f"{name} {form}: {k} differs from a new object's"
            assert np.array_equal(bits(got["val"]), bits(want["val"]))
        assert_csc_is_host(Q.r_sparse("csc"), Q.export_r(with_h=False), name + " after refactorize")
        assert first["val"].size and not np.array_equal(first["val"], Q.r_sparse("csc")["val"]), "the new values changed nothing"
    finally:
        Q.close(); F.close()
