"""H, HTau and HPinv of the resident factors made on the device (stmmqr_plan_h_sparse; kernels: csrc/stmmqr_hsparse.hip).

Yardstick: the host export (SparseQR.export_r(with_h=True) / stmmqr_plan_export_r: one download, qr_rcount + qr_rconvert on one host
thread) of the same object, and the numpy walker of tests/hsparse_reference.py on the plan's own download (tests/test_hsparse_cpu.py
holds that walker against qr_rcount / qr_rconvert on the reference's factorization).  Both move data and count it, no arithmetic:
"equal" is equality of bits.  That the arrays are a usable Q is checked against qmult(0, .) of the same plan at the project's parity
bar, 1e-13 (README).

Sizes: the fixtures hold columns of H shorter than 64 rows, longer than 64 and longer than 256 (a wave's trips and its four-trip
loop: lns_3937, reorientation_8), fronts of more than 64 columns (column slabs), dead pivot columns, slots with t >= h and Tau == 0,
h capped at fm, m < n."""
import importlib

import numpy as np
import pytest

from hsparse_reference import apply_reflectors, walk_h_of_download
from stmmqr_testlib import Symbolic, load_golden, scalar
from test_refactor_cpu import full_matrix, new_values

pytestmark = pytest.mark.gpu
PKG = "stm-multifrontal-qr-factorization-empowered-by-gcn_amd"
ERR_INVALID = -4
I64 = np.int64
FIXTURES = ["syn_dense6x4", "syn_wide5x8", "syn_emptycol", "syn_dupcol", "syn_chain", "syn_star", "syn_rand60x40", "syn_grid2d",
            "syn_rankdef_grid", "syn_grid3d", "dwt_992", "bcsstk14", "lns_3937", "reorientation_8"]
IS_A_Q = ["syn_wide5x8", "syn_dupcol", "syn_rankdef_grid", "dwt_992", "bcsstk14", "lns_3937"]
LAYOUTS = [dict(STMMQR_RECYCLE="2", STMMQR_RESIDENT_CACHE="0"), dict(STMMQR_RECYCLE="2", STMMQR_RESIDENT_CACHE="1"), dict(STMMQR_RECYCLE="0")]
ARRAYS = ("Hp", "Hi", "Hx", "HTau", "HPinv")


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


def plan_of(capi, Q):
    """the device plan of a SparseQR object as a HipQR (borrowed: valid until Q.close())"""
    sym = Q.symbolic()
    p = capi.HipQR.__new__(capi.HipQR)
    p._keep, p._borrowed, p._h = {}, True, capi.lib.stmmqr_sparseqr_plan(Q._h)
    p.sym = {k: int(sym[k]) for k in ["m", "n", "anz", "nf", "maxfn", "rjsize", "hisize"]}
    return p


def assert_same_arrays(got, want, what, keys=ARRAYS):
    for k in keys:
        assert got[k].shape == want[k].shape, f"{what}: {k} has {got[k].shape}, not {want[k].shape}"
        same = np.array_equal(bits(got[k]), bits(want[k])) if got[k].dtype == np.float64 else np.array_equal(got[k], want[k])
        assert same, f"{what}: {k} differs"


def assert_is_host(got, host, what):
    nh = host["Hp"].size - 1
    assert got["shape"][1] == nh and got["info"][0] == nh and got["info"][1] == host["Hp"][-1], f"{what}: nh / hnz differ"
    assert_same_arrays(got, host, what, ("Hp", "Hi", "Hx", "HTau"))


@pytest.fixture(scope="module")
def exports(pkg, capi):
    """per fixture: the host export, the device export and the HPinv of the download of ONE object, made once and left unchanged"""
    cache = {}

    def get(name):
        if name not in cache:
            Q = make(pkg, name)
            try:
                cache[name] = {"host": Q.export_r(with_h=True), "dev": Q.h_sparse(), "HPinv": plan_of(capi, Q).download().HPinv,
                               "sym": Q.symbolic()}
            finally:
                Q.close()
        return cache[name]
    return get


# ---- 1: equals the host export, bit for bit ----
@pytest.mark.parametrize("name", FIXTURES)
def test_equals_host_export(exports, name):
    E = exports(name)
    m = int(E["sym"]["m"])
    got = E["dev"]
    assert got["shape"][0] == m and got["info"][3] == m and got["HPinv"].size == m
    assert_is_host(got, E["host"], name)
    assert np.array_equal(got["HPinv"], E["HPinv"][:m]), f"{name}: HPinv differs from the download's"
    assert np.array_equal(np.sort(got["HPinv"]), np.arange(m)), f"{name}: HPinv is no permutation"
    assert got["info"][2] >= got["info"][1]


@pytest.mark.parametrize("name,rows", [("syn_grid3d", 64), ("bcsstk14", 64), ("lns_3937", 256), ("reorientation_8", 256)])
def test_fixtures_reach_every_trip_count(exports, name, rows):
    """the sizes the module docstring counts on, read from the host export: a column of H that keeps more than `rows` entries below
    its diagonal (more than one trip of 64 rows; more than 256: the four-trip loop), and columns shorter than one trip"""
    kept = np.diff(exports(name)["host"]["Hp"]) - 1
    assert kept.max() > rows, f"{name}: the longest column of H keeps {kept.max()} entries below its diagonal"
    assert kept.min() < 64


def golden_plan(pkg, name, Ax=None, keep_h=True):
    g = load_golden(name)
    S = Symbolic(g)
    sym = {**S.sc, **{k: v for k, v in S.arr.items() if v is not None}, "keepH": 1 if keep_h else 0}
    plan = pkg.HipQR(sym)
    plan.factorize(g["in_Ax"] if Ax is None else Ax, scalar(g, "in_tol"), int(scalar(g, "in_ntol")), g["in_Ap"], g["in_Ai"])
    return g, S, plan


# ---- 2: the arrays are a Q ----
@pytest.mark.parametrize("name", IS_A_Q)
def test_arrays_are_a_q(pkg, name):
    g, S, plan = golden_plan(pkg, name)
    try:
        H = plan.h_sparse()
        rng = np.random.default_rng(20240611)
        for trial in range(3):
            x = rng.standard_normal(S.m)
            want = plan.qmult(0, x)
            got = apply_reflectors(H, x)
            rel = np.linalg.norm(got - want) / np.linalg.norm(want)
            print(f"[h_sparse is a Q] {name} vector {trial}: nh {H['shape'][1]}, relative difference {rel:.3e}")
            assert rel <= 1e-13, f"{name} vector {trial}: relative difference {rel:.3e} to qmult(0, x)"
    finally:
        plan.close()


# ---- 3: zero dropping, with a zero that is certain to be there ----
def test_zero_dropping(pkg):
    g = load_golden("dwt_992")
    S = Symbolic(g)
    q0 = int(S.Qfill[0]) if S.Qfill is not None else 0
    Ap, Ax = g["in_Ap"], np.array(g["in_Ax"], np.float64, copy=True)
    p0, p1 = int(Ap[q0]), int(Ap[q0 + 1])
    assert p1 - p0 == 8 and np.all(Ax[p0:p1] == 1.0), "the first column of the factorized matrix is not the eight ones the test counts on"
    assert int(S.Super[1]) - int(S.Super[0]) >= 1
    Ax[p0 + 2] = 0.0
    Ax[p0 + 5] = 0.0
    _, _, plan = golden_plan(pkg, "dwt_992", Ax=Ax)
    try:
        N = plan.download()
        assert int(N.HStair[int(S.Rp[0])]) == 8, "front 0 does not start with the column of eight rows"
        W = walk_h_of_download(S, N)
        assert W["zeros"] >= 1, "no exact zero in an H part of the plan's own download: the zero test went unexercised"
        H = plan.h_sparse()
        print(f"[h_sparse zeros] visited {H['info'][2]} (walk {W['visited']}), dropped {H['info'][2] - H['info'][1]} (walk {W['zeros']})")
        assert H["info"][2] - H["info"][1] == W["zeros"]
        assert H["info"][2] == W["visited"]
        assert H["info"][0] == W["nh"]
        assert_same_arrays(H, W, "dwt_992 with two zeroed values", ("Hp", "Hi", "Hx", "HTau"))
        assert not np.any(H["Hx"] == 0.0)
    finally:
        plan.close()


# ---- 4: device pointers ----
def on_device(pkg, capi, plan, nh, hnz, m):
    """the fill call into sentinel-filled device buffers from device_alloc, each with one spare element -> the five host copies, info"""
    host = [np.full(nh + 2, -7, I64), np.full(hnz + 1, -7, I64), np.full(hnz + 1, -7.0), np.full(nh + 1, -7.0), np.full(m + 1, -7, I64)]
    info = np.zeros(4, I64)
    dev = [pkg.device_alloc(h.nbytes) for h in host]
    try:
        for d, h in zip(dev, host):
            pkg.device_copy(d, h.ctypes.data, h.nbytes)
        assert capi.lib.stmmqr_plan_h_sparse(plan._h, dev[0], dev[1], dev[2], dev[3], dev[4], nh, hnz, info.ctypes.data_as(capi.c_long_p),
                                             1) == 0, capi.last_error()
        for d, h in zip(dev, host):
            pkg.device_copy(h.ctypes.data, d, h.nbytes)
    finally:
        for d in dev:
            pkg.device_free(d)
    return host, info


@pytest.mark.parametrize("name", ["syn_rankdef_grid", "dwt_992"])
def test_device_pointers(pkg, capi, name):
    g, S, plan = golden_plan(pkg, name)
    try:
        want = plan.h_sparse()
        nh, hnz, m = int(want["info"][0]), int(want["info"][1]), S.m
        (Hp, Hi, Hx, HTau, HPinv), info = on_device(pkg, capi, plan, nh, hnz, m)
        assert Hp[-1] == -7 and Hi[-1] == -7 and Hx[-1] == -7.0 and HTau[-1] == -7.0 and HPinv[-1] == -7, "a spare element was written"
        got = {"Hp": Hp[:-1], "Hi": Hi[:-1], "Hx": Hx[:-1], "HTau": HTau[:-1], "HPinv": HPinv[:-1]}
        assert_same_arrays(got, want, name + " (device pointers)")
        assert np.array_equal(info, want["info"])
        T = plan.h_sparse(device=True)
        assert T["shape"] == (m, nh) and np.array_equal(T["info"], want["info"]) and isinstance(T["info"], np.ndarray)
        for k in ARRAYS:
            assert T[k].is_cuda, f"{k} is not on the device"
        assert_same_arrays({k: T[k].cpu().numpy() for k in ARRAYS}, want, name + " (device=True)")
    finally:
        plan.close()


# ---- 5: the two-call protocol and the refusals ----
def test_protocol_and_refusals(pkg, capi):
    lib = capi.lib
    g = load_golden("syn_grid2d")
    S = Symbolic(g)
    sym = {**S.sc, **{k: v for k, v in S.arr.items() if v is not None}}
    m = S.m
    plan = pkg.HipQR(sym)
    info = np.full(4, -7, I64)
    big = max(S.rjsize, m) + 1
    A = {"Hp": np.full(big + 1, -7, I64), "Hi": np.full(1, -7, I64), "Hx": np.full(1, -7.0), "HTau": np.full(big, -7.0),
         "HPinv": np.full(m, -7, I64)}
    ip = lambda a: a.ctypes.data_as(capi.c_long_p)

    def call(Hp=None, Hi=None, Hx=None, HTau=None, HPinv=None, colcap=0, cap=0, inf=info):
        ptr = lambda a: None if a is None else a.ctypes.data
        return lib.stmmqr_plan_h_sparse(plan._h, ptr(Hp), ptr(Hi), ptr(Hx), ptr(HTau), ptr(HPinv), colcap, cap,
                                        None if inf is None else ip(inf), 0)

    def untouched():
        return all(np.all(A[k] == -7) for k in A)
    try:
        assert call(HPinv=A["HPinv"]) == ERR_INVALID and "no factorization" in capi.last_error()
        with pytest.raises(pkg.StmmqrError, match="no factorization") as e:
            plan.h_sparse()
        assert e.value.code == ERR_INVALID
        plan.factorize(g["in_Ax"], scalar(g, "in_tol"), int(scalar(g, "in_ntol")), g["in_Ap"], g["in_Ai"])
        x0 = plan.solve(np.ones(m))
        four = dict(Hp=A["Hp"], Hi=A["Hi"], Hx=A["Hx"], HTau=A["HTau"])
        partial = [{k: v for k, v in four.items() if k != drop} for drop in four] + [dict(Hp=A["Hp"]), dict(Hi=A["Hi"], Hx=A["Hx"])]
        for kw, word in [(dict(colcap=-1), "colcap"), (dict(cap=-1), "cap"), (dict(inf=None), "info")] + [(kw, "all") for kw in partial]:
            assert call(HPinv=A["HPinv"], **kw) == ERR_INVALID and word in capi.last_error(), f"{list(kw)}: {capi.last_error()}"
        assert lib.stmmqr_plan_h_sparse(None, None, None, None, None, ip(A["HPinv"]), 0, 0, ip(info), 0) == ERR_INVALID
        assert untouched() and np.all(info == -7)                           # no refusal wrote anything
        # the count call: info alone, and HPinv where it is given
        assert call() == 0
        nh, hnz = int(info[0]), int(info[1])
        assert nh > 1 and hnz > nh and info[2] >= hnz and info[3] == m and untouched()
        assert call(HPinv=A["HPinv"]) == 0
        hpinv = plan.download().HPinv[:m]
        assert np.array_equal(A["HPinv"], hpinv)
        A["HPinv"][:] = -7
        # a capacity one short, either of the two: both numbers named, info written, nothing else
        A["Hi"], A["Hx"] = np.full(hnz, -7, I64), np.full(hnz, -7.0)
        four = dict(Hp=A["Hp"], Hi=A["Hi"], Hx=A["Hx"], HTau=A["HTau"], HPinv=A["HPinv"])
        for colcap, cap in ((nh - 1, hnz), (nh, hnz - 1)):
            info[:] = -7
            assert call(colcap=colcap, cap=cap, **four) == ERR_INVALID
            msg = capi.last_error()
            assert str(nh) in msg and str(hnz) in msg and str(colcap) in msg and str(cap) in msg and "colcap" in msg and "cap = " in msg
            assert untouched() and info[0] == nh and info[1] == hnz
        assert call(colcap=nh, cap=hnz, **four) == 0
        want = plan.h_sparse()
        got = {"Hp": A["Hp"][:nh + 1], "Hi": A["Hi"], "Hx": A["Hx"], "HTau": A["HTau"][:nh], "HPinv": A["HPinv"]}
        assert_same_arrays(got, want, "the full call")
        assert np.all(A["Hp"][nh + 1:] == -7) and np.all(A["HTau"][nh:] == -7.0), "written beyond nh + 1 / nh entries"
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
            plan.h_sparse()
        assert e.value.code == ERR_INVALID
        assert plan.result_sizes()[1] == S.n                                 # the plan stays usable
    finally:
        plan.close()
    # an object without H: refused by name, and its R still comes out
    Q = make(pkg, "syn_grid2d", keep_h=False)
    try:
        with pytest.raises(pkg.StmmqrError, match="keepH") as e:
            Q.h_sparse()
        assert e.value.code == ERR_INVALID
        host, csc = Q.export_r(with_h=False), Q.r_sparse("csc")
        assert np.array_equal(csc["ptr"], host["Rp"]) and np.array_equal(csc["idx"], host["Ri"])
        assert np.array_equal(bits(csc["val"]), bits(host["Rx"]))
    finally:
        Q.close()


# ---- 6: the scratch layouts ----
@pytest.mark.parametrize("name", ["dwt_992", "bcsstk14"])
def test_scratch_layouts(pkg, exports, monkeypatch, name):
    want = exports(name)["dev"]
    for layout in LAYOUTS:
        for k in ("STMMQR_RECYCLE", "STMMQR_RESIDENT_CACHE"):
            monkeypatch.delenv(k, raising=False)
        for k, v in layout.items():
            monkeypatch.setenv(k, v)
        Q = make(pkg, name)
        try:
            got = Q.h_sparse()
            assert_same_arrays(got, want, f"{name} {layout}")
            assert np.array_equal(got["info"], want["info"]), f"{name} {layout}: info differs"
        finally:
            Q.close()


# ---- 7: a second factorization ----
@pytest.mark.parametrize("name", ["dwt_992", "bcsstk14"])
def test_after_refactorize(pkg, name):
    Ax2 = new_values(full_matrix(name)[4])
    Q, F = make(pkg, name), make(pkg, name, Ax2)
    try:
        first = Q.h_sparse()
        Q.refactorize(Ax2)
        got, want = Q.h_sparse(), F.h_sparse()
        assert_same_arrays(got, want, name + " against a new object")
        assert np.array_equal(got["info"], want["info"])
        assert_is_host(got, F.export_r(with_h=True), name + " against the new object's host export")
        assert first["Hx"].size and not (first["Hx"].shape == got["Hx"].shape and np.array_equal(first["Hx"], got["Hx"])), \
            "the new values changed nothing"
    finally:
        Q.close(); F.close()
