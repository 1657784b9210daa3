"""Factors without H (QRsym->keepH = 0) and the least-squares solve by the corrected seminormal equations on the GPU.

The R-only pack only moves data, so it is checked bit for bit against a restatement of qr_rhpack's keepH = 0 loop
(SparseQR_factorize.c:1691-1784) applied to the R+H blocks of a keepH = 1 factorization with the same plan settings."""
import importlib
import os

import numpy as np
import pytest
import scipy.sparse as sp

from pack_window_cases import front_walk
from stmmqr_testlib import EPS, Symbolic, cond_probe, load_golden, numeric_from_gpu, scalar, solve_tol

pytestmark = pytest.mark.gpu

PACK_NAMES = ["syn_grid3d", "syn_rankdef_grid", "syn_dupcol", "dwt_992", "lns_3937", "epb1", "bayer10", "cvxqp3"]
SOLVE_NAMES = ["syn_grid3d", "syn_rankdef_grid", "dwt_992", "lns_3937", "bayer10"]


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("stm-multifrontal-qr-factorization-empowered-by-gcn_amd")
    assert p.device_count() >= 1
    return p


@pytest.fixture
def env():
    """set environment knobs for the plans created inside a test, restored afterwards"""
    saved = {}

    def put(**kw):
        for k, v in kw.items():
            saved.setdefault(k, os.environ.get(k))
            os.environ[k] = str(v)
    yield put
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def plan_for(pkg, g, keep_h):
    S = Symbolic(g)
    sym = {**S.sc, **{k: v for k, v in S.arr.items() if v is not None}, "keepH": 1 if keep_h else 0}
    plan = pkg.HipQR(sym)
    plan.fstats = plan.factorize(g["in_Ax"], scalar(g, "in_tol"), int(scalar(g, "in_ntol")), g["in_Ap"], g["in_Ai"])
    return S, plan


def r_only_blocks(S, N):
    """qr_rhpack's keepH = 0 loop, front by front, on the R+H blocks of a keepH = 1 download (its HStair and Hm): the R part
    of every column.  -> list of blocks in Post order"""
    out = []
    for f in S.Post[:S.nf]:
        f = int(f)
        fp = int(S.Super[f + 1] - S.Super[f])
        p1, fn = int(S.Rp[f]), int(S.Rp[f + 1] - S.Rp[f])
        fm = int(N.Hm[f])
        stair = N.HStair[p1:p1 + fn]
        src = N.Stack[int(N.Rblock_off[f]):]
        blk = []
        rm_k, clen = front_walk(stair, fp, fn, fm)      # R+H column k: clen[k] entries, R = the first rm_k[k]
        at = 0
        for k in range(fn if fm > 0 else 0):
            blk.append(src[at:at + int(rm_k[k])])
            at += int(clen[k])
        out.append(np.concatenate(blk) if blk else np.zeros(0))
    return out


def check_r_only_pack(S, N1, N0, rdead=True):
    blocks = r_only_blocks(S, N1)
    ref = np.concatenate(blocks) if blocks else np.zeros(0)
    assert N0.Stack.size == ref.size
    assert np.array_equal(N0.Stack.view(np.uint64), ref.view(np.uint64))
    sizes = np.zeros(S.nf, np.int64)
    sizes[S.Post[:S.nf]] = [b.size for b in blocks]
    off = np.zeros(S.nf, np.int64)
    run = 0
    for f in S.Post[:S.nf]:
        off[f] = run
        run += sizes[f]
    assert np.array_equal(np.asarray(N0.Rblock_off)[:S.nf], off)
    if rdead:
        assert np.array_equal(np.asarray(N0.Rdead[:S.n]), np.asarray(N1.Rdead[:S.n]))
    assert (N0.rank, N0.rank1, N0.maxfrank) == (N1.rank, N1.rank1, N1.maxfrank)


@pytest.mark.parametrize("name", PACK_NAMES)
@pytest.mark.parametrize("recycle", ["0", "2", "2-overflow"])
def test_r_only_pack_bits(pkg, env, name, recycle):
    env(STMMQR_RECYCLE=recycle[0])
    if recycle.endswith("overflow"):
        env(STMMQR_RH_EST_SCALE="0.3")                   # (the arena sized below the factors: the overflow retry)
    g = load_golden(name)
    S, p1 = plan_for(pkg, g, True)
    _, p0 = plan_for(pkg, g, False)
    try:
        assert p1.keep_h and not p0.keep_h
        N1, N0 = p1.download(), p0.download()
        check_r_only_pack(S, N1, N0)
        if N1.Stack.size:
            assert N0.Stack.size < N1.Stack.size or N1.rank == 0
        if recycle.endswith("overflow") and N0.Stack.size > 16384:
            # (an arena of 0.3 x the estimate + 4096 cannot hold these factors: k_r_count flags the overflow, the factorization is
            #  repeated once with the arena at its hard bound)
            assert p0.fstats["retries"] == 1
    finally:
        p1.close(); p0.close()


@pytest.mark.parametrize("name", ["xenon1_standin", "c5mini_standin"])
def test_r_only_device_bytes(pkg, name):
    g = load_golden(name)
    out = {}
    for keep in (True, False):
        _, p = plan_for(pkg, g, keep)
        try:
            out[keep] = (p.device_bytes(), p.result_sizes()[0])
        finally:
            p.close()
    print(f"[device bytes] {name}: keepH=1 {out[True][0] / 1e9:.3f} GB ({out[True][1]} packed), "
          f"keepH=0 {out[False][0] / 1e9:.3f} GB ({out[False][1]} packed)")
    assert out[False][1] < out[True][1]
    assert out[False][0] < out[True][0]


def rsolve_or_error(pkg, plan, system, B):
    try:
        return plan.rsolve(system, B)
    except pkg.StmmqrError as e:
        return str(e)


@pytest.mark.parametrize("name", SOLVE_NAMES)
@pytest.mark.parametrize("cache", ["0", "1"])
def test_rsolve_same_bits(pkg, env, name, cache):
    env(STMMQR_RECYCLE="2", STMMQR_RESIDENT_CACHE=cache)
    g = load_golden(name)
    S, p1 = plan_for(pkg, g, True)
    _, p0 = plan_for(pkg, g, False)
    try:
        rng = np.random.default_rng(3)
        for system in range(4):
            rows = S.m if system <= 1 else S.n
            for nrhs in (1, 33):
                B = rng.standard_normal((rows, nrhs))
                x1 = rsolve_or_error(pkg, p1, system, B)
                x0 = rsolve_or_error(pkg, p0, system, B)
                if isinstance(x1, str):
                    assert x0 == x1
                    continue
                assert np.array_equal(x0.view(np.uint64), x1.view(np.uint64)), (system, nrhs)
    finally:
        p1.close(); p0.close()


def test_refusals(pkg):
    g = load_golden("dwt_992")
    S, p0 = plan_for(pkg, g, False)
    try:
        X = np.ones(S.m)
        for method in range(4):
            with pytest.raises(pkg.StmmqrError, match="keepH"):
                p0.qmult(method, X if method <= 1 else X.reshape(1, -1))
        with pytest.raises(pkg.StmmqrError, match="keepH"):
            p0.solve(X)
        with pytest.raises(pkg.StmmqrError, match="keepH"):
            p0.set_groups(np.ones(S.nf, np.int32))
        x = p0.rsolve(0, X)                              # the plan stays usable
        assert np.all(np.isfinite(x))
    finally:
        p0.close()
    Ap, Ai, Ax = g["in_Ap"], g["in_Ai"], g["in_Ax"]
    q = pkg.SparseQR(S.m, S.n, Ap, Ai, Ax, keep_h=False)
    try:
        with pytest.raises(pkg.StmmqrError, match="keepH"):
            q.qmult(0, np.ones(S.m))
        with pytest.raises(pkg.StmmqrError, match="keepH"):
            q.export_r(with_h=True)
        R = q.export_r(with_h=False)
        assert R["Rp"][-1] > 0
        x = q.solve(0, np.ones(S.m))
        assert np.all(np.isfinite(x))
    finally:
        q.close()


def seam_sym(g, keep_h):
    S = Symbolic(g)
    return S, {**S.sc, **{k: v for k, v in S.arr.items() if v is not None}, "keepH": keep_h}


@pytest.mark.parametrize("name", ["syn_rankdef_grid", "lns_3937", "bayer10"])
def test_seam_keeph_sequence(pkg, env, name):
    env(STMMQR_PLAN_CACHE="2")
    g = load_golden(name)
    args = (g["in_Ap"], g["in_Ai"], g["in_Ax"], scalar(g, "in_tol"), int(scalar(g, "in_ntol")))
    S, _ = seam_sym(g, 1)
    _, p1 = plan_for(pkg, g, True)
    try:
        N1 = p1.download()
    finally:
        p1.close()
    pkg.plan_cache_clear()
    try:
        for keep in (1, 0, 1):                           # through the seam's plan cache: the key holds keepH
            N = pkg.qr_factorize_seam(seam_sym(g, keep)[1], *args)
            try:
                assert int(N._p.contents.keepH) == keep
                a = N.arrays()
                if keep:
                    assert np.array_equal(a["Stack"].view(np.uint64), N1.Stack.view(np.uint64))
                    continue
                assert int(N._p.contents.maxfm) == -1       # (qr_hpinv sets it: not run without H)
                G = type("G", (), {})()
                G.Stack, G.Rblock_off = a["Stack"], a["Rblock_off"]
                G.rank, G.rank1, G.maxfrank = (int(getattr(N._p.contents, k)) for k in ("rank", "rank1", "maxfrank"))
                check_r_only_pack(S, N1, G, rdead=False)     # (Rdead: checked on the plan's download, test_r_only_pack_bits)
            finally:
                N.close()
    finally:
        pkg.plan_cache_clear()


@pytest.mark.parametrize("name", ["syn_grid3d", "dwt_992", "lns_3937", "bayer10"])
def test_spmv(pkg, name):
    g = load_golden(name)
    S, p = plan_for(pkg, g, False)
    try:
        A = sp.csc_matrix((g["in_Ax"], g["in_Ai"], g["in_Ap"]), shape=(S.m, S.n))
        absA = abs(A)
        rng = np.random.default_rng(9)
        for trans in (0, 1):
            M, Mabs = (A.T.tocsr(), absA.T.tocsr()) if trans else (A.tocsr(), absA.tocsr())
            rows = S.m if trans else S.n
            for nrhs in (1, 5, 32, 40):
                X = rng.standard_normal((rows, nrhs))
                Y = p.spmv(X, trans)
                bound = 8 * EPS * (Mabs @ np.abs(X))
                assert np.all(np.abs(Y - M @ X) <= bound), (trans, nrhs)
                Y2 = p.spmv(X, trans)
                assert np.array_equal(Y.view(np.uint64), Y2.view(np.uint64))
                for j in (0, nrhs - 1):
                    y = p.spmv(X[:, j], trans)
                    assert np.array_equal(y.view(np.uint64), Y[:, j].view(np.uint64))
    finally:
        p.close()


@pytest.mark.parametrize("name", ["syn_grid3d", "syn_grid2d", "syn_chain", "syn_rand60x40", "epb1", "t2d_q9"])
def test_seminormal_full_rank(pkg, oracle, name):
    g = load_golden(name)
    S, p1 = plan_for(pkg, g, True)
    _, p0 = plan_for(pkg, g, False)
    try:
        N1 = p1.download()
        assert N1.rank == S.n
        kappa = cond_probe(oracle, S, numeric_from_gpu(S, N1))
        assert kappa <= 1e6, kappa
        rng = np.random.default_rng(4)
        A = sp.csc_matrix((g["in_Ax"], g["in_Ai"], g["in_Ap"]), shape=(S.m, S.n))
        B = A @ rng.standard_normal((S.n, 3))
        B[:, 1] += 1e-3 * rng.standard_normal(S.m)      # inconsistent
        B[:, 2] = rng.standard_normal(S.m)
        X1, info1 = p1.solve_seminormal(B, refine=1)
        X0, info0 = p0.solve_seminormal(B, refine=1)
        assert np.array_equal(X0.view(np.uint64), X1.view(np.uint64)) and info0 == info1
        Xq = p1.solve(B)
        d = np.linalg.norm(X0 - Xq, axis=0) / np.maximum(np.linalg.norm(Xq, axis=0), 1e-300)
        print(f"[csne] {name} cond_probe {kappa:.2e} diff {d.max():.2e} allowed {solve_tol(kappa):.1e} info {info0:.2e}")
        assert np.all(d <= solve_tol(kappa))
        assert info0 <= 1e-12
    finally:
        p1.close(); p0.close()


@pytest.mark.parametrize("name", ["bayer10", "ex18"])
def test_seminormal_info_recomputed(pkg, name):
    g = load_golden(name)
    S, p = plan_for(pkg, g, False)
    try:
        A = sp.csc_matrix((g["in_Ax"], g["in_Ai"], g["in_Ap"]), shape=(S.m, S.n))
        B = np.random.default_rng(2).standard_normal((S.m, 2))
        X, info = p.solve_seminormal(B, refine=1)
        assert np.all(np.isfinite(X))
        af = np.linalg.norm(g["in_Ax"])
        den = [af * (af * np.linalg.norm(X[:, j]) + np.linalg.norm(B[:, j])) for j in range(2)]
        host = max(np.linalg.norm(A.T @ (B[:, j] - A @ X[:, j])) / den[j] for j in range(2))
        # A'r of a least-squares solution is rounding noise: two evaluations in different summation orders agree to 1e-10 only
        # where that noise allows; the bound is the rounding error of forming A'(b - A x) in double precision
        absA = abs(A)
        noise = max(np.linalg.norm(absA.T @ (np.abs(B[:, j]) + absA @ np.abs(X[:, j]))) / den[j] for j in range(2))
        print(f"[csne info] {name} device {info:.3e} host {host:.3e} rounding bound {64 * EPS * noise:.1e}")
        assert abs(info - host) <= max(1e-10 * host, 64 * EPS * noise)
    finally:
        p.close()


@pytest.mark.parametrize("name", ["syn_rankdef_grid", "syn_dupcol", "dwt_992", "lns_3937"])
def test_seminormal_rank_deficient(pkg, name):
    g = load_golden(name)
    S, p = plan_for(pkg, g, False)
    try:
        N = p.download()
        assert N.rank < S.n
        B = np.random.default_rng(6).standard_normal((S.m, 2))
        X, info = p.solve_seminormal(B, refine=2)
        assert np.all(np.isfinite(X)) and np.isfinite(info)
        q = S.Qfill if S.Qfill is not None else np.arange(S.n)
        dead = q[np.flatnonzero(np.asarray(N.Rdead[:S.n]) != 0)]
        assert dead.size == S.n - N.rank
        assert np.all(X[dead, :] == 0.0)
    finally:
        p.close()


def seminormal_by_parts(p, B):
    """x = E R^-1 R^-T E' A'b spelled out with the plan's own operations: the launches of solve_seminormal(refine=0), batch by batch"""
    return p.rsolve(1, p.rsolve(3, p.spmv(B, 1)))


def check_seminormal_parts(pkg, name, keep_h, nrhs):
    g = load_golden(name)
    S, p = plan_for(pkg, g, keep_h)
    try:
        if name == "syn_rankdef_grid":
            assert p.download().rank < S.n                 # (dead columns; its Qfill is no identity)
        B = np.random.default_rng(17).standard_normal((S.m, nrhs))
        X, _ = p.solve_seminormal(B, refine=0)
        Xp = seminormal_by_parts(p, B)
        assert np.array_equal(X.view(np.uint64), Xp.view(np.uint64))
    finally:
        p.close()


@pytest.mark.parametrize("name", ["syn_grid2d", "syn_rankdef_grid"])
@pytest.mark.parametrize("keep_h", [False, True])
@pytest.mark.parametrize("nrhs", [3, 33])
def test_seminormal_equals_its_parts(pkg, name, keep_h, nrhs):
    """the fused solve runs the passes that rsolve and spmv run one by one: the same bits, with a full batch of 32 plus one as well"""
    check_seminormal_parts(pkg, name, keep_h, nrhs)


@pytest.mark.parametrize("keep_h", [False, True])
def test_seminormal_equals_its_parts_level_rebuild(pkg, env, keep_h):
    """... with recycled slabs and no cache of the front forms: every pass puts every level back into front form"""
    env(STMMQR_RECYCLE="2", STMMQR_RESIDENT_CACHE="0")
    check_seminormal_parts(pkg, "syn_rankdef_grid", keep_h, 33)


def test_seminormal_too_wide_front(pkg):
    """c5mini_standin has a front too wide for the one-workgroup R' solve: on a FRESH plan (nothing resident-factor related has run
    yet) the seminormal solve returns the error of rsolve system 3, before any launch of the solve"""
    g = load_golden("c5mini_standin")
    S, p = plan_for(pkg, g, False)
    try:
        with pytest.raises(pkg.StmmqrError) as e:
            p.solve_seminormal(np.ones(S.m))
        assert e.value.code == -3
    finally:
        p.close()
    _, q = plan_for(pkg, g, False)
    try:
        with pytest.raises(pkg.StmmqrError) as e3:
            q.rsolve(3, np.ones(S.n))
        assert e3.value.code == -3 and str(e3.value).split(": ", 1)[1] == str(e.value).split(": ", 1)[1]
        x = q.rsolve(0, np.ones(S.m))                 # (the plan stays usable)
        assert np.all(np.isfinite(x))
    finally:
        q.close()


@pytest.mark.parametrize("name", ["syn_rankdef_grid", "dwt_992", "lns_3937"])
def test_export_r_without_h(pkg, name):
    """qr_rcount / qr_rconvert on an R-only stack (walk_packed's keepH = 0 branch) give the R of the R+H stack"""
    g = load_golden(name)
    m, n = int(scalar(g, "in_m")), int(scalar(g, "in_n"))
    out = {}
    for keep in (True, False):
        q = pkg.SparseQR(m, n, g["in_Ap"], g["in_Ai"], g["in_Ax"], keep_h=keep)
        try:
            out[keep] = q.export_r(with_h=False)
        finally:
            q.close()
    for k in ("Rp", "Ri"):
        assert np.array_equal(out[False][k], out[True][k])
    assert np.array_equal(out[False]["Rx"].view(np.uint64), out[True]["Rx"].view(np.uint64))


@pytest.mark.parametrize("name", ["bayer10", "ex18"])
@pytest.mark.parametrize("refine", [0, 1])
def test_seminormal_info_from_device_products(pkg, name, refine):
    """info is |A'r| / (|A|_F (|A|_F |x| + |b|)) of the RETURNED x: recomputed from the same products (spmv gives the bits the
    solve's residual and A'r have), only the norms are summed in another order -- so it matches to 1e-10 however small A'r is"""
    g = load_golden(name)
    S, p = plan_for(pkg, g, False)
    try:
        B = np.random.default_rng(2).standard_normal((S.m, 2))
        X, info = p.solve_seminormal(B, refine=refine)
        Z = p.spmv(B - p.spmv(X, 0), 1)
        af = np.linalg.norm(g["in_Ax"])
        ref = max(np.linalg.norm(Z[:, j]) / (af * (af * np.linalg.norm(X[:, j]) + np.linalg.norm(B[:, j]))) for j in range(2))
        print(f"[csne info from products] {name} refine {refine}: device {info:.6e} recomputed {ref:.6e}")
        assert ref > 0 and abs(info - ref) <= 1e-10 * ref
    finally:
        p.close()


def test_sparseqr_seminormal_with_singletons(pkg):
    """the SparseQR-level seminormal solve (full A on the device, singleton rows through stmmqr_sparseqr_solve) against the Q-based
    least-squares solution, on a full-rank matrix with a column singleton; with and without H the same bits"""
    from test_gpu_sparseqr import driver_tol
    g = load_golden("syn_star")
    m, n = int(g["A_m"][0]), int(g["A_n"][0])
    Ap, Ai, Ax = g["A_p"], g["A_i"], g["A_x"]
    kw = dict(ordering=7, tol=driver_tol(m, n, Ap, Ax), relax=pkg.relax_for_qr(n, int(Ap[-1])))
    q1 = pkg.SparseQR(m, n, Ap, Ai, Ax, **kw)
    q0 = pkg.SparseQR(m, n, Ap, Ai, Ax, keep_h=False, **kw)
    try:
        assert q1.info["n1cols"] > 0 and int(q1.info["rank"]) == n
        A = sp.csc_matrix((Ax, Ai, Ap), shape=(m, n))
        rng = np.random.default_rng(8)
        B = A @ rng.standard_normal((n, 2))
        B[:, 1] += 1e-3 * rng.standard_normal(m)
        X1, info1 = q1.solve_seminormal(B, refine=1)
        X0, info0 = q0.solve_seminormal(B, refine=1)
        assert np.array_equal(X0.view(np.uint64), X1.view(np.uint64)) and info0 == info1
        Xq = q1.solve(1, q1.qmult(0, B))
        d = np.linalg.norm(X0 - Xq, axis=0) / np.linalg.norm(Xq, axis=0)
        print(f"[sparseqr csne] syn_star diff {d.max():.2e} info {info0:.2e}")
        assert np.all(d <= 1e-9) and info0 <= 1e-12
    finally:
        q1.close(); q0.close()
