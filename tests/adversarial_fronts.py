"""Dense fronts whose rank decisions sit close to the tolerance, an extended-precision reference of the front
factorization, and the backward quantities that any correct factorization of such a front must reach
(TEST INFRASTRUCTURE, imports no GPU code).

The seeded Gaussian fronts of tests/test_gpu_seams.py never bring a column norm near tol and never make the Gram-based
panel (csrc/stmmqr_capanel.hip) refresh its Gram matrix.  Here some columns are a combination of columns before them plus
`delta` times a fresh unit vector: in exact arithmetic the pivot of such a column is |beta| = delta * (norm of the part of
the fresh vector orthogonal to the columns before), a large fraction of delta.  delta = 8 tol must stay live, delta =
tol / 8 must die; a column norm taken from a Gram matrix that was not refreshed is wrong by many orders there.  The crafted
columns sit at the edges of the 32-column panels and the 8-column sub-panels, fill one whole sub-panel (40..47), and the
last pivot (95 / 159) is dead.
"""
import hashlib

import numpy as np

I64 = np.int64
LD = np.longdouble
# x87 extended precision (64-bit mantissa) or better: the reference must be more accurate than what it judges
assert np.finfo(LD).eps < 1e-18, "np.longdouble is not an extended-precision type on this platform"

TOL = 1e-10
HI = 8 * TOL
LO = TOL / 8


def crafted_columns(n):
    """{k: (delta, span)} of make_adversarial for a front of n columns (n = 96 or 160)"""
    c = {7: (HI, 5), 8: (LO, 5), 31: (LO, 5), 32: (HI, 5), 33: (LO, 5), 63: (HI, 5), 64: (LO, 5), 95: (LO, 5),
         20: (1e-3, 20), 21: (1e-6, 21), 70: (1e-8, 6)}
    for k in range(40, 48):
        c[k] = (LO, 40)
    if n == 160:
        c.update({127: (LO, 5), 128: (HI, 5), 159: (LO, 5)})
    assert max(c) < n
    return dict(sorted(c.items()))


def make_adversarial(m, n, kind, seed=None, craft=True):
    """(F, Stair, crafted): staircase by the rules of make_front (tests/test_gpu_seams.py), Gaussian columns of unit
    expected norm, then the crafted columns written over them in increasing k.  craft = False: the same Gaussian front
    without the crafted columns (the draws of the Gaussian part are identical)."""
    rng = np.random.default_rng(5 + m if seed is None else seed)
    if kind == "full":
        St = np.full(n, m, I64)
    elif kind == "steps":
        inc = rng.integers(1, 4, n)
        St = np.minimum(m, 2 + np.cumsum(inc)).astype(I64)
    else:
        assert kind == "ramp"
        St = np.minimum(m, (np.arange(1, n + 1) * m) // n + 8).astype(I64)
    F = np.zeros((m, n), order="F")
    for k in range(n):
        F[:St[k], k] = rng.standard_normal(St[k]) / np.sqrt(St[k])
    crafted = crafted_columns(n)
    if craft:
        for k, (delta, span) in crafted.items():
            lo = max(0, k - span)
            c = rng.standard_normal(k - lo)
            w = np.zeros(m)
            w[:St[k]] = rng.standard_normal(St[k])
            w /= np.linalg.norm(w)
            base = F[:, lo:k] @ c
            F[:, k] = base / np.linalg.norm(base) + delta * w
    return F, St, crafted


_REF = {}


def ref_front(F, Stair, npiv, tol, ntol):
    """The unblocked column loop of the reference's qr_front in np.longdouble (fp64 restatement: classic_panel in
    tests/ca_model.py, oracle/stmmqr_oracle.c orc_front): (rank, Stair, Rdead, |beta| per column).  F and Stair are not
    modified; results are cached per argument tuple and returned read-only."""
    F = np.asarray(F)
    m, n = F.shape
    key = (m, n, hashlib.sha1(np.ascontiguousarray(F).tobytes()).hexdigest(), np.asarray(Stair, I64).tobytes(),
           int(npiv), float(tol), int(ntol))
    if key in _REF:
        return _REF[key]
    A = np.asfortranarray(F, dtype=LD)
    St = np.array(Stair, I64)
    npiv = min(n, max(0, int(npiv)))
    ntol = min(int(ntol), npiv)
    Rdead = np.zeros(max(npiv, 1), np.int8)
    absb = np.zeros(n, LD)
    rank = min(m, npiv)
    g = 0
    for k in range(n):
        if g >= m:                                # no rows left: remaining pivots are dead, remaining columns are empty
            Rdead[k:npiv] = 1
            St[k:npiv] = 0
            St[max(k, npiv):] = m
            break
        t = max(g + 1, int(St[k]))
        alpha = A[g, k]
        x = A[g + 1:t, k]
        ss = x @ x if x.size else LD(0)
        if ss == 0:
            beta, tau = alpha, LD(0)              # H = I
        else:
            beta = -np.copysign(np.sqrt(alpha * alpha + ss), alpha)
            tau = (beta - alpha) / beta
        absb[k] = abs(beta)
        if k < ntol and absb[k] <= tol:
            A[g:, k] = 0
            St[k] = 0
            Rdead[k] = 1
        else:
            St[k] = t
            if tau != 0:
                v = x / (alpha - beta)
                if k + 1 < n:
                    w = tau * (A[g, k + 1:] + v @ A[g + 1:t, k + 1:])
                    A[g, k + 1:] -= w
                    A[g + 1:t, k + 1:] -= np.outer(v, w)
                A[g + 1:t, k] = v
            A[g, k] = beta
            g += 1
        if k == npiv - 1:
            rank = g
    out = (int(rank), St, Rdead[:npiv], absb)
    for a in out[1:]:
        a.setflags(write=False)
    _REF[key] = out
    return out


def backward_metrics(F0, Fout, Stair_out, Tau, Rdead, npiv):
    """(e_live, e_dead, orth) of a front factorization as it was returned (R and the Householder vectors in Fout, Tau, the
    output staircase, the dead pivots), evaluated in long double.  Live columns take the pivot rows 0, 1, ... in order;
    the reflector of a live column on pivot row g is v = (1, Fout[g+1:t, k]) on the rows g..t-1, t = Stair_out[k].
      e_live = ||(F0 - QR)[:, live]||_F / ||F0||_F
      e_dead = largest column norm of F0 - QR over the dead columns (what the factorization dropped)
      orth   = ||Q1'Q1 - I||_F, Q1 = the first g columns of Q = H_1 ... H_g."""
    m, n = F0.shape
    R = np.zeros((m, n), LD, order="F")
    refl = []                                     # (pivot row, t, column, v, tau)
    live = np.zeros(n, bool)
    g = 0
    for k in range(n):
        dead = k < npiv and Rdead[k] != 0
        if dead or g >= m:
            R[:g, k] = Fout[:g, k]
            live[k] = not dead
            continue
        t = int(Stair_out[k])
        assert g < t <= m, (k, g, t)
        R[:g + 1, k] = Fout[:g + 1, k]
        v = np.ones(t - g, LD)
        v[1:] = Fout[g + 1:t, k]
        refl.append((g, t, k, v, LD(Tau[k])))
        live[k] = True
        g += 1
    # H_i leaves the columns before its own alone (they are zero on its rows), and likewise the unit vectors e_c, c < i
    Q1 = np.zeros((m, g), LD, order="F")
    Q1[np.arange(g), np.arange(g)] = 1
    for i, t, k, v, tau in reversed(refl):
        if tau == 0:
            continue
        R[i:t, k:] -= np.outer(v, tau * (v @ R[i:t, k:]))
        Q1[i:t, i:] -= np.outer(v, tau * (v @ Q1[i:t, i:]))
    E = np.asarray(F0, LD) - R
    cn = np.sqrt((E * E).sum(axis=0))
    e_live = float(np.sqrt((cn[live] ** 2).sum()) / np.sqrt((np.asarray(F0, LD) ** 2).sum()))
    e_dead = float(cn[~live].max()) if (~live).any() else 0.0
    Gm = Q1.T @ Q1
    Gm[np.arange(g), np.arange(g)] -= 1
    orth = float(np.sqrt((Gm * Gm).sum()))
    return e_live, e_dead, orth
