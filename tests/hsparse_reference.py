"""A numpy model of H as the sparse export defines it (TEST INFRASTRUCTURE; no GPU, no torch): the walk of walk_packed
(csrc/stmmqr_export.cpp, n1rows = 0) over a packed R+H stack as stmmqr_plan_download or the reference's qr_factorize return it.

Slots (front f ascending, k = 0 .. fn - 1).  k < fp: t = Stair[k]; a dead column (t == 0) sets t = rm, a live one does rm++ (at most
fm); both h = rm.  k >= fp: h = min(h + 1, fm).  Column k of the packed block holds rm entries of R and then, where t >= h, the front
rows h .. t - 1.  The slot is a column of H iff t >= h and Tau[k] != 0.0: the unit diagonal (Hii[Hip[f] + h - 1], 1.0), then the
entries of rows h .. t - 1 with value != 0.0 in that order (row id Hii[Hip[f] + i]); exact zeros, -0.0 included, are dropped."""
import numpy as np

I64 = np.int64


def walk_h(S, Stack, Rblock_off, HStair, HTau, Hii, Hm):
    """S: nf, Super, Rp, Hip (the symbolic arrays); Stack / Rblock_off / HStair / HTau / Hii / Hm as downloaded (Hii after qr_hpinv).
    -> {"nh", "Hp", "Hi", "Hx", "HTau", "zeros": exact zeros among the H parts of the columns of H, "visited": entries before the zero
    test, unit diagonals included, "longest": the most rows below a diagonal}"""
    Stack = np.asarray(Stack, np.float64)
    Hp, Hi, Hx, Tau = [0], [], [], []
    zeros = visited = longest = 0
    for f in range(int(S.nf)):
        p = int(Rblock_off[f])
        col1, pr, hip = int(S.Super[f]), int(S.Rp[f]), int(S.Hip[f])
        fp, fn, fm = int(S.Super[f + 1]) - col1, int(S.Rp[f + 1]) - pr, int(Hm[f])
        rm = h = t = 0
        for k in range(fn):
            if k < fp:
                t = int(HStair[pr + k])
                if t == 0:
                    t = rm
                elif rm < fm:
                    rm += 1
                h = rm
            else:
                t = int(HStair[pr + k])
                h = min(h + 1, fm)
            p += rm                                                          # the R part
            if t < h:
                continue
            tau = HTau[pr + k]
            if tau != 0.0:
                v = Stack[p:p + (t - h)]
                keep = v != 0.0
                rows = np.asarray(Hii[hip + h:hip + t], I64)
                Hi.append(np.concatenate([[int(Hii[hip + h - 1])], rows[keep]]).astype(I64))
                Hx.append(np.concatenate([[1.0], v[keep]]))
                Tau.append(tau)
                Hp.append(Hp[-1] + 1 + int(np.count_nonzero(keep)))
                zeros += int(v.size - np.count_nonzero(keep))
                visited += 1 + int(v.size)
                longest = max(longest, int(v.size))
            p += t - h
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return {"nh": len(Tau), "Hp": np.asarray(Hp, I64), "Hi": cat(Hi, I64), "Hx": cat(Hx, np.float64), "HTau": np.asarray(Tau, np.float64),
            "zeros": zeros, "visited": visited, "longest": longest}


def walk_h_of_download(S, N):
    """walk_h on what HipQR.download() returned"""
    return walk_h(S, N.Stack, N.Rblock_off, N.HStair, N.HTau, N.Hii, N.Hm)


def apply_reflectors(H, X):
    """X (m or m x k, the caller's row order) -> H_{nh-1} .. H_0 applied to X scattered through HPinv: Q'X in the permuted row order"""
    X = np.asarray(X, np.float64)
    W = np.zeros_like(X)
    W[np.asarray(H["HPinv"], I64)] = X
    Hp, Hi, Hx, Tau = H["Hp"], H["Hi"], H["Hx"], H["HTau"]
    for q in range(Tau.size):
        i, v = Hi[Hp[q]:Hp[q + 1]], Hx[Hp[q]:Hp[q + 1]]
        W[i] -= np.multiply.outer(v, Tau[q] * (v @ W[i]))
    return W
