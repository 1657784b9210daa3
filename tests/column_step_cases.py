"""Inputs of the column-step tests (tests/test_gpu_column_step.py) and of the pin against the parent build
(tests/golden/make_column_step_golden.py): dense fronts for qr_front whose panels take the column pipeline
(big_front_cols = 8, tall_min_rows = 0, panel_algo = 1), one row into each register class of its column groups and at its top."""
import hashlib

import numpy as np

I64 = np.int64
OPTIONS = dict(big_front_cols=8, tall_min_rows=0, panel_algo=1)
DEFAULTS = dict(big_front_cols=64, tall_min_rows=0, panel_algo=0)
NO_WAVE_PANEL = 16384          # STMMQR_DBG bit: short panels go through the multi-workgroup pipeline too
HEAD = 37                      # rows of F the pin keeps as numbers; the in-staircase entries below them are kept as digests


def staircase(m, n, seed, kind):
    rng = np.random.default_rng(seed)
    if kind == "full":
        return np.full(n, m, I64)
    if kind == "steps":        # irregular increments (1..3 rows per column) from the top, as tests/test_gpu_seams.py
        return np.minimum(m, 2 + np.cumsum(rng.integers(1, 4, n))).astype(I64)
    if kind == "tail":         # the same increments, ending at row m: every panel is as tall as the front
        c = np.cumsum(rng.integers(1, 4, n))
        return np.maximum(1, m - (c[-1] - c)).astype(I64)
    if kind == "diag12":       # the first 12 columns end at the diagonal (ss == 0, identity reflectors, t = g + 1), the others are full
        St = np.full(n, m, I64)
        St[:12] = np.arange(1, 13)
        return St
    raise ValueError(kind)


def make_front(m, n, seed, kind):
    St = staircase(m, n, seed, kind)
    rng = np.random.default_rng(seed + 1)
    F = np.zeros((m, n), order="F")
    for k in range(n):
        F[:St[k], k] = rng.standard_normal(St[k])
    return F, St


DEAD_AT = (3, 8, 15, 20)       # duplicates in the middle, first and last of an 8-column group; a zero column


def make_dead_front(m, n=37):
    F, St = make_front(m, n, 555 + m, "full")
    F[:, 3] = F[:, 1]
    F[:, 8] = F[:, 2]
    F[:, 15] = F[:, 5]
    F[:, 20] = 0.0
    return F, St


def run_front(pkg, F0, St0, npiv, tol, ntol):
    """qr_front on copies, every panel through the column pipeline.  Returns (rank, Tau, Rdead, flops, F, Stair)."""
    F, St = F0.copy(order="F"), St0.copy()
    m, n = F.shape
    pkg.set_options(**OPTIONS)
    try:
        r, Tau, Rdead, fl = pkg.qr_front(m, n, npiv, tol, ntol, F, St)
    finally:
        pkg.set_options(**DEFAULTS)
    return r, Tau, Rdead, fl, F, St


def in_staircase(St0, St, m):
    """(m, n) mask of the entries a column holds: rows below its staircase on entry or on return."""
    t = np.maximum(St0, St)
    return np.arange(m)[:, None] < t[None, :]


def pin(F, St0, St):
    """What the pin keeps of F: its first HEAD rows (zero outside the staircase) and one SHA-256 digest per column of the
    in-staircase entries below them (+ 0.0: the sign of a zero is not pinned)."""
    m, n = F.shape
    mask = in_staircase(St0, St, m)
    head = np.where(mask[:HEAD], F[:HEAD], 0.0) + 0.0
    dig = [hashlib.sha256((F[HEAD:, k][mask[HEAD:, k]] + 0.0).tobytes()).hexdigest() for k in range(n)]
    return head, np.array(dig)


# the fronts of the pin: name -> (kind, m, n, npiv, tol, ntol, STMMQR_DBG)
GOLDEN = {f"steps_{m}": ("steps", m, 37, 37, -1.0, 37, None) for m in (513, 1025, 2049)}
GOLDEN.update({f"tail_{m}": ("tail", m, 37, 37, -1.0, 37, NO_WAVE_PANEL if m == 300 else None) for m in (300, 513, 1025, 2049, 4097)})
GOLDEN["diag12_1025"] = ("diag12", 1025, 37, 37, -1.0, 37, None)
GOLDEN["dead_1025"] = ("dead", 1025, 37, 37, 1e-9, 37, None)
GOLDEN["runout_520"] = ("steps", 520, 600, 560, -1.0, 600, None)


def golden_case(name):
    """(front, npiv, tol, ntol, STMMQR_DBG) of a pinned case."""
    kind, m, n, npiv, tol, ntol, dbg = GOLDEN[name]
    front = make_dead_front(m, n) if kind == "dead" else make_front(m, n, 1234 + m, kind)
    return front, npiv, tol, ntol, dbg
