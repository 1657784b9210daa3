"""A numpy model of the packed factors (qr_rhpack, SURVEY.md A.6: the rule of k_rh_count / k_r_count) and of where the windows of
stmmqr_plan_download cut them (TEST INFRASTRUCTURE; no GPU, no torch).

* ``front_walk``      one front: per column its R rows and its packed length, with and without H -- the walk that
                      tests/test_gpu_qless.py (r_only_blocks) and tests/test_gpu_rsparse.py (stored_and_zero) share
* ``packed_layout``   every front's column offsets and the Post-order offsets of the blocks
* ``classify_edges``  the window edges (multiples of the window below rh_total) by what they cut, for kept and staged fronts
* ``aimed_windows``   windows that put an edge exactly on an R/H seam, a column start, a block start -- and into the pieces of a
                      small front that keeps its slab
* ``window_list``     the windows a test downloads with: generic ones + the aimed ones, at most MAX_WINDOWS windows per download

The classes of an edge at position p of the stack (p inside the non-empty block of front f, inside its non-empty column k):
  A  strictly inside a pivotal column                        B  strictly inside the R part of a non-pivotal column
  C  exactly on the R/H seam of a non-pivotal column with a non-empty H part
  D  strictly inside an H part                               E  exactly on a column start that is not a block start
  F  exactly on a block start                                I  inside or at either end of a dead pivot column of that block
and, counted per column / per block instead of per edge:
  G  a column with two or more edges strictly inside (the window is shorter than the column)
  H  a non-empty block with no edge strictly inside (the whole block inside one window)
C and D do not exist without H (keepH = 0).  The classes overlap: an edge inside a dead pivot column counts for A and for I."""
import numpy as np

I64 = np.int64
CLASSES = "ABCDEFGHI"
EXACT = "CEF"                  # the classes that need an edge at one exact position
INNER = "ABDI"                 # the classes of an edge anywhere inside a piece of a column
MAX_WINDOWS = 4096             # windows per download: what keeps a test to seconds


def front_walk(stair, fp, fn, fm):
    """qr_rhpack over the columns of one front (fp pivotal of fn columns, fm rows, Stair as downloaded): -> (rm_k, clen), int64[fn].
    rm_k[k]: the R rows column k stores (the live pivots among columns 0..k, at most fm; all of them for k >= fp) -- its length in
    the keepH = 0 layout.  clen[k]: its length in the R+H layout: a live pivot column its Stair, a dead one the R rows so far, a
    non-pivotal one the rm rows of R + the H rows h .. Stair-1 (h = min(rm + (k - fp) + 1, fm))."""
    rm_k, clen = np.zeros(fn, I64), np.zeros(fn, I64)
    if fm <= 0 or fn <= 0:
        return rm_k, clen
    rm = 0
    for k in range(fp):
        t = int(stair[k])
        if t == 0:
            t = rm                                    # dead: the R rows so far
        elif rm < fm:
            rm += 1
        rm_k[k], clen[k] = rm, t
    h = rm
    for k in range(fp, fn):
        t = int(stair[k])
        h = min(h + 1, fm)
        rm_k[k], clen[k] = rm, rm + max(t - h, 0)
    return rm_k, clen


def packed_layout(S, HStair, Hm, keep_h):
    """-> dict: per front (list "fronts", index = front) fp, fn, fm, rm, off (int64[fn + 1]: column offsets inside the block, off[fn] =
    the block's size), rlen / hlen (int64[fn]: R rows and rows below them of every column; a pivotal column is one piece of
    rlen + hlen entries), dead (bool[fn]); "block_off" / "block_size" (int64[nf], by front: the Post-order offsets = Rblock_off),
    "rh_total", "post", "keep_h"."""
    nf = int(S.nf)
    fronts = [None] * nf
    size = np.zeros(max(nf, 1), I64)
    for f in range(nf):
        fp = int(S.Super[f + 1] - S.Super[f])
        p1, fn = int(S.Rp[f]), int(S.Rp[f + 1] - S.Rp[f])
        fm = int(Hm[f])
        stair = np.asarray(HStair[p1:p1 + fn], I64)
        rm_k, clen = front_walk(stair, fp, fn, fm)
        if not keep_h:
            clen = rm_k.copy()
        assert np.all(clen >= rm_k), (f, "a live pivot column shorter than its R rows")
        off = np.zeros(fn + 1, I64)
        np.cumsum(clen, out=off[1:])
        dead = np.zeros(fn, bool)
        if fm > 0:
            dead[:fp] = stair[:fp] == 0
        fronts[f] = {"fp": fp, "fn": fn, "fm": fm, "rm": int(rm_k[-1]) if fn else 0, "off": off, "rlen": rm_k, "hlen": clen - rm_k,
                     "dead": dead}
        size[f] = off[fn]
    post = [int(f) for f in S.Post[:nf]]
    block_off = np.zeros(max(nf, 1), I64)
    run = 0
    for f in post:
        block_off[f] = run
        run += int(size[f])
    return {"fronts": fronts, "block_off": block_off, "block_size": size, "rh_total": int(run), "post": post, "keep_h": bool(keep_h),
            "nf": nf}


def _columns(layout):
    """the non-empty columns of the non-empty blocks in stack order, as parallel arrays (memoized in the layout)"""
    if "_cols" in layout:
        return layout["_cols"]
    front, start, ln, rl, piv, dead, first = [], [], [], [], [], [], []
    dfront, dstart, dend = [], [], []                 # dead pivot columns of non-empty blocks, empty ones included
    for f in layout["post"]:
        F = layout["fronts"][f]
        if layout["block_size"][f] <= 0:
            continue
        b0 = int(layout["block_off"][f])
        clen = F["rlen"] + F["hlen"]
        ks = np.flatnonzero(clen > 0)
        front.append(np.full(ks.size, f, I64)); start.append(b0 + F["off"][ks]); ln.append(clen[ks]); rl.append(F["rlen"][ks])
        piv.append(ks < F["fp"]); dead.append(F["dead"][ks])
        kd = np.flatnonzero(F["dead"])
        dfront.append(np.full(kd.size, f, I64)); dstart.append(b0 + F["off"][kd]); dend.append(b0 + F["off"][kd + 1])
    cat = lambda v, t: np.concatenate(v).astype(t) if v else np.zeros(0, t)
    c = {"front": cat(front, I64), "start": cat(start, I64), "len": cat(ln, I64), "rlen": cat(rl, I64), "piv": cat(piv, bool),
         "dead": cat(dead, bool), "dfront": cat(dfront, I64), "dstart": cat(dstart, I64), "dend": cat(dend, I64)}
    blocks = np.array([f for f in layout["post"] if layout["block_size"][f] > 0], I64)
    c["blocks"] = blocks
    c["bstart"] = layout["block_off"][blocks] if blocks.size else np.zeros(0, I64)
    c["bend"] = c["bstart"] + (layout["block_size"][blocks] if blocks.size else 0)
    layout["_cols"] = c
    return c


def window_edges(layout, win):
    """the positions where a window of `win` doubles ends and the next begins: the multiples of win below rh_total"""
    return np.arange(int(win), layout["rh_total"], int(win), dtype=I64)


def kept_mask(layout, kept):
    """kept: the fronts that keep their slab (any iterable of front numbers) -> bool[nf]"""
    m = np.zeros(max(layout["nf"], 1), bool)
    for f in kept:
        m[int(f)] = True
    return m


def classify_edges_per_front(layout, win):
    """-> int64[nf, len(CLASSES)]: per front, how many edges (columns for G, blocks for H) of each class the windows of `win`
    doubles give (module docstring)"""
    c = _columns(layout)
    out = np.zeros((max(layout["nf"], 1), len(CLASSES)), I64)
    E = window_edges(layout, win)

    def add(cl, fronts):
        np.add.at(out[:, CLASSES.index(cl)], fronts, 1)
    if c["start"].size == 0:
        return out
    if E.size:
        j = np.searchsorted(c["start"], E, side="right") - 1         # the column that holds the edge (E < rh_total: there is one)
        f, s, ln, rl, piv = c["front"][j], c["start"][j], c["len"][j], c["rlen"][j], c["piv"][j]
        r = E - s
        add("A", f[piv & (r > 0)])
        add("B", f[~piv & (r > 0) & (r < rl)])
        if layout["keep_h"]:
            add("C", f[~piv & (r == rl) & (ln > rl)])
            add("D", f[~piv & (r > rl)])
        b = np.searchsorted(c["bstart"], E, side="right") - 1
        at_block = c["bstart"][b] == E
        add("E", f[(r == 0) & ~at_block])
        add("F", f[at_block])
        if c["dstart"].size:
            d = np.searchsorted(c["dstart"], E, side="right") - 1    # the last dead column (stack order) that starts at or before the edge
            ok = d >= 0
            d = np.maximum(d, 0)
            ok &= (c["dend"][d] >= E) & (c["dfront"][d] == f)
            add("I", f[ok])
        # G: per column, the edges strictly inside
        inside = j[r > 0]
        if inside.size:
            cols, cnt = np.unique(inside, return_counts=True)
            add("G", c["front"][cols[cnt >= 2]])
    # H: per block, no edge strictly inside: the first multiple of win above bstart is at or beyond bend
    nxt = (c["bstart"] // int(win) + 1) * int(win)
    add("H", c["blocks"][nxt >= c["bend"]])
    return out


def classify_edges(layout, kept, win):
    """-> {"kept": {class: count}, "staged": {class: count}} for the windows of `win` doubles and the fronts `kept`"""
    M = classify_edges_per_front(layout, win)
    km = kept_mask(layout, kept)
    return {who: {cl: int(M[m, i].sum()) for i, cl in enumerate(CLASSES)} for who, m in (("kept", km), ("staged", ~km))}


def class_positions(layout, cl):
    """-> (positions, fronts): where an edge would be of the exact class cl (one of EXACT), ascending, 0 < p < rh_total, and the
    front each position belongs to (memoized in the layout)"""
    memo = layout.setdefault("_pos", {})
    if cl not in memo:
        c = _columns(layout)
        if cl == "C":
            sel = ~c["piv"] & (c["len"] > c["rlen"]) if layout["keep_h"] else np.zeros(c["start"].size, bool)
            p, f = (c["start"] + c["rlen"])[sel], c["front"][sel]
        else:
            is_block = np.isin(c["start"], c["bstart"])
            sel = is_block if cl == "F" else ~is_block
            p, f = c["start"][sel], c["front"][sel]
        ok = (p > 0) & (p < layout["rh_total"])
        memo[cl] = (p[ok], f[ok])
    return memo[cl]


def class_intervals(layout, cl):
    """-> (lo, hi, fronts): per column the positions lo .. hi (inclusive; lo > hi: none) where an edge would be of the class cl, one
    of INNER, in stack order (memoized in the layout)"""
    memo = layout.setdefault("_int", {})
    if cl not in memo:
        c = _columns(layout)
        s, e, r = c["start"], c["start"] + c["len"], c["start"] + c["rlen"]
        if cl == "A":
            sel, lo, hi, f = c["piv"], s + 1, e - 1, c["front"]
        elif cl == "B":
            sel, lo, hi, f = ~c["piv"], s + 1, r - 1, c["front"]
        elif cl == "D":
            sel, lo, hi, f = ~c["piv"] & layout["keep_h"], r + 1, e - 1, c["front"]
        else:                                           # I: a dead pivot column, its ends included, inside its own block
            bend = (layout["block_off"] + layout["block_size"])[c["dfront"]]
            sel, lo, hi, f = np.ones(c["dstart"].size, bool), np.maximum(c["dstart"], 1), np.minimum(c["dend"], bend - 1), c["dfront"]
        memo[cl] = (lo[sel], hi[sel], f[sel])
    return memo[cl]


def aimed_windows(layout, kept, cap=MAX_WINDOWS):
    """-> {(who, class): window} for who in kept / staged.
    The exact classes C, E, F: an edge lands on position p exactly when the window divides p; of the divisors of p that are at most
    p, give at least two windows (d < rh_total) and at most `cap` windows per download (d >= rh_total / cap) the largest is p itself
    where p >= rh_total / cap, and there is none otherwise.  Target: the first position of the class from rh_total / cap on (the
    most windows).
    The classes A, B, D, I, which the generic windows hit in a large front but may miss in a small one that keeps its slab: the
    window is the last position of the class (the fewest windows).  G: the largest window with two edges inside one column.
    A class the layout does not have for `who` is left out."""
    total = layout["rh_total"]
    least = max(1, -(-total // int(cap)))
    km = kept_mask(layout, kept)
    out = {}
    for cl in EXACT:
        p, f = class_positions(layout, cl)
        big = p >= least
        for who, m in (("kept", km[f] & big), ("staged", ~km[f] & big)):
            i = np.flatnonzero(m)
            if i.size:
                out[(who, cl)] = int(p[i[0]])
    for cl in INNER:
        lo, hi, f = class_intervals(layout, cl)
        ok = (hi >= np.maximum(lo, least)) & (hi < total)
        for who, m in (("kept", km[f] & ok), ("staged", ~km[f] & ok)):
            i = np.flatnonzero(m)
            if i.size:
                out[(who, cl)] = int(hi[i[-1]])
    c = _columns(layout)
    for who, m in (("kept", km[c["front"]]), ("staged", ~km[c["front"]])):
        i = np.flatnonzero(m & (c["len"] >= 2 * least + 1))
        if i.size:
            q = i[np.argmax(c["len"][i])]               # the longest column: open interval (a, b)
            a, b = int(c["start"][q]), int(c["start"][q] + c["len"][q])
            for w in range((b - a - 1) // 2 + 1, least - 1, -1):
                if w >= 1 and (a // w + 2) * w < b:     # the first two multiples of w above a
                    out[(who, "G")] = w
                    break
    return out


def generic_windows(total):
    g = [1] if total <= MAX_WINDOWS else []
    return g + [61, 64, 257, -(-total // 3), -(-total // 2), total - 1, total, total + 1]


def window_list(layout, kept):
    """the windows (doubles) a test downloads with: the generic ones and the aimed ones, each raised to where a download takes at
    most MAX_WINDOWS windows, without duplicates, ascending.  Never empty for a non-empty stack."""
    total = layout["rh_total"]
    if total <= 0:
        return [1]
    least = -(-total // MAX_WINDOWS)
    ws = generic_windows(total) + list(aimed_windows(layout, kept).values())
    return sorted({max(int(w), least, 1) for w in ws})
