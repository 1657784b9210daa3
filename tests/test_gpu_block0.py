"""T + column block 0 of a riding step in one launch (k_upd_b0w: dev_k_upd_b0, csrc/stmmqr_update.hip) -- its two tile phases
alternate between two pairs of chunk images with one barrier per 64-row chunk, and phase 2 subtracts from the registers.

Yardstick: the serial kernels, which that change does not touch.  Every case factorizes ONE input under options.lookahead = 2 (the
default: the riding steps go through k_upd_b0w) and under lookahead = 0 (k_upd_w + k_upd_c for every column block) and asks for the
same bits in Stack[:rh_total], HTau, HStair, Rdead, Rblock_off and rank.  The same input then goes through the CPU oracle with the
checks of test_gpu_column_step.py::check_against_oracle (rank, staircase, Rdead and flops exact; Tau and the packed factors within
1e-11 of their 2-norms).

That the block-0 role really ran: the lookahead = 2 factorization runs with STMMQR_DBG = 32768, under which slab 0 of every block-0
workgroup set counts itself when it reaches the end of dev_k_upd_b0 and the host prints the count on stderr
(`[block-0 launch, ...] (count)`); the count must be the number of (riding step, front) pairs that block0_cases.riding_block0
derives from the shapes -- never zero.

Shapes (block0_cases.py): a front of 600 x 97 (three slabs: row-parallel steps) whose first 32 columns reach `first` rows, so that
panel 0 updates mp = first rows and panel 1 updates 568 (three slabs, the last one partial, every workgroup through the ticket).
mp = 33 .. 256 is the path of one slab without a ticket with one chunk, a partial second one, two .. four chunks (both
parities of the image pairs); 257 a second slab of one row; 320 and 513 two and three slabs with a partial last chunk.
Relative to the panel's first pivot row the unit diagonals of V are rows 0 .. 31 at most (one per live column), i.e. always inside
chunk 0; what a staircase moves is where the columns END -- "steps": inside chunk 0 and just behind it, "boundary": on rows 64
and 128 exactly.  Dead reflectors (pdiag = STM_BIGROW): two duplicate columns and a zero column in panel 0 under tol = 1e-9.

Block 0 of a riding step of ONE front is always 32 columns wide (a step rides when a second column block follows), so nc = 1 and
nc = 31 come from two fronts in one step: diag(A, B) with B = 600 x 97 riding in steps 0 and 1 and A = 300 x 65 / 300 x 95, whose
panel 1 is followed by 1 / 31 columns.  A has two slabs where the launch has three (maxsl above the front's own).

PanelDesc::t_deferred: under the default knobs every panel of a riding step comes from the column pipeline or the wave panel,
which leave T to the update whenever the panel has a live reflector (t_deferred = 1); t_deferred = 0 with reflectors reaches
dev_k_upd_b0 only from the one-workgroup panel (dev_panel), which the default planner takes for no panel of a large front.
options.tall_min_rows = 1 << 30 sends every panel there: two cases run so, the T slot read instead of built.

The head of the role (its descriptors in one load per structure) runs in every case; its ordered sums take one batch up to four
slabs (eight without G), so two taller fronts (1400 and 2400 rows) give them a second, partly padded batch."""
import importlib

import numpy as np
import pytest

from block0_cases import (B0_TIMELINE, DEAD_AT, analyzed, assert_oracle, assert_same_bits, block0_count, factorize, make_front,
                          riding_block0)

pytestmark = pytest.mark.gpu
M, FN = 600, 97


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("stm-multifrontal-qr-factorization-empowered-by-gcn_amd")
    assert p.device_count() >= 1
    return p


def check(pkg, oracle, monkeypatch, capfd, fronts, tol=-1.0, **options):
    """lookahead = 2 against lookahead = 0 bit for bit, the count of block-0 workgroup sets, then the oracle.  Returns the factors."""
    sym, S, Ap, Ai, Ax = analyzed(pkg, fronts)
    n = int(sym["n"])
    st0, A = factorize(pkg, sym, Ap, Ai, Ax, tol, n, lookahead=0, **options)
    capfd.readouterr()
    monkeypatch.setenv("STMMQR_DBG", str(B0_TIMELINE))
    try:
        st2, B = factorize(pkg, sym, Ap, Ai, Ax, tol, n, lookahead=2, **options)
    finally:
        monkeypatch.delenv("STMMQR_DBG")
    ran = block0_count(capfd.readouterr().err)
    want = riding_block0([F.shape for F, _ in fronts])
    print(f"block-0 workgroup sets: {ran} (expected {len(want)}: {want})")
    assert want and ran == len(want)
    assert st0["retries"] == 0 and st2["retries"] == 0 and st0["reschedules"] == 0 and st2["reschedules"] == 0
    assert_same_bits(A, B)                                      # the serial kernels: the same bits
    assert_oracle(oracle, S, Ap, Ai, Ax, tol, n, st2, B)         # the CPU oracle (test_gpu_column_step.py::check_against_oracle)
    return B


@pytest.mark.parametrize("mp", [33, 64, 65, 128, 129, 192, 193, 256, 257, 320, 513])
def test_rows_below_the_diagonal_block(pkg, oracle, monkeypatch, capfd, mp):
    """panel 0 with mp rows, panel 1 with 568; block 0 is 32 columns wide in both"""
    B = check(pkg, oracle, monkeypatch, capfd, [make_front(M, FN, mp, seed=mp)])
    assert B.rank == FN


@pytest.mark.parametrize("kind", ["steps", "boundary"])
def test_staircase_ends_inside_a_chunk_and_on_its_boundary(pkg, oracle, monkeypatch, capfd, kind):
    B = check(pkg, oracle, monkeypatch, capfd, [make_front(M, FN, 0, kind, seed=5)])
    assert B.rank == FN


@pytest.mark.parametrize("mp", [129, 320])
def test_dead_reflectors(pkg, oracle, monkeypatch, capfd, mp):
    """three dead columns in panel 0: no reflector at their place (pdiag = STM_BIGROW), the rows of the panels behind shift"""
    B = check(pkg, oracle, monkeypatch, capfd, [make_front(M, FN, mp, seed=mp, dead=True)], tol=1e-9)
    assert B.rank == FN - len(DEAD_AT)
    assert all(B.Rdead[k] == 1 for k in DEAD_AT) and int(np.count_nonzero(B.Rdead[:FN])) == len(DEAD_AT)


@pytest.mark.parametrize("fn_a,nc", [(65, 1), (95, 31)])
def test_two_fronts_in_one_step(pkg, oracle, monkeypatch, capfd, fn_a, nc):
    """diag(A, B): step 1 rides for B's sake and A's block 0 there is nc columns wide; A has two slabs, the launch three"""
    fronts = [make_front(300, fn_a, 193, seed=fn_a), make_front(M, FN, 257, seed=fn_a + 1)]
    assert (0, 1, nc) in riding_block0([F.shape for F, _ in fronts])
    B = check(pkg, oracle, monkeypatch, capfd, fronts)
    assert B.rank == fn_a + FN


@pytest.mark.parametrize("m,mp,options", [(1400, 1100, {}), (2400, 2100, {"tall_min_rows": 1 << 30})])
def test_more_slabs_than_one_batch_of_the_ordered_sums(pkg, oracle, monkeypatch, capfd, m, mp, options):
    """A thread adds its entries of W1 and G over the slabs in batches (stm_ordered_sums: four slabs per batch with G, eight
    without): 5 and 6 slabs with a deferred T, 9 and 10 with T read from its slot -- a second batch with padded terms"""
    B = check(pkg, oracle, monkeypatch, capfd, [make_front(m, FN, mp, seed=m)], **options)
    assert B.rank == FN


@pytest.mark.parametrize("mp", [65, 257])
def test_t_read_from_its_slot(pkg, oracle, monkeypatch, capfd, mp):
    """t_deferred = 0 (not a default path: tall_min_rows = 1 << 30, every panel by the one-workgroup panel kernel, which builds T)"""
    B = check(pkg, oracle, monkeypatch, capfd, [make_front(M, FN, mp, seed=mp)], tall_min_rows=1 << 30)
    assert B.rank == FN
