"""What tests/test_gpu_adversarial.py relies on, checked with the references alone (no GPU): on the fronts of
tests/adversarial_fronts.py every rank decision is far enough from tol that rounding cannot turn it, the fp64 restatement
of the reference's front (oracle) and the long-double loop agree on every integer output, the backward quantities of the
oracle's own factors are at rounding level, and the fronts discriminate: the numpy model of the Gram-based panel
(tests/ca_model.py) reproduces the decisions with its refresh rule and gets them wrong without it."""
import numpy as np
import pytest

import ca_model
from adversarial_fronts import TOL, backward_metrics, crafted_columns, make_adversarial, ref_front

CASES96 = [(m, 96, kind, 96, 96) for m in (186, 1300, 4500, 8300) for kind in ("full", "ramp", "steps")] + \
          [(1300, 96, "full", 96, 90), (1300, 96, "full", 64, 64)]
CASES160 = [(m, 160, "full", 160, 160) for m in (700, 2600, 4500)]


@pytest.mark.parametrize("m,n,kind,npiv,ntol", CASES96 + CASES160)
def test_margin_agreement_and_backward_error_of_the_reference(oracle, m, n, kind, npiv, ntol):
    F0, St0, crafted = make_adversarial(m, n, kind)
    assert F0.flags.f_contiguous
    rank, St, Rdead, absb = ref_front(F0, St0, npiv, TOL, ntol)
    # every decision is at least 3x away from tol: no rounding of a correct fp64 factorization (cond(R) ~ 1e9, so a
    # pivot of size 1e-10 carries an error around 1e-16 * ||F||, 1e-6 of itself) can turn it
    ratio = np.array(absb[:min(ntol, npiv)], float) / TOL
    print(f"{m}x{n} {kind} npiv={npiv} ntol={ntol}: |beta|/tol closest to 1: "
          f"{min(max(r, 1 / r) for r in ratio):.2f}, rank {rank}")
    assert np.all((ratio < 1 / 3) | (ratio > 3)), ratio
    # the decisions are the crafted ones: delta = tol / 8 dies where a column can die, everything else lives
    want_dead = [k for k, (delta, _) in crafted.items() if delta < TOL and k < min(ntol, npiv)]
    assert np.flatnonzero(Rdead).tolist() == want_dead
    assert rank == npiv - len(want_dead)
    # the fp64 restatement of the reference agrees on every integer
    Fo, So = F0.copy(order="F"), St0.copy()
    ro, To, Do, _ = oracle.front(Fo, So, npiv, TOL, ntol)
    assert ro == rank
    np.testing.assert_array_equal(So, St)
    np.testing.assert_array_equal(Do, Rdead)
    # ... and its factors reproduce the front to rounding; what it dropped is below tol
    e_live, e_dead, orth = backward_metrics(F0, Fo, So, To, Do, npiv)
    print(f"  oracle: e_live {e_live:.2e} e_dead {e_dead:.2e} orth {orth:.2e}")
    assert e_live <= 1e-13 and orth <= 1e-13
    assert e_dead <= TOL


def test_crafted_columns_sit_on_the_edges():
    """last / first column of a 32-column panel and of an 8-column sub-panel, one whole sub-panel, the last pivot"""
    c96, c160 = crafted_columns(96), crafted_columns(160)
    dead = [k for k, (d, _) in c160.items() if d < TOL]
    assert {31, 95, 127, 159} <= set(dead) and {8, 64} <= set(dead) and set(range(40, 48)) <= set(dead)
    assert max(c96) == 95 and max(c160) == 159 and len([k for k, (d, _) in c96.items() if d < TOL]) == 13


def test_reference_is_cached_and_leaves_its_input_alone():
    F0, St0, _ = make_adversarial(186, 96, "steps")
    Fc, Sc = F0.copy(), St0.copy()
    a = ref_front(F0, St0, 96, TOL, 96)
    b = ref_front(F0.copy(order="F"), St0.copy(), 96, TOL, 96)
    assert a is b
    np.testing.assert_array_equal(F0, Fc)
    np.testing.assert_array_equal(St0, Sc)
    assert not a[1].flags.writeable
    G0, Sg, _ = make_adversarial(186, 96, "steps", craft=False)
    keep = [k for k in range(96) if k not in crafted_columns(96)]
    np.testing.assert_array_equal(G0[:, keep], F0[:, keep])
    rank, St, Rdead, _ = ref_front(G0, Sg, 96, TOL, 96)
    assert rank == 96 and not Rdead.any()


@pytest.mark.parametrize("m", [186, 1300])
@pytest.mark.parametrize("kind", ["full", "ramp", "steps"])
def test_fronts_discriminate_the_gram_refresh(m, kind):
    """The Gram-based panel takes its column norms from a downdated Gram matrix: with the refresh rule (K = 32) the
    model decides every column like the reference, without it (K = 1e300) it does not."""
    F0, St0, _ = make_adversarial(m, 96, kind)
    rank, St, Rdead, _ = ref_front(F0, St0, 96, TOL, 96)
    Fm, Sm = F0.copy(order="F"), St0.copy()
    rk, _, Rd = ca_model.front_qr(Fm, Sm, 96, TOL, 96, "ca", 32.0)
    assert rk == rank
    np.testing.assert_array_equal(Sm, St)
    np.testing.assert_array_equal(Rd[:96], Rdead)
    Fm, Sm = F0.copy(order="F"), St0.copy()
    with np.errstate(all="ignore"):
        rk, _, Rd = ca_model.front_qr(Fm, Sm, 96, TOL, 96, "ca", 1e300)
    wrong = int(np.count_nonzero(Rd[:96] != Rdead))
    print(f"{m} {kind}: Gram model without refresh decides {wrong} columns differently")
    assert wrong >= 1
