"""wave_reduce8<NV> (csrc/stmmqr_wave.h) as a numpy model: the halving butterfly with its exchanges as index permutations
(row_half_mirror, quad_perm [1,0,3,2] and [2,3,0,1], row_ror:8, the two row swaps), sized against unsized.

NV says that v[NV..7] are structurally zero.  A pair whose upper member is zero becomes `n = v + moved(v)` in every lane, a
pair with both members zero does not exist.  The contract: lane l with red8_idx(l) < NV ends with the same BYTES as the
unsized form; the other lanes hold anything.  IEEE double addition in numpy is the addition of v_add_f64 (round to nearest
even, no flush of denormals in the panel kernels), so equal association gives equal bytes here as on the device."""
import numpy as np
import pytest

LANES = np.arange(64)
HALF_MIRROR = (LANES & ~7) | (7 - (LANES & 7))      # DPP 0x141: lane l reads lane 7 - (l & 7) of its half row
XOR1, XOR2 = LANES ^ 1, LANES ^ 2                   # DPP 0xB1 / 0x4E
ROR8, XOR16, XOR32 = LANES ^ 8, LANES ^ 16, LANES ^ 32   # row_ror:8 in a row of 16, v_permlane16_swap, v_permlane32_swap
S_A, S_B, S_C = ((LANES >> 2) & 1).astype(bool), (LANES & 1).astype(bool), ((LANES >> 1) & 1).astype(bool)
RED8_IDX = ((LANES >> 1) & 1) + 2 * (LANES & 1) + 4 * ((LANES >> 2) & 1)
FULL_PAIR, PLAIN_PAIR = 7, 3                        # instructions: 4 selects + 2 DPP moves + 1 add / 2 DPP moves + 1 add


def _pair(lo, hi, side, perm):
    """One exchange-add of the butterfly: (value, instructions) or None where the pair does not exist."""
    if lo is None:
        assert hi is None                           # live values are a prefix: an upper member never outlives its lower one
        return None
    if hi is None:
        return lo + lo[perm], PLAIN_PAIR
    keep, send = np.where(side, hi, lo), np.where(side, lo, hi)
    return keep + send[perm], FULL_PAIR


def reduce8(v, nv=8):
    """v: (8, 64) doubles, one row per value.  Returns (the 64 lanes of wave_reduce8<nv>, instructions of the butterfly)."""
    cur, count = [v[i] if i < nv else None for i in range(8)], 0
    for side, perm in ((S_A, HALF_MIRROR), (S_B, XOR1), (S_C, XOR2)):
        half = len(cur) // 2
        nxt = []
        for i in range(half):
            p = _pair(cur[i], cur[i + half], side, perm)
            nxt.append(None if p is None else p[0])
            count += 0 if p is None else p[1]
        cur = nxt
    r = cur[0]
    for perm in (ROR8, XOR16, XOR32):               # wave_sum_stride8: unchanged by NV
        r = r + r[perm]
    return r, count


def _vectors(rng, n):
    """n inputs of (8, 64): signs mixed, exponents over 16 decades, so that every association of a sum rounds differently."""
    mag = 10.0 ** rng.uniform(-8.0, 8.0, size=(n, 8, 64))
    return mag * rng.choice([-1.0, 1.0], size=mag.shape) * rng.uniform(0.5, 1.0, size=mag.shape)


def test_unsized_model_sums_every_value():
    v = np.round(_vectors(np.random.default_rng(1), 1)[0] * 1e3 % 1013.0) - 500.0     # integers: every sum exact
    r, count = reduce8(v)
    assert count == 49
    assert np.array_equal(r, v.sum(axis=1)[RED8_IDX])


def test_association_matters_on_this_data():
    """The data must be able to tell two orders of addition apart, or equal bytes would prove nothing."""
    v = _vectors(np.random.default_rng(2), 50)
    differs = 0
    for x in v:
        r, _ = reduce8(x)
        differs += int(np.any(r != x.sum(axis=1)[RED8_IDX]))
    assert differs > 25


@pytest.mark.parametrize("nv", range(1, 9))
def test_sized_equals_unsized_in_specified_lanes(nv):
    rng = np.random.default_rng(100 + nv)
    v = _vectors(rng, 2000)
    v[:, nv:, :] = 0.0
    spec = RED8_IDX < nv
    assert spec.sum() == 8 * nv
    for x in v:
        want, _ = reduce8(x)
        got, _ = reduce8(x, nv)
        assert want[spec].tobytes() == got[spec].tobytes()


def test_unspecified_lanes_never_feed_specified_ones():
    """Poison (NaN) in place of the structural zeros reaches no specified lane of the sized form."""
    rng = np.random.default_rng(7)
    for nv in range(1, 8):
        x = _vectors(rng, 1)[0]
        x[nv:] = 0.0
        want, _ = reduce8(x)
        # the sized form never reads v[nv..7]: poisoning them changes nothing at all
        y = x.copy()
        y[nv:] = np.nan
        got, _ = reduce8(y, nv)
        spec = RED8_IDX < nv
        assert want[spec].tobytes() == got[spec].tobytes()


def test_instructions_per_butterfly():
    want = {8: 49, 7: 45, 6: 41, 5: 37, 4: 33, 3: 26, 2: 19, 1: 9}
    x = np.zeros((8, 64))
    assert {nv: reduce8(x, nv)[1] for nv in range(1, 9)} == want
