"""The rule behind the word-exact CDF draws of the accumulating kernels, as a numpy model: for a uniform that is a 32-bit word
over 2^32, counting the table entries floor(cdf 2^32) (saturated) below the word IS lowerBound(cdf, u), and the guide bucket and
the uniform / log split of the energy draw are a shift and a compare of the word."""
import numpy as np

from tests.word_draw_cases import TWO32, hi32, lower_bound, make_rows, words_for

ROWS = make_rows()


def test_count_of_saturated_words_below_z_is_the_lower_bound():
    n_cases = 0
    for row in ROWS:
        z = words_for(row)
        t = hi32(row)
        count = (t[None, :] < z[:, None]).sum(axis=1)
        want = lower_bound(row, z)
        assert (count == want).all(), (z[count != want][:5], count[count != want][:5], want[count != want][:5])
        n_cases += z.size
    assert n_cases >= 1000


def test_saturated_entries_are_never_below_a_word():
    row = np.array([0.5, 1.0 - 2.0**-31, 1.0 - 2.0**-32, 1.0 - 2.0**-33, 1.0 - 2.0**-53, 1.0])
    t = hi32(row)
    assert t.tolist() == [0x80000000, 0xFFFFFFFE, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF]
    z = np.array([0xFFFFFFFE, 0xFFFFFFFF], dtype=np.uint32)
    assert ((t[None, :] < z[:, None]).sum(axis=1) == lower_bound(row, z)).all()


def test_bucket_and_split_of_the_word_equal_the_f64_expressions():
    div = 1024                                              # kEnergyGuideDiv
    z = np.unique(np.concatenate([words_for(r) for r in ROWS] + [np.arange(0, 2**32, 2**22 - 3, dtype=np.uint64).astype(np.uint32)]))
    u = z.astype(np.float64) / TWO32
    assert ((u * div).astype(np.int64) == (z >> np.uint32(22))).all()          # (int)(u5 * Div)
    assert (((1.0 - u) > 0.03125) == (z < np.uint32(0xF8000000))).all()        # v > 1/32
    # the radius draw's buckets are already taken from the word (floor(u2 2^32) >> 21, >> 17): the same floor as the product
    assert ((u * 2048).astype(np.int64) == (z >> np.uint32(21))).all()
