"""The bucket records of the energy draw as a numpy model (tests/energy_records_model.py): the record draw is lowerBound for every
(row, word) of the word-draw cases and for rows of 1, 2, 5 and 1500 entries; every bucket's words lie in one aligned block of 2^22
once the log buckets' words are taken one lower; and on the headline tables the records settle all but 1 draw in 300."""
import numpy as np
import pytest

from tests import energy_records_model as M
from tests.word_draw_cases import lower_bound, make_rows, words_for

FIRST, LAST = M.bucket_word_ranges()


def _edge_words():
    ok = FIRST <= LAST
    z = np.concatenate([FIRST[ok] - 1, FIRST[ok], FIRST[ok] + 1, LAST[ok] - 1, LAST[ok], LAST[ok] + 1, [0, 2**32 - 1, M.SPLIT - 1, M.SPLIT, M.SPLIT + 1]])
    return np.unique(np.clip(z, 0, 2**32 - 1)).astype(np.uint32)


def _check_row(row):
    z = np.unique(np.concatenate([words_for(row), _edge_words()]))
    _, _, _, packed = M.build_records(row, FIRST, LAST)
    got, rare = M.draw(row, packed, z)
    want = np.minimum(lower_bound(row, z), len(row) - 1)
    assert (got == want).all(), (z[got != want][:8], got[got != want][:8], want[got != want][:8])
    return z.size, int(rare.sum())


def test_bucket_count_and_sizes_are_the_device_header_s():
    assert M.BUCKETS == 2593 and M.UNIFORM == 992 and M.LO_MAX + 1 == 1 << 11 and 11 + M.K * M.BLOCK_BITS + 1 <= 128


def test_every_bucket_is_an_interval_of_words_with_these_edges():
    """bucket_of_word at both edges of every bucket and one word beyond them: the ranges tile 0 .. 2^32 - 1 without a gap."""
    ok = FIRST <= LAST
    assert ok[:M.UNIFORM + 1].all() and ok[-1] and ok.sum() > M.UNIFORM + 1300
    k = np.nonzero(ok)[0]
    assert (M.bucket_of_word(FIRST[k]) == k).all() and (M.bucket_of_word(LAST[k]) == k).all()
    assert FIRST[k[0]] == 0 and LAST[k[-1]] == 2**32 - 1 and (FIRST[k[1:]] == LAST[k[:-1]] + 1).all()
    assert FIRST[M.UNIFORM] == LAST[M.UNIFORM] == M.SPLIT          # j = 0: the single point u = 31/32


def test_block_property_at_every_bucket_edge():
    """Uniform buckets ARE aligned blocks of 2^22 words.  A log bucket is the words 2^32 - m of an aligned block of m: in the words
    themselves it starts one past an aligned address, so its LAST word may open the next block of 2^22 - the words less one never do.
    The draw therefore compares (word - 1) in the log part."""
    k = np.arange(M.BUCKETS)
    ok = FIRST <= LAST
    uni = k < M.UNIFORM
    assert ((FIRST[uni] & M.EMPTY) == 0).all() and ((LAST[uni] & M.EMPTY) == M.EMPTY).all()
    lg = ok & ~uni
    width = LAST[lg] - FIRST[lg] + 1
    assert width.max() == 1 << 20 and (width & (width - 1)).tolist().count(0) >= width.size - 1   # powers of two (the last bucket: m = 1 .. 4)
    assert (((FIRST[lg] - 1) >> M.BLOCK_BITS) == ((LAST[lg] - 1) >> M.BLOCK_BITS)).all()
    # ... and the words themselves do cross a block edge in some log bucket: the shift by one is needed
    assert ((FIRST[lg] >> M.BLOCK_BITS) != (LAST[lg] >> M.BLOCK_BITS)).any()
    wide = width > 4
    assert (((FIRST[lg][wide] - 1) & (width[wide] - 1)) == 0).all()    # aligned to its own width, one below its first word


def test_record_draw_is_the_lower_bound_on_the_word_draw_cases():
    n, rare = 0, 0
    for row in make_rows():
        a, b = _check_row(row)
        n, rare = n + a, rare + b
    assert n >= 4 * 5000 and rare > 0        # the ten-entry run of every row takes the fall-back


@pytest.mark.parametrize("n", [1, 2, 5, 1500])
def test_record_draw_on_short_and_long_rows(n):
    rng = np.random.default_rng(n)
    row = np.sort(rng.random(n))
    if n >= 5:
        row[1] = row[2]                                                # a duplicate
    row[-1] = 1.0
    _check_row(row)
    row = np.sort(np.concatenate([rng.random(n - 1) * 2.0**-9 + 0.971, [1.0]]))   # everything in two buckets, some beyond 31/32
    _check_row(row)


def test_bucket_with_exactly_k_and_k_plus_one_entries():
    base = 300 / 1024.0
    for extra in (M.K, M.K + 1):
        row = np.sort(np.concatenate([[0.1, 0.2], base + np.arange(1, extra + 1) * 2.0**-14, [0.5, 1.0]]))
        lo, thr, mark, _ = M.build_records(row, FIRST, LAST)
        assert lo[300] == 2 and mark[300] == (extra > M.K) and (thr[300] != M.EMPTY).all()
        _, rare = _check_row(row)
        assert (rare > 0) == (extra > M.K)


def _fallback_share(k_thr):
    """Share of the headline workload's energy draws that a record of k_thr thresholds does not settle: per row, the words of the
    marked buckets above the record's last threshold, weighted with the radius draw."""
    from solaraxionraytracing_amd import tables as T
    radii, energies = T.solar_grid()
    rcdf, ecdf = T.build_cdfs(T.primakoff_emission_table(), radii, energies)
    p_row = np.diff(np.concatenate([[0.0], rcdf]))
    uni = np.arange(M.BUCKETS) < M.UNIFORM
    share = np.zeros(2)
    for r in np.nonzero(p_row > 0)[0]:
        lo, thr, mark, _ = M.build_records(ecdf[r], FIRST, LAST, k_thr)
        off = (~uni).astype(np.int64)
        block = ((FIRST - off) >> M.BLOCK_BITS) << M.BLOCK_BITS
        t_last = thr[:, k_thr - 1] + off + block                        # the last threshold as a word of the table
        words = np.where((mark == 1) & (thr[:, k_thr - 1] != M.EMPTY), np.maximum(LAST - np.maximum(t_last, FIRST - 1), 0), 0)
        share += p_row[r] * np.array([words[uni].sum(), words[~uni].sum()]) / M.TWO32
    return share


def test_fallback_share_on_the_headline_tables_is_capped():
    uni5, log5 = _fallback_share(M.K)
    print("fall-back share, K = %d: uniform part %.5f, log part %.3e" % (M.K, uni5, log5))
    assert uni5 + log5 <= 1.0 / 300.0, (uni5, log5)
    assert log5 < 1e-6
