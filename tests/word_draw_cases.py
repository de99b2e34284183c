"""Shared inputs of the word-draw tests (CPU model and GPU entry): CDF rows with the entries that can trip a 32-bit compare, and
the random words at which a draw's answer can change.  numpy's searchsorted(row, z / 2^32, 'left') on the f64 row is the reference
(lowerBound: z / 2^32 is exact in f64 for every 32-bit z)."""
import numpy as np

TWO32 = 4294967296.0


def hi32(cdf):
    """floor(cdf 2^32), saturated at 0xFFFFFFFF (cdf_hi32_kernel / stage_tables); exact: cdf <= 1 has at most 53 significant bits."""
    t = np.floor(np.asarray(cdf, dtype=np.float64) * TWO32)
    return np.minimum(t, 4294967295.0).astype(np.uint64).astype(np.uint32)


def make_rows(n_rows=4, n=64, seed=11):
    """Sorted rows of n entries in (0, 1], last entry 1.0: exact multiples of 2^-32, entries a hair (2^-40 .. 2^-52) off such a
    multiple on either side, duplicates, runs of more than four entries inside one guide bucket, entries within 2^-40 of 1."""
    rng = np.random.default_rng(seed)
    rows = []
    for r in range(n_rows):
        words = np.sort(rng.integers(1, 2**32 - 1, size=n, dtype=np.uint64))
        row = words.astype(np.float64) / TWO32                       # exact multiples of 2^-32
        off = rng.choice([0.0, 2.0**-40, -2.0**-40, 2.0**-52, -2.0**-52, 2.0**-33], size=n)
        row = np.clip(row + off, 2.0**-60, 1.0)
        row[5] = row[4]                                              # duplicates
        row[9] = row[10] = row[11] = row[8]
        # a bucket wider than four entries: ten entries inside one 2^-10 bucket of the uniform (and one 2^-11 radius bucket)
        base = (100 + 37 * r) / 1024.0
        row[20:30] = base + np.arange(1, 11) * 2.0**-16 + rng.choice([0.0, 2.0**-45], size=10)
        # the top of the table: beyond 31/32 (the log buckets), within 2^-40 of 1, at and beyond 1 - 2^-32, 1.0 itself
        row[-8:] = [0.97, 0.99, 1.0 - 2.0**-20, 1.0 - 2.0**-31, 1.0 - 2.0**-32, 1.0 - 2.0**-40, 1.0 - 2.0**-53, 1.0]
        rows.append(np.sort(row))
    rows = np.array(rows)
    assert (np.diff(rows, axis=1) >= 0).all() and (rows[:, -1] == 1.0).all() and (rows > 0).all()
    return rows


def words_for(row):
    """Every entry's word and its two neighbours, 0, 2^32 - 1, the uniform / log split 0xF8000000 +- 1, bucket edges k << 22."""
    w = hi32(row).astype(np.int64)
    z = np.concatenate([w - 1, w, w + 1, [0, 1, 2**32 - 1, 2**32 - 2, 0xF8000000 - 1, 0xF8000000, 0xF8000000 + 1],
                        (np.arange(0, 1024, 17, dtype=np.int64) << 22), (np.arange(1, 1024, 29, dtype=np.int64) << 22) - 1])
    return np.unique(np.clip(z, 0, 2**32 - 1)).astype(np.uint32)


def lower_bound(row, z):
    return np.searchsorted(row, z.astype(np.float64) / TWO32, side="left")
