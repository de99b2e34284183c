"""numpy model of the energy draw's bucket records (csrc/sart_tables.hip: energy_records_kernel; csrc/sart_kernels.hip: the WORD form of
energy_draw_begin / energy_draw_finish), shared by the CPU and the GPU tests.

One 16-byte record per (row, guide bucket).  With T[i] = floor(cdf[i] 2^32) saturated (cdf_hi32) and a bucket whose words are
first .. last, bracketed by the guide entries g[k], g[k + 1]:
  lo      g[k] + #{i in [g[k], g[k + 1]): T[i] < first}  (entries below every word of the bucket; none in a uniform bucket)
  t[s]    s < K: T[lo + s] - off - block for lo + s < g[k + 1] and T[lo + s] <= last, else EMPTY; off = 0 in the uniform buckets and
          1 in the log buckets, block = (first - off) with its low 22 bits cleared
  mark    lo + K < g[k + 1]
and the draw of a word z of the bucket is lo + #{s: t[s] < ((z - off) & EMPTY)}; only a marked record whose last threshold lies
below the word goes on from lo + K with the two-level draw (candidates of cdf_hi32, then the search in the f64 row)."""
import numpy as np

DIV = 1024                       # kEnergyGuideDiv
UNIFORM = DIV // 32 * 31         # kEnergyGuideUniform
LOG_MAX = 25 * 64                # kEnergyGuideLogMax
BUCKETS = UNIFORM + LOG_MAX + 1  # kEnergyGuideBuckets
CODE0 = (1023 - 5) << 6          # kEnergyGuideCode0
SPLIT = 0xF8000000               # 31/32 of 2^32
K = 5                            # thresholds per record
EMPTY = 0x3FFFFF
BLOCK_BITS = 22
LO_MAX = 2047                    # 11 bits
TWO32 = 4294967296.0


def hi32(cdf):
    t = np.floor(np.asarray(cdf, dtype=np.float64) * TWO32)
    return np.minimum(t, 4294967295.0).astype(np.int64)


def _log_j(z):
    """Log bucket j of the words z >= SPLIT, as energy_draw_begin reads it off the bits of the double v = 1 - z / 2^32."""
    v = 1.0 - np.asarray(z, dtype=np.float64) / TWO32                      # exact
    code = (v.view(np.uint64) >> np.uint64(32 + 14)).astype(np.int64)
    return np.minimum(CODE0 - code, LOG_MAX)


def bucket_of_word(z):
    z = np.asarray(z, dtype=np.int64)
    out = z >> BLOCK_BITS
    top = z >= SPLIT
    if top.any():
        out = out.copy()
        out[top] = UNIFORM + _log_j(z[top])
    return out


def bucket_word_ranges():
    """(first, last) word of every bucket; first > last for a log bucket that no word falls into.  The log part by bisection over
    the words with bucket_of_word itself (it is monotone in the word), not from a formula."""
    first = np.zeros(BUCKETS, dtype=np.int64)
    last = np.zeros(BUCKETS, dtype=np.int64)
    k = np.arange(UNIFORM, dtype=np.int64)
    first[:UNIFORM] = k << BLOCK_BITS
    last[:UNIFORM] = ((k + 1) << BLOCK_BITS) - 1
    # smallest word z >= SPLIT with j(z) >= j, for j = 0 .. LOG_MAX + 1 (2^32 where there is none)
    j = np.arange(LOG_MAX + 2, dtype=np.int64)
    lo = np.full(j.size, SPLIT, dtype=np.int64)
    hi = np.full(j.size, 1 << 32, dtype=np.int64)
    while (lo < hi).any():
        mid = (lo + hi) >> 1
        ge = _log_j(np.minimum(mid, (1 << 32) - 1)) >= j
        ge &= mid < (1 << 32)
        hi = np.where((lo < hi) & ge, mid, hi)
        lo = np.where((lo < hi) & ~ge, mid + 1, lo)
    first[UNIFORM:] = lo[:-1]
    last[UNIFORM:] = lo[1:] - 1
    return first, last


def guide_of(row):
    """The guide entries of one row (sart_set_solar_tables / energy_guide_kernel)."""
    row = np.asarray(row, dtype=np.float64)
    n = row.size
    g = np.empty(BUCKETS + 1, dtype=np.int64)
    g[:UNIFORM + 1] = np.searchsorted(row, np.arange(UNIFORM + 1) / float(DIV), "left")
    j = np.arange(1, LOG_MAX + 1, dtype=np.int64)
    dec = ((CODE0 - j + 1).astype(np.uint64) << np.uint64(14 + 32)).view(np.float64)
    g[UNIFORM + 1:BUCKETS] = np.searchsorted(row, 1.0 - dec, "right")
    g[BUCKETS] = n - 1
    return np.minimum(g, n - 1)


def build_records(row, first, last, k_thr=K):
    """(lo, t[BUCKETS][k_thr], mark, packed uint32[BUCKETS][4] for k_thr == 5) of one row."""
    t_row = hi32(row)
    g = guide_of(row)
    glo, ghi = g[:-1], g[1:]
    off = (np.arange(BUCKETS) >= UNIFORM).astype(np.int64)
    block = ((first - off) >> BLOCK_BITS) << BLOCK_BITS
    lo = np.clip(np.searchsorted(t_row, first, "left"), glo, np.maximum(glo, ghi))
    tp = np.concatenate([t_row, np.full(k_thr + 1, 1 << 40, dtype=np.int64)])
    idx = lo[:, None] + np.arange(k_thr)[None, :]
    tv = tp[np.minimum(idx, tp.size - 1)]
    inside = (idx < ghi[:, None]) & (tv <= last[:, None])
    thr = np.where(inside, tv - off[:, None] - block[:, None], EMPTY)
    assert ((thr >= 0) & (thr <= EMPTY)).all()
    mark = (lo + k_thr < ghi).astype(np.int64)
    packed = None
    if k_thr == 5:
        t4 = thr[:, 4]
        packed = np.stack([thr[:, 0] << 10 | (lo & 0x3FF), thr[:, 1] << 10 | ((lo >> 10) << 8) | (t4 >> 14),
                           thr[:, 2] << 10 | ((t4 >> 6) & 0xFF), thr[:, 3] << 10 | (mark << 8) | ((t4 & 0x3F) << 2)], axis=1).astype(np.uint32)
    return lo, thr, mark, packed


def draw(row, packed, z):
    """The record draw of the words z in one row, in the kernel's 32-bit arithmetic on the packed records; (index, fell back)."""
    z = np.asarray(z, dtype=np.int64)
    n = len(row)
    t_row = hi32(row)
    g = guide_of(row)
    k = bucket_of_word(z)
    off = (z >= SPLIT).astype(np.int64)
    w = packed[k].astype(np.int64)
    m32 = 0xFFFFFFFF
    xs = ((z - off) << 10) & m32
    cnt = sum((w[:, s] < xs).astype(np.int64) for s in range(4))
    t4s = ((w[:, 1] & 0xFF) << 24) | ((w[:, 2] & 0xFF) << 16) | ((w[:, 3] & 0xFF) << 8)   # the low bytes of words 1 - 3, then a zero byte
    b4 = t4s < xs
    lo = (w[:, 0] & 0x3FF) | ((w[:, 1] & 0x100) << 2)
    out = lo + cnt + b4
    rare = b4 & ((w[:, 3] & 0x100) != 0)
    for i in np.nonzero(rare)[0]:                       # the two-level draw from lo + K on
        a, hi = int(lo[i]) + K, int(g[k[i] + 1])
        c = t_row[a:a + 4]
        a2 = a + int((c < z[i]).sum())
        if c.size == 4 and c[3] < z[i] and hi > a + 4:
            a2 = a2 + int(np.searchsorted(row[a2:hi], z[i] / TWO32, "left"))
        out[i] = a2
    return np.minimum(out, n - 1), rare
