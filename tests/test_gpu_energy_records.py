"""The bucket records of the energy draw on the GPU, through the internal entry sart_internal_record_draw: the record draw, the
two-level word draw and the general draw all give numpy's lowerBound of the f64 row, and the device's record table is the numpy
model's (tests/energy_records_model.py), word for word."""
import ctypes as C

import numpy as np
import pytest

from solaraxionraytracing_amd import _lib as L
from tests import energy_records_model as M
from tests.word_draw_cases import lower_bound, make_rows, words_for

pytestmark = pytest.mark.gpu

FIRST, LAST = M.bucket_word_ranges()


def _draw(cdf, rows, words, use_records, want_table=False):
    fn = L.load_sart().sart_internal_record_draw
    fn.restype = C.c_int
    cdf = np.ascontiguousarray(cdf, dtype=np.float64)
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    words = np.ascontiguousarray(words, dtype=np.uint32)
    out_w = np.full(words.size, -1, dtype=np.int32)
    out_g = np.full(words.size, -1, dtype=np.int32)
    used = C.c_int(-1)
    table = np.zeros((cdf.shape[0], M.BUCKETS, 4), dtype=np.uint32) if want_table else None
    rc = fn(cdf.ctypes.data_as(C.POINTER(C.c_double)), C.c_int(cdf.shape[0]), C.c_int(cdf.shape[1]),
            rows.ctypes.data_as(C.POINTER(C.c_int32)), words.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_int(words.size),
            C.c_int(int(use_records)), out_w.ctypes.data_as(C.POINTER(C.c_int32)), out_g.ctypes.data_as(C.POINTER(C.c_int32)),
            C.byref(used), table.ctypes.data_as(C.POINTER(C.c_uint32)) if want_table else None)
    assert rc == 0
    return out_w, out_g, used.value, table


def _edge_words():
    """Every bucket's first and last word and their neighbours (the uniform edges +- 1, 0xF8000000 +- 1, every log-bucket edge - the top
    three octaves among them), 0 and 2^32 - 1."""
    ok = FIRST <= LAST
    z = np.concatenate([FIRST[ok] - 1, FIRST[ok], FIRST[ok] + 1, LAST[ok] - 1, LAST[ok], LAST[ok] + 1, [0, 2**32 - 1, M.SPLIT - 1, M.SPLIT, M.SPLIT + 1]])
    return np.unique(np.clip(z, 0, 2**32 - 1)).astype(np.uint32)


def _cases(cdf):
    rows, words, want = [], [], []
    edges = _edge_words()
    for r, row in enumerate(cdf):
        z = np.unique(np.concatenate([words_for(row), edges]))
        rows.append(np.full(z.size, r))
        words.append(z)
        want.append(np.minimum(lower_bound(row, z), cdf.shape[1] - 1))
    return np.concatenate(rows), np.concatenate(words), np.concatenate(want)


def _special_rows(n=64):
    """Rows of n entries: exactly K and K + 1 entries in one bucket, a ten-entry run in one bucket, duplicates at a threshold (in a
    uniform and in a log bucket), everything beyond 31/32."""
    rng = np.random.default_rng(3)
    rows = []
    for kind in range(5):
        row = np.sort(rng.random(n))
        if kind in (0, 1):
            row = row[(row < 300 / 1024.0) | (row >= 301 / 1024.0)]
            row = np.concatenate([row[:n - (M.K + kind) - 1], 300 / 1024.0 + np.arange(1, M.K + kind + 1) * 2.0**-14])
        elif kind == 2:
            row[10:20] = 517 / 1024.0 + np.arange(1, 11) * 2.0**-15
        elif kind == 3:
            row[8:12] = row[8]                                   # four equal entries: thresholds 0 .. 3 of their bucket
            row[30:36] = 0.99 + 2.0**-21                         # six equal entries in a log bucket: the fifth threshold and the mark
        else:
            row = 31 / 32.0 + row / 32.0
            row[:3] = [31 / 32.0, 31 / 32.0, 31 / 32.0 + 2.0**-32]
        row = np.sort(np.concatenate([row[:n - 1], [1.0]]))
        assert row.size == n
        rows.append(row)
    return np.array(rows)


@pytest.mark.parametrize("table", ["word_draw_cases", "special_rows"])
def test_record_draw_two_level_draw_and_lower_bound_agree(table):
    cdf = make_rows(4, 64) if table == "word_draw_cases" else _special_rows()
    rows, words, want = _cases(cdf)
    rec_w, rec_g, used, dev_table = _draw(cdf, rows, words, True, want_table=True)
    two_w, two_g, used0, _ = _draw(cdf, rows, words, False)
    assert used == 1 and used0 == 0
    for name, got in (("records", rec_w), ("two-level", two_w), ("general", rec_g), ("general, records off", two_g)):
        bad = got != want
        assert not bad.any(), (name, words[bad][:8], got[bad][:8], want[bad][:8])
    # the device's table is the model's, wherever a word can read it; the model's draw on it takes the fall-back for some words
    ok = FIRST <= LAST
    n_rare = 0
    for r, row in enumerate(cdf):
        _, _, mark, packed = M.build_records(row, FIRST, LAST)
        assert (dev_table[r][ok] == packed[ok]).all(), (r, np.nonzero((dev_table[r] != packed).any(axis=1) & ok)[0][:8])
        n_rare += int(M.draw(row, packed, words[rows == r])[1].sum())
    assert n_rare > 0


def test_exactly_k_and_k_plus_one_entries_in_a_bucket():
    cdf = _special_rows()
    for r, more in ((0, 0), (1, 1)):
        lo, thr, mark, _ = M.build_records(cdf[r], FIRST, LAST)
        assert (thr[300] != M.EMPTY).all() and mark[300] == more


def test_a_table_of_2100_energies_draws_without_records():
    rng = np.random.default_rng(8)
    row = np.sort(rng.random(2100))
    row[-1] = 1.0
    cdf = row[None, :]
    rows, words, want = _cases(cdf)
    got_w, got_g, used, _ = _draw(cdf, rows, words, True)
    assert used == 0
    assert (got_w == want).all() and (got_g == want).all()
    assert want.max() > M.LO_MAX          # indices a record could not hold
