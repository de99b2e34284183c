"""The two CDF draws of the ray kernels on the GPU, through the internal entry sart_internal_word_draw: the word-exact form (the
accumulating kernels: uniform = random word / 2^32) and the general form (the record kernel) must both give numpy's lowerBound
of the f64 row, for every (row, word) of tests/word_draw_cases.py."""
import ctypes as C

import numpy as np
import pytest

from solaraxionraytracing_amd import _lib as L
from tests.word_draw_cases import lower_bound, make_rows, words_for

pytestmark = pytest.mark.gpu


def _draw(kind, cdf, rows, words):
    lib = L.load_sart()
    fn = lib.sart_internal_word_draw
    fn.restype = C.c_int
    cdf = np.ascontiguousarray(cdf, dtype=np.float64)
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    words = np.ascontiguousarray(words, dtype=np.uint32)
    out_w = np.full(words.size, -1, dtype=np.int32)
    out_g = np.full(words.size, -1, dtype=np.int32)
    n_rows, n_cols = (cdf.shape if cdf.ndim == 2 else (1, cdf.size))
    rc = fn(C.c_int(kind), cdf.ctypes.data_as(C.POINTER(C.c_double)), C.c_int(n_rows), C.c_int(n_cols),
            rows.ctypes.data_as(C.POINTER(C.c_int32)), words.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_int(words.size),
            out_w.ctypes.data_as(C.POINTER(C.c_int32)), out_g.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == 0
    return out_w, out_g


def test_energy_draw_both_forms_give_the_lower_bound():
    cdf = make_rows(4, 64)
    rows, words, want = [], [], []
    for r, row in enumerate(cdf):
        z = words_for(row)
        rows.append(np.full(z.size, r))
        words.append(z)
        want.append(np.minimum(lower_bound(row, z), 63))       # the draw clamps to the last energy
    rows, words, want = np.concatenate(rows), np.concatenate(words), np.concatenate(want)
    assert words.size >= 1000
    got_w, got_g = _draw(0, cdf, rows, words)
    assert (got_w == want).all(), (words[got_w != want][:8], got_w[got_w != want][:8], want[got_w != want][:8])
    assert (got_g == want).all(), (words[got_g != want][:8], got_g[got_g != want][:8], want[got_g != want][:8])
    # the wide-bucket search was exercised: some answers lie more than four entries above the guide's lower edge
    base = np.array([np.searchsorted(cdf[r], np.floor(z / 2.0**32 * 1024) / 1024, "left") for r, z in zip(rows, words.astype(np.float64))])
    assert ((want - base) > 4).any()


def test_radius_draw_both_forms_give_the_lower_bound():
    row = make_rows(1, 64, seed=5)[0]
    assert (row >= 1.0 - 2.0**-32).sum() >= 3                    # saturated entries in the staged table
    z = np.unique(np.concatenate([words_for(row), np.array([0xFFFFFFFF], dtype=np.uint32)]))
    want = np.minimum(lower_bound(row, z), 63)
    got_w, got_g = _draw(1, row, np.zeros(z.size), z)
    assert (got_w == want).all(), (z[got_w != want][:8], got_w[got_w != want][:8], want[got_w != want][:8])
    assert (got_g == want).all(), (z[got_g != want][:8], got_g[got_g != want][:8], want[got_g != want][:8])
