"""The paired polynomial evaluations of the ray kernels (two chains of one polynomial side by side, one set of scalar constants)
against the single forms, bit for bit, through the math_eval cases 15 - 22 (element i is paired with element i ^ 1, once as the
first and once as the second member of the pair)."""
import ctypes as C

import numpy as np
import pytest

from solaraxionraytracing_amd import _lib as L

pytestmark = pytest.mark.gpu

N = 4096           # pairs
rng = np.random.default_rng(23)


def _eval(fn, x):
    lib = L.load_sart()
    tab = np.empty(2 * 129)
    lib.sart_internal_sincos_table(tab.ctypes.data_as(C.POINTER(C.c_double)))
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(x)
    dp = C.POINTER(C.c_double)
    assert lib.sart_internal_math_eval(fn, x.ctypes.data_as(dp), out.ctypes.data_as(dp), x.size, tab.ctypes.data_as(dp)) == 0
    return out


def _same_bits(a, b):
    return (a.view(np.uint64) == b.view(np.uint64)).all()


def test_paired_asin_has_the_bits_of_asin_small():
    inside = rng.uniform(0.0, 0.06, 2 * N)
    inside[inside == 0.0] = 1e-9                                 # (0, 0.06), both members drawn independently
    # exactly one member of each pair beyond the series' range: its lane takes the library branch, its partner stays on the series
    mixed = rng.uniform(1e-9, 0.06, 2 * N)
    far = rng.uniform(0.06, 1.0, N)
    mixed[0:N:2] = far[0:N:2]                                    # the first member in the first half of the pairs ...
    mixed[N + 1::2] = far[1:N:2][: mixed[N + 1::2].size]         # ... the second member in the other half
    for x in (inside, mixed, -mixed):
        want = _eval(7, x)
        assert _same_bits(_eval(15, x), want) and _same_bits(_eval(16, x), want)
    pairs = np.abs(mixed).reshape(-1, 2) >= 0.06
    assert (pairs.sum(axis=1) == 1).all()


@pytest.mark.parametrize("n, first, second, single", [(16, 17, 18, 21), (6, 19, 20, 22)])
def test_paired_spoke_measure_has_the_bits_of_spoke_measure(n, first, second, single):
    c = rng.uniform(-1.0, 1.0, N)
    c[:4] = [-1.0, 1.0, 0.0, 0.5]
    want = _eval(single, c)
    assert _same_bits(_eval(first, c), want) and _same_bits(_eval(second, c), want)
    # the scaled Chebyshev forms themselves: T16 / 32768 and T6 of c
    t = np.cos(n * np.arccos(c)) / (32768.0 if n == 16 else 1.0)
    assert np.abs(want - t).max() < (1e-15 if n == 16 else 1e-13)
