"""Pins tests/fixed64_model.py - the plain-integer reference the FIXED64 back end is held to in test_gpu_fixed64_backend.py - on the
CPU: values worked by hand for every rule of include/sart.h "accumulation mode", the builders against the model's own checks, a
second, naive computation (everything as one Fraction, no limbs) and single-slot planted errors."""
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import fixed64_model as M

Q = dict(weight=2.0 ** -30, weight_sq=2.0 ** -70, position=2.0 ** -32, reflect=2.0 ** -40)
T40 = 1 << 40


def test_the_model_needs_no_gpu():
    import sys
    src = open(M.__file__).read()
    assert "import torch" not in src and "solaraxionraytracing_amd" not in src
    assert "tests.fixed64_model" in sys.modules


# ---- by hand ------------------------------------------------------------------------------------------------------------------------
def hand_accumulator():
    """2 x 1 image, spectra with 2 radial bins and 3 energy bins: 2 + 24 + 4 + 9 = 39 slots."""
    sh = M.Shape(2, 1, n_radial=2, n_e1=3)
    a = np.zeros(sh.total, dtype=np.int64)
    a[0], a[1] = 5, T40 + 7                            # pixels: 2^40 + 12
    s = sh.s0
    # SUM_WEIGHTS = 3 * 2^40 + 20 = pixels + outside, outside = 2 * 2^40 + 8
    a[s + 0], a[s + 12] = 20, 3
    a[s + 17], a[s + 18] = 8, 2
    a[s + 1] = 300                                     # N_PASSED: 3 * 2^40 + 20 >= 4096 * 300
    a[s + 7], a[s + 16] = 64 * 300, 0                  # squares exactly at 64 per ray
    a[s + 4], a[s + 13] = 3, 1                         # SUM_X = 2^40 + 3
    a[s + 8] = 1000
    a[sh.rc0:sh.rw0] = [100, 200]
    a[sh.rw0:sh.ec0] = [T40 + 20, 2 * T40]
    a[sh.ec0:sh.ew0] = [1, 2, 297]
    a[sh.ew0:sh.er0] = [20, 3 * T40, 0]
    a[sh.er0:sh.total] = [1 << 40, 3, 0]
    return sh, a


def test_accumulator_by_hand():
    sh, a = hand_accumulator()
    assert sh.total == 39
    out, st = M.finalize_accumulator(a, None, sh, Q)
    assert st == 0
    s = sh.s0
    assert out[0] == 5 * 2.0 ** -30 and out[1] == (T40 + 7) * 2.0 ** -30
    assert out[s + 0] == (3 * T40 + 20) * 2.0 ** -30
    assert out[s + 1] == 300.0 and out[s + 8] == 1000.0
    assert out[s + 4] == (T40 + 3) * 2.0 ** -32
    assert out[s + 7] == 64 * 300 * 2.0 ** -70
    for k in (12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23):
        assert out[s + k] == 0.0                       # the *_HI slots, OUTSIDE and the reserved slots read 0
    assert list(out[sh.rc0:sh.rw0]) == [100.0, 200.0]
    assert list(out[sh.rw0:sh.ec0]) == [(T40 + 20) * 2.0 ** -30, 2 * T40 * 2.0 ** -30]
    assert list(out[sh.ec0:sh.ew0]) == [1.0, 2.0, 297.0]
    assert list(out[sh.er0:sh.total]) == [1.0, 3 * 2.0 ** -40, 0.0]


def test_rounding_is_to_nearest_even_once():
    assert M.to_float((1 << 53) + 1, 1.0) == float(1 << 53)             # tie -> even
    assert M.to_float((1 << 53) + 3, 1.0) == float((1 << 53) + 4)
    assert M.to_float((1 << 54) + 2, 0.5) == float(1 << 53)             # the quantum does not round
    rng = np.random.default_rng(1)
    for _ in range(2000):                                               # the written-out division is the Fraction, digit for digit
        n = M.draw(rng, (1 << 103) - 1) * (1 if rng.integers(0, 8) else -1)
        for q in (1.0, 2.0 ** -40, 2.0 ** -97, 8.0):
            assert M.to_float(n, q) == float(Fraction(n) * Fraction(q))
    # hi 2^40 + lo rounded ONCE: rounding (double)lo first (to 2^61 + 2^40) makes the sum a tie, which goes to 2^93 + 2^61
    sh = M.Shape(0, 0)
    a = np.zeros(sh.total, dtype=np.int64)
    a[0], a[12] = (1 << 40) + (1 << 61) + 1, 1 << 53                    # exact total 2^93 + 2^61 + 2^40 + 1; ulp at 2^93 is 2^41
    out, _ = M.finalize_accumulator(a, None, sh, dict(Q, weight=1.0))
    assert out[0] == float((1 << 93) + (1 << 61) + (1 << 41))           # 2^40 + 1 is above the half-ulp tie 2^40: rounds up
    assert not M.accumulator_exact_mask(a, None, sh)[0]
    a[0] = (1 << 53)
    assert M.accumulator_exact_mask(a, None, sh)[0]


def test_thresholds_by_hand():
    sh, a = hand_accumulator()
    s = sh.s0

    def status(mut, limbs=None):
        b = a.copy()
        mut(b)
        return M.finalize_accumulator(b, limbs, sh, Q)[1]

    def set_(i, v):
        return lambda b: b.__setitem__(i, v)

    # wrapped: 2^62 - 1 is a value, 2^62 and -1 are not (conservation breaks as well: only the WRAPPED bit is looked at)
    assert not status(set_(s + 9, (1 << 62) - 1)) & M.WRAPPED
    assert status(set_(s + 9, 1 << 62)) & M.WRAPPED
    assert status(set_(s + 9, -1)) & M.WRAPPED
    limbs = np.zeros(sh.total, dtype=np.int64)
    assert status(lambda b: None, limbs) == 0
    limbs[s + 9] = -1
    assert status(lambda b: None, limbs) & M.WRAPPED
    # unresolved: 256 rays, 4096 * 256 - 1 quanta; 255 rays are not judged
    def faint(n, w, sq):
        def mut(b):
            b[:] = 0
            b[s + 1], b[s + 0], b[s + 17], b[s + 7] = n, w, w, sq
            b[sh.rw0], b[sh.ew0] = w, w
        return mut
    assert status(faint(256, 4096 * 256, 64 * 256)) == 0
    assert status(faint(256, 4096 * 256 - 1, 64 * 256)) == M.UNRESOLVED
    assert status(faint(255, 4096 * 256 - 1, 0)) == 0
    assert status(faint(255, 1, 0)) == 0
    # squares: NaN below 64 per ray, no status
    b = a.copy()
    faint(256, 4096 * 256, 64 * 256 - 1)(b)
    out, st = M.finalize_accumulator(b, None, sh, Q)
    assert st == 0 and math.isnan(out[s + 7])
    faint(256, 4096 * 256, 64 * 256)(b)
    out, st = M.finalize_accumulator(b, None, sh, Q)
    assert st == 0 and out[s + 7] == 64 * 256 * 2.0 ** -70
    faint(255, 4096 * 256, 0)(b)
    assert M.finalize_accumulator(b, None, sh, Q)[0][s + 7] == 0.0


def test_conservation_by_hand():
    sh, a = hand_accumulator()
    s = sh.s0
    for i in (0, 1, sh.rw0, sh.rw0 + 1, sh.ew0, sh.ew0 + 2, s + 17, s + 0):
        for d in (1, -1, T40):
            b = a.copy()
            b[i] += d
            if b[i] < 0:
                continue
            assert M.finalize_accumulator(b, None, sh, Q)[1] == M.NOT_CONSERVED, (i, d)
    # counts and the reflectivity spectrum are in no law
    for i in (sh.rc0, sh.ec0, sh.er0):
        b = a.copy()
        b[i] += 1
        assert M.finalize_accumulator(b, None, sh, Q)[1] == 0
    # a full wrap: SUM_WEIGHTS 2^64 above the pixels, every slot inside [0, 2^62)
    b = a.copy()
    b[s + 12] += 1 << 24
    assert M.finalize_accumulator(b, None, sh, Q)[1] == M.NOT_CONSERVED
    # limbs: the limb of a *_HI slot counts 2^80 - SUM_WEIGHTS_HI's limb 1 = pixel limbs of 2^40 in all
    limbs = np.zeros(sh.total, dtype=np.int64)
    limbs[s + 12] = 1
    assert M.finalize_accumulator(a, limbs, sh, Q)[1] == M.NOT_CONSERVED
    limbs[0], limbs[sh.rw0], limbs[sh.ew0 + 1] = T40, T40, T40
    out, st = M.finalize_accumulator(a, limbs, sh, Q)
    assert st == 0 and out[s] == float(Fraction((1 << 80) + 3 * T40 + 20) * Fraction(2.0 ** -30))


def test_rollover_by_hand():
    raw = np.array([5, T40, 3 * T40 + 9, (1 << 62) - 1, 0], dtype=np.int64)
    hi = np.array([0, 7, 1, 2, 4], dtype=np.int64)
    r, h, st = M.rollover(raw, hi)
    assert list(r) == [5, 0, 9, T40 - 1, 0] and list(h) == [0, 8, 4, 2 + (1 << 22) - 1, 4] and st == 0
    assert M.rollover(np.array([1 << 62]), np.array([0]))[2] == M.WRAPPED
    assert M.rollover(np.array([-1]), np.array([5]))[2] == M.WRAPPED
    assert M.rollover(np.array([T40]), np.array([-2]))[2] == M.WRAPPED       # the limb stays negative
    assert M.rollover(np.array([2 * T40]), np.array([-2]))[2] == 0


def test_scan_rows_by_hand():
    rows = np.zeros((3, 8), dtype=np.int64)
    rows[0, [0, 4, 1, 5, 2, 3]] = [9, 2, 64 * 300, 0, 300, 77]
    rows[1, [0, 4, 1, 5, 2]] = [4096 * 256 - 1, 0, 64 * 256 - 1, 0, 256]     # unresolved, squares too
    rows[2, :5] = [10, 9, 8, 7, 6]
    qw, q2 = [2.0 ** -20, 2.0 ** -22], [2.0 ** -50, 2.0 ** -52]
    out, st = M.finalize_scan(rows, 2, qw, q2, M.MASS_COUNTERS, False)
    out = out.reshape(3, 8)
    assert st == M.UNRESOLVED
    assert out[0, 0] == (2 * T40 + 9) * 2.0 ** -20 and out[0, 1] == 64 * 300 * 2.0 ** -50 and out[0, 2] == 300.0
    assert out[0, 3] == 0.0 and out[0, 4] == 0.0                              # slot 3 is no counter of the mass scan; *_HI reads 0
    assert out[1, 0] == (4096 * 256 - 1) * 2.0 ** -22 and math.isnan(out[1, 1])
    assert list(out[2]) == [10.0, 9.0, 8.0, 7.0, 6.0, 0.0, 0.0, 0.0]
    out, st = M.finalize_scan(rows, 2, qw, q2, M.ANGULAR_COUNTERS, True)
    out = out.reshape(3, 8)
    assert st == 0 and math.isnan(out[1, 0]) and math.isnan(out[1, 1]) and out[1, 2] == 256.0
    assert out[0, 3] == 77.0 and out[0, 0] == (2 * T40 + 9) * 2.0 ** -20
    rows[2, 7] = 1 << 62
    assert M.finalize_scan(rows, 2, qw, q2, M.ANGULAR_COUNTERS, True)[1] == M.WRAPPED


def test_shell_block_by_hand():
    n_s, n_e1 = 2, 3
    a = np.zeros(M.shell_block_len(n_s, n_e1, True), dtype=np.int64)
    a[0:8] = [50, 4, 30, 3, 7, 1, 1, 0]                      # shell 0: N_PASSED 3, SUM_WEIGHTS 2^40 + 7
    a[8:16] = [9, 0, 0, 256, 4096 * 256, 64 * 256 - 1, 0, 0]   # shell 1: resolved weights, unresolved squares
    a[16:19], a[19:22] = [1, 1, 1], [0, 256, 0]
    a[22:25], a[25:28] = [T40, 3, 4], [4096 * 256, 0, 0]
    out, st = M.finalize_shells(a, n_s, n_e1, True, Q)
    assert st == 0
    assert list(out[0:8]) == [50.0, 4.0, 30.0, 3.0, (T40 + 7) * 2.0 ** -30, 2.0 ** -70, 0.0, 0.0]
    assert math.isnan(out[8 + 5]) and out[8 + 4] == 4096 * 256 * 2.0 ** -30
    assert list(out[16:22]) == [1.0, 1.0, 1.0, 0.0, 256.0, 0.0] and out[22] == T40 * 2.0 ** -30
    for i, d in ((16, 1), (21, -1), (22, -1), (27, 1), (3, 1), (4, 1), (8 + 6, 1)):
        b = a.copy()
        b[i] += d
        assert M.finalize_shells(b, n_s, n_e1, True, Q)[1] & M.NOT_CONSERVED, (i, d)
    b = a.copy()
    b[8 + 4] -= 1
    b[25] -= 1
    assert M.finalize_shells(b, n_s, n_e1, True, Q)[1] == M.UNRESOLVED
    # without spectra the block has no law of its own
    b = a[:16].copy()
    b[3] = 200
    assert M.finalize_shells(b, n_s, n_e1, False, Q)[1] == 0


def test_channel_block_by_hand():
    t, n_e1, n_img = 2, 3, 2
    a = np.zeros(M.channel_block_len(t, n_e1, True, n_img), dtype=np.int64)
    a[0:8] = [7, 11, 5, 2, 1, 1, 0, 0]                       # channel 0: SUM_WEIGHTS 2^40 + 7, outside 2
    a[8:16] = [0, 0, 0, 0, 0, 0, 0, 0]                       # channel 1: empty
    a[16:19] = [T40, 7, 0]
    a[22:24] = [T40, 5]
    out, st = M.finalize_channels(a, t, n_e1, True, n_img, Q)
    assert st == 0
    assert list(out[0:8]) == [(T40 + 7) * 2.0 ** -30, (T40 + 11) * 2.0 ** -70, 5.0, 2 * 2.0 ** -30, 0.0, 0.0, 0.0, 0.0]
    assert out[16] == T40 * 2.0 ** -30 and out[23] == 5 * 2.0 ** -30
    for i in (0, 3, 4, 7, 16, 18, 19, 21, 22, 23, 24, 25, 8, 8 + 3):
        b = a.copy()
        b[i] += 1
        assert M.finalize_channels(b, t, n_e1, True, n_img, Q)[1] == M.NOT_CONSERVED, i
    # a faint channel is no error, and its squares never read NaN
    b = a.copy()
    b[8:16] = [300, 0, 300, 300, 0, 0, 0, 0]
    b[19] = 300
    out, st = M.finalize_channels(b, t, n_e1, True, n_img, Q)
    assert st == 0 and out[8 + 1] == 0.0
    # flux only: every ray is outside
    c = np.array([9, 1, 1, 9, 2, 0, 0, 2], dtype=np.int64)
    assert M.finalize_channels(c, 1, n_e1, False, 0, Q)[1] == 0
    c[3] = 8
    assert M.finalize_channels(c, 1, n_e1, False, 0, Q)[1] == M.NOT_CONSERVED


# ---- the builders against the model, and the model against a naive second computation ----------------------------------------------
SHAPES = [M.Shape(0, 0), M.Shape(1, 1), M.Shape(3, 5, 1, 4), M.Shape(4, 4, 7, 11), M.Shape(5, 3, 3, 2)]


def naive_accumulator(raw, limbs, sh, q):
    """Everything as Fractions of quanta; no limb is ever split."""
    val = [Fraction(int(v)) + (Fraction(int(limbs[i])) * T40 if limbs is not None else 0) for i, v in enumerate(raw)]
    s = sh.s0
    two = {k: val[s + k] + val[s + kh] * T40 for k, kh in M.ACC_TWO_LIMB.items()}
    bad = sum(val[:sh.n_img], Fraction(0)) + two[17] != two[0]
    if sh.spectra:
        bad = bad or sum(val[sh.rw0:sh.ec0]) != two[0] or sum(val[sh.ew0:sh.er0]) != two[0]
    wrapped = any(not 0 <= int(v) < 2 ** 62 for v in raw) or (limbs is not None and any(int(h) < 0 for h in limbs[sh.s0:sh.s0 + 24]))
    n = val[s + 1]
    st = (1 if wrapped else 0) | (2 if n >= 256 and two[0] / 4096 < n else 0) | (4 if bad else 0)
    out = [float(v * Fraction(q["weight"])) for v in val[:sh.n_img]] + [0.0] * 24
    for k in M.ACC_COUNTERS:
        out[s + k] = float(val[s + k])
    for k, name in M.ACC_QUANTUM.items():
        out[s + k] = float(two[k] * Fraction(q[name]))
    if n >= 256 and two[7] / 64 < n:
        out[s + 7] = float("nan")
    if sh.spectra:
        qs = [1.0] * sh.n_radial + [q["weight"]] * sh.n_radial + [1.0] * sh.n_e1 + [q["weight"]] * sh.n_e1 + [q["reflect"]] * sh.n_e1
        out += [float(v * Fraction(x)) for v, x in zip(val[sh.rc0:], qs)]
    return np.array(out), st


@pytest.mark.parametrize("unnormalised", [False, True])
def test_builders_satisfy_the_model_and_the_naive_computation_agrees(unnormalised):
    rng = np.random.default_rng(20 + unnormalised)
    seen_big = False
    for sh in SHAPES:
        for _ in range(25):
            a = M.consistent_accumulator(rng, sh, unnormalised)
            assert a.dtype == np.int64 and a.size == sh.total
            out, st = M.finalize_accumulator(a, None, sh, Q)
            assert st == 0, (sh, a)
            ref, st2 = naive_accumulator(a, None, sh, Q)
            assert st2 == 0 and np.array_equal(out, ref, equal_nan=True)
            lo = a[sh.s0 + 0]
            assert unnormalised or 0 <= lo < T40
            seen_big = seen_big or lo >= T40
            # rolled over: the same values, and limbs that are part of every sum
            r, h, rs = M.rollover(a, np.zeros_like(a))
            assert rs == 0 and all(0 <= int(x) < T40 for x in r)
            out2, st3 = M.finalize_accumulator(r, h, sh, Q)
            assert st3 == 0 and np.array_equal(out, out2, equal_nan=True)
            ref2, st4 = naive_accumulator(r, h, sh, Q)
            assert st4 == 0 and np.array_equal(out2, ref2, equal_nan=True)
    assert seen_big == unnormalised


def test_sums_of_built_accumulators_stay_consistent():
    rng = np.random.default_rng(5)
    sh = M.Shape(3, 3, 2, 5)
    for r in (2, 8, 1000):
        cap = (1 << 62) // r - 1
        total = sum(M.consistent_accumulator(rng, sh, False, slot_cap=cap) for _ in range(r))
        assert total.dtype == np.int64 and total.min() >= 0
        out, st = M.finalize_accumulator(total, None, sh, Q)
        assert st == 0
        assert np.array_equal(out, naive_accumulator(total, None, sh, Q)[0], equal_nan=True)
        if r == 1000:
            assert total[sh.s0] >= T40                   # the low limbs have left [0, 2^40)


def test_planted_single_slot_errors_are_flagged():
    rng = np.random.default_rng(9)
    for sh in SHAPES[1:]:
        a = M.consistent_accumulator(rng, sh, slot_cap=(1 << 61))
        law_slots = list(range(sh.n_img)) + [sh.s0 + 0, sh.s0 + 12, sh.s0 + 17, sh.s0 + 18]
        if sh.spectra:
            law_slots += list(range(sh.rw0, sh.ec0)) + list(range(sh.ew0, sh.er0))
        for i in law_slots:
            for d in (1, -1, T40):
                b = a.copy()
                b[i] += d
                st = M.finalize_accumulator(b, None, sh, Q)[1]
                assert st & (M.NOT_CONSERVED | M.WRAPPED), (sh, i, d)
                assert st == naive_accumulator(b, None, sh, Q)[1]
                if b[i] >= 0:
                    assert st & M.NOT_CONSERVED, (sh, i, d)


def test_scan_shell_and_channel_builders():
    rng = np.random.default_rng(3)
    for unnorm in (False, True):
        for n in (1, 5, 33):
            for counters, nan in ((M.MASS_COUNTERS, False), (M.ENERGY_COUNTERS, False), (M.ANGULAR_COUNTERS, True)):
                rows = M.consistent_scan(rng, n, counters, unnorm)
                out, st = M.finalize_scan(rows, n, [Q["weight"]] * n, [Q["weight_sq"]] * n, counters, nan)
                assert st == 0 and not np.isnan(out).any()
                v = rows.reshape(n + 1, 8)
                for k in range(n):                       # naive: one Fraction per sum
                    assert out[k * 8] == float((Fraction(int(v[k, 4])) * T40 + int(v[k, 0])) * Fraction(Q["weight"]))
        for spectra in (False, True):
            a = M.consistent_shells(rng, 4, 7, spectra, unnorm)
            out, st = M.finalize_shells(a, 4, 7, spectra, Q)
            assert st == 0 and not np.isnan(out).any()
            for n_img in (0, 6):
                c = M.consistent_channels(rng, 3, 7, spectra, n_img, unnorm)
                out, st = M.finalize_channels(c, 3, 7, spectra, n_img, Q)
                assert st == 0
                for i in range(len(c)):
                    if i % 8 == M.CHAN_RESERVED and i < 24 or i % 8 in (M.CHAN_SQ, M.CHAN_SQ_HI, M.CHAN_N) and i < 24:
                        continue
                    b = c.copy()
                    b[i] += 1
                    assert M.finalize_channels(b, 3, 7, spectra, n_img, Q)[1] & (M.NOT_CONSERVED | M.WRAPPED), (spectra, n_img, i)
