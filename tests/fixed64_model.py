"""Reference model of the SART_ACCUM_FIXED64 back end in plain Python integers (no GPU, no torch).

Written from include/sart.h ("accumulation mode", the layouts of the accumulator, the scan rows, the shell block and the channel
block), not from the kernels.  A raw buffer is a sequence of int64 slots; every value below is an exact Python integer and every
converted value is ``float(Fraction(integer) * Fraction(quantum))``: the integer times its power-of-two quantum, rounded to nearest
even once.

Two-limb sums: value = hi * 2^40 + lo, lo in the slot SART_*_SUM_*, hi in its *_HI slot; lo need not be below 2^40 (a limb-wise
int64 reduce over ranks leaves it larger).  With roll-over limbs (sart_rollover_accumulator_device) slot i stands for
limb[i] * 2^40 + raw[i], so the limb of a *_HI slot counts 2^80 quanta.

Status bits (what the next sart_synchronize turns into SART_ERR_ACCUMULATOR):
  WRAPPED        a raw slot outside [0, 2^62), or a negative roll-over limb under one of the SART_ACC_COUNT scalars (the roll-over
                 itself reports a limb that turns negative under any slot; under a pixel or a bin the finalize does not look at
                 the limb's sign by itself - its 2^40 quanta are part of the conservation sums, and that is where it shows)
  UNRESOLVED     N_PASSED >= 256 and SUM_WEIGHTS < 4096 N_PASSED   (not for channel blocks; the angular scan reads NaN instead)
  NOT_CONSERVED  accumulator: sum of the pixels != SUM_WEIGHTS - SUM_WEIGHTS_OUTSIDE, with spectra also sum of the radial weight
                 bins != SUM_WEIGHTS or sum of the energy weight bins != SUM_WEIGHTS
                 shell block (spectra): per shell N_PASSED != sum of its energy counts or SUM_WEIGHTS != sum of its energy weights
                 channel block: per channel SUM_WEIGHTS != sum of its energy bins (spectra) or != pixels + SUM_WEIGHTS_OUTSIDE
Converted values: SUM_WEIGHTS_SQ reads NaN when N_PASSED >= 256 and the squared sum is < 64 N_PASSED (accumulator, scan rows,
shells; not channels); the *_HI slots and the accumulator's SUM_WEIGHTS_OUTSIDE read 0.

How closely a finalize kernel is held to this model (``exact_mask``): the kernels convert the PARTS of a value to doubles and add
them once ("hi * 2^40 and lo are exact doubles: one rounding in the sum", "with a roll-over limb the sum of the two exact doubles
rounds once").  That promise is one rounding - the model's - wherever every part is an exact double, i.e. below 2^53 in magnitude:
  * single slots without roll-over limbs (pixels, radial / energy bins, counters, block bins): always bit for bit (one int64 ->
    double conversion, the power-of-two quantum is exact);
  * single slots with a roll-over limb: bit for bit where raw < 2^53 and |limb| < 2^53 (always after a roll-over: raw < 2^40);
  * two-limb sums (SUM_WEIGHTS, SUM_X, SUM_Y, SUM_R, SUM_WEIGHTS_SQ, the rows' and blocks' sums, a channel's OUTSIDE) without
    roll-over limbs: bit for bit where 0 <= lo < 2^53 and hi < 2^53 - every normalised accumulator and every limb-wise sum of up
    to 2^13 of them;
  * everything else (lo >= 2^53 after a very wide reduce; two-limb sums whose slots carry roll-over limbs): within 1 ulp.
"""
import math
from fractions import Fraction

import numpy as np

LIMB_BITS = 40
TWO40 = 1 << LIMB_BITS
MASK40 = TWO40 - 1
LIMIT = 1 << 62                 # a slot at or above it counts as wrapped
MIN_RAYS_FOR_MEANS = 256
MIN_QUANTA_PER_RAY = 4096       # SUM_WEIGHTS
MIN_SQ_QUANTA_PER_RAY = 64      # SUM_WEIGHTS_SQ
WRAPPED, UNRESOLVED, NOT_CONSERVED = 1, 2, 4

# include/sart.h: SART_ACC_*
ACC = dict(SUM_WEIGHTS=0, N_PASSED=1, N_PASSED_TILL_WINDOW=2, N_HIT_NICKEL=3, SUM_X=4, SUM_Y=5, SUM_R=6, SUM_WEIGHTS_SQ=7, N_RAYS=8,
           N_REACHED_TELESCOPE=9, N_SHELL_SELECTED=10, N_OUTSIDE_IMAGE=11, SUM_WEIGHTS_HI=12, SUM_X_HI=13, SUM_Y_HI=14, SUM_R_HI=15,
           SUM_WEIGHTS_SQ_HI=16, SUM_WEIGHTS_OUTSIDE=17, SUM_WEIGHTS_OUTSIDE_HI=18)
ACC_COUNT = 24
ACC_TWO_LIMB = {0: 12, 4: 13, 5: 14, 6: 15, 7: 16, 17: 18}          # lo slot -> hi slot
ACC_COUNTERS = (1, 2, 3, 8, 9, 10, 11)
ACC_QUANTUM = {0: "weight", 4: "position", 5: "position", 6: "position", 7: "weight_sq"}
# SART_SCAN_* / SART_ASCAN_* / SART_ESCAN_* (rows of 8: the sums sit in the same slots in all three)
ROW = 8
SCAN_SW, SCAN_SQ, SCAN_NP, SCAN_SW_HI, SCAN_SQ_HI = 0, 1, 2, 4, 5
MASS_COUNTERS = (2,)
ENERGY_COUNTERS = (2, 3)
ANGULAR_COUNTERS = (2, 3, 6, 7)
# SART_SHELL_*
SHELL_COUNTERS = (0, 1, 2, 3)
SHELL_NP, SHELL_SW, SHELL_SQ, SHELL_SW_HI, SHELL_SQ_HI = 3, 4, 5, 6, 7
# SART_CHAN_*
CHAN_SW, CHAN_SQ, CHAN_N, CHAN_OUT, CHAN_SW_HI, CHAN_SQ_HI, CHAN_RESERVED, CHAN_OUT_HI = 0, 1, 2, 3, 4, 5, 6, 7


class Shape:
    """Layout of one accumulator: image [ny][nx], SART_ACC_COUNT scalars, with ``n_radial`` > 0 the spectra behind them."""

    def __init__(self, nx, ny, n_radial=0, n_e1=0):
        self.nx, self.ny, self.n_radial, self.n_e1 = int(nx), int(ny), int(n_radial), int(n_e1)
        self.spectra = self.n_radial > 0
        self.n_img = self.nx * self.ny
        self.s0 = self.n_img
        self.rc0 = self.s0 + ACC_COUNT
        self.rw0 = self.rc0 + self.n_radial
        self.ec0 = self.rw0 + self.n_radial
        self.ew0 = self.ec0 + (self.n_e1 if self.spectra else 0)
        self.er0 = self.ew0 + (self.n_e1 if self.spectra else 0)
        self.total = self.er0 + (self.n_e1 if self.spectra else 0)

    def __repr__(self):
        return "Shape(%dx%d, radial %d, e1 %d)" % (self.nx, self.ny, self.n_radial, self.n_e1)


def ints(buf):
    return [int(x) for x in np.asarray(buf).reshape(-1)]


def to_float(n, q):
    """The exact integer n times the quantum q (a power of two), rounded to nearest even: float(Fraction(n) * Fraction(q)), which
    is numerator / denominator in Python's correctly rounded integer division - written out for q = 2^e, because the block models
    convert tens of thousands of slots per call (test_fixed64_model_cpu.py holds the two forms together)."""
    m, e = math.frexp(q)
    if m != 0.5:
        return float(Fraction(n) * Fraction(q))
    e -= 1
    return n / (1 << -e) if e < 0 else float(n << e)


def split_limbs(total, carry=0):
    """(lo, hi) with hi 2^40 + lo == total; carry > 0 leaves that many units of 2^40 in lo (an unnormalised pair)."""
    lo, hi = total & MASK40, total >> LIMB_BITS
    c = min(carry, hi)
    return lo + c * TWO40, hi - c


def _slot_wrapped(v):
    return v < 0 or v >= LIMIT


def _values(raw, limbs):
    return list(raw) if limbs is None else [h * TWO40 + v for v, h in zip(raw, limbs)]


def _means(n_passed, sw, sq):
    """(unresolved, squares unresolved)"""
    if n_passed < MIN_RAYS_FOR_MEANS:
        return False, False
    return sw < MIN_QUANTA_PER_RAY * n_passed, sq < MIN_SQ_QUANTA_PER_RAY * n_passed


def accumulator_sums(raw, limbs, shape):
    """The exact sums the conservation laws of an accumulator speak about (quanta)."""
    raw = ints(raw)
    val = _values(raw, None if limbs is None else ints(limbs))
    s0 = shape.s0
    two = {k: val[s0 + kh] * TWO40 + val[s0 + k] for k, kh in ACC_TWO_LIMB.items()}
    sums = {"pixels": sum(val[:shape.n_img]), "SUM_WEIGHTS": two[0], "SUM_WEIGHTS - outside": two[0] - two[17]}
    if shape.spectra:
        sums["radial bins"] = sum(val[shape.rw0:shape.rw0 + shape.n_radial])
        sums["energy bins"] = sum(val[shape.ew0:shape.ew0 + shape.n_e1])
    return sums, two, val


def finalize_accumulator(raw, limbs, shape, quanta):
    """Expected f64 layout (numpy array of shape.total doubles) and status bits of sart_finalize_accumulator[_limbs]_device.
    ``quanta``: dict with weight, weight_sq, position, reflect (sart_fixed_quanta_t)."""
    raw_i = ints(raw)
    assert len(raw_i) == shape.total
    limbs_i = None if limbs is None else ints(limbs)
    sums, two, val = accumulator_sums(raw_i, limbs_i, shape)
    status = 0
    s0 = shape.s0
    if any(_slot_wrapped(v) for v in raw_i) or (limbs_i is not None and any(h < 0 for h in limbs_i[s0:s0 + ACC_COUNT])):
        status |= WRAPPED
    unresolved, sq_nan = _means(val[s0 + ACC["N_PASSED"]], two[0], two[7])
    if unresolved:
        status |= UNRESOLVED
    bad = sums["pixels"] != sums["SUM_WEIGHTS - outside"]
    if shape.spectra:
        bad = bad or sums["radial bins"] != sums["SUM_WEIGHTS"] or sums["energy bins"] != sums["SUM_WEIGHTS"]
    if bad:
        status |= NOT_CONSERVED
    qw, qr = quanta["weight"], quanta["reflect"]
    out = np.zeros(shape.total)
    for i in range(shape.n_img):
        out[i] = to_float(val[i], qw)
    for k in ACC_COUNTERS:
        out[s0 + k] = to_float(val[s0 + k], 1.0)
    for k, name in ACC_QUANTUM.items():
        out[s0 + k] = to_float(two[k], quanta[name])
    if sq_nan:
        out[s0 + ACC["SUM_WEIGHTS_SQ"]] = float("nan")
    if shape.spectra:
        for i in range(shape.rc0, shape.total):
            q = 1.0 if i < shape.rw0 else qw if i < shape.ec0 else 1.0 if i < shape.ew0 else qw if i < shape.er0 else qr
            out[i] = to_float(val[i], q)
    return out, status


def _part_exact(v):
    return -(1 << 53) <= v <= (1 << 53)


def accumulator_exact_mask(raw, limbs, shape):
    """True where the finalize kernel's promise is one rounding (bit for bit), False where it is held to 1 ulp: module docstring."""
    raw_i = ints(raw)
    limbs_i = None if limbs is None else ints(limbs)
    if limbs_i is None:
        m = np.ones(shape.total, dtype=bool)
    else:
        m = np.array([_part_exact(v) and _part_exact(h) for v, h in zip(raw_i, limbs_i)])
    for k, kh in ACC_TWO_LIMB.items():
        m[shape.s0 + k] = limbs_i is None and 0 <= raw_i[shape.s0 + k] <= (1 << 53) and _part_exact(raw_i[shape.s0 + kh])
        m[shape.s0 + kh] = True
    return m


def rollover(raw, limbs):
    """sart_rollover_accumulator_device: (new raw, new limbs, status) - every slot keeps its low 40 bits, the rest moves to its limb."""
    raw_i, limbs_i = ints(raw), ints(limbs)
    new_raw = [v & MASK40 for v in raw_i]
    new_limbs = [h + (v >> LIMB_BITS) for v, h in zip(raw_i, limbs_i)]
    status = WRAPPED if any(_slot_wrapped(v) for v in raw_i) or any(h < 0 for h in new_limbs) else 0
    return np.array(new_raw, dtype=np.int64), np.array(new_limbs, dtype=np.int64), status


def finalize_scan(raw, n, q_w, q_w2, counters, unresolved_nan):
    """A scan accumulator of n rows + the counter row.  q_w / q_w2: one quantum per row.  ``counters``: the row slots that are plain
    counters.  unresolved_nan False (mass and energy scan): an unresolved row sets UNRESOLVED; True (angular scan): that row's
    SUM_WEIGHTS reads NaN and the status stays clean."""
    rows = np.asarray(raw).reshape(n + 1, ROW)
    out = np.zeros((n + 1, ROW))
    status = 0
    for k in range(n + 1):
        v = ints(rows[k])
        if any(_slot_wrapped(x) for x in v):
            status |= WRAPPED
        if k == n:
            out[k] = [to_float(x, 1.0) for x in v]
            break
        sw, sq = v[SCAN_SW_HI] * TWO40 + v[SCAN_SW], v[SCAN_SQ_HI] * TWO40 + v[SCAN_SQ]
        unresolved, sq_nan = _means(v[SCAN_NP], sw, sq)
        out[k, SCAN_SW] = to_float(sw, q_w[k])
        out[k, SCAN_SQ] = float("nan") if sq_nan else to_float(sq, q_w2[k])
        if unresolved:
            if unresolved_nan:
                out[k, SCAN_SW] = float("nan")
            else:
                status |= UNRESOLVED
        for j in counters:
            out[k, j] = to_float(v[j], 1.0)
    return out.reshape(-1), status


def scan_exact_mask(raw, n):
    rows = np.asarray(raw).reshape(n + 1, ROW)
    m = np.ones((n + 1, ROW), dtype=bool)
    for k in range(n):
        v = ints(rows[k])
        m[k, SCAN_SW] = 0 <= v[SCAN_SW] <= (1 << 53) and _part_exact(v[SCAN_SW_HI])
        m[k, SCAN_SQ] = 0 <= v[SCAN_SQ] <= (1 << 53) and _part_exact(v[SCAN_SQ_HI])
    return m.reshape(-1)


def shell_block_len(n_shells, n_e1, spectra):
    return n_shells * ROW + (2 * n_shells * n_e1 if spectra else 0)


def finalize_shells(raw, n_shells, n_e1, spectra, quanta):
    raw_i = ints(raw)
    assert len(raw_i) == shell_block_len(n_shells, n_e1, spectra)
    out = np.zeros(len(raw_i))
    status = WRAPPED if any(_slot_wrapped(v) for v in raw_i) else 0
    c0 = n_shells * ROW
    w0 = c0 + n_shells * n_e1
    for s in range(n_shells):
        v = raw_i[s * ROW:(s + 1) * ROW]
        sw, sq = v[SHELL_SW_HI] * TWO40 + v[SHELL_SW], v[SHELL_SQ_HI] * TWO40 + v[SHELL_SQ]
        unresolved, sq_nan = _means(v[SHELL_NP], sw, sq)
        if unresolved:
            status |= UNRESOLVED
        for j in SHELL_COUNTERS:
            out[s * ROW + j] = to_float(v[j], 1.0)
        out[s * ROW + SHELL_SW] = to_float(sw, quanta["weight"])
        out[s * ROW + SHELL_SQ] = float("nan") if sq_nan else to_float(sq, quanta["weight_sq"])
        if spectra:
            ec = raw_i[c0 + s * n_e1:c0 + (s + 1) * n_e1]
            ew = raw_i[w0 + s * n_e1:w0 + (s + 1) * n_e1]
            if sum(ec) != v[SHELL_NP] or sum(ew) != sw:
                status |= NOT_CONSERVED
            for e in range(n_e1):
                out[c0 + s * n_e1 + e] = to_float(ec[e], 1.0)
                out[w0 + s * n_e1 + e] = to_float(ew[e], quanta["weight"])
    return out, status


def channel_block_len(t, n_e1, spectra, n_img):
    return t * ROW + (t * n_e1 if spectra else 0) + t * n_img


def finalize_channels(raw, t, n_e1, spectra, n_img, quanta):
    raw_i = ints(raw)
    assert len(raw_i) == channel_block_len(t, n_e1, spectra, n_img)
    out = np.zeros(len(raw_i))
    status = WRAPPED if any(_slot_wrapped(v) for v in raw_i) else 0
    e0 = t * ROW
    p0 = e0 + (t * n_e1 if spectra else 0)
    for c in range(t):
        v = raw_i[c * ROW:(c + 1) * ROW]
        sw = v[CHAN_SW_HI] * TWO40 + v[CHAN_SW]
        sq = v[CHAN_SQ_HI] * TWO40 + v[CHAN_SQ]
        outside = v[CHAN_OUT_HI] * TWO40 + v[CHAN_OUT]
        pix = raw_i[p0 + c * n_img:p0 + (c + 1) * n_img]
        if sum(pix) + outside != sw:
            status |= NOT_CONSERVED
        if spectra:
            ew = raw_i[e0 + c * n_e1:e0 + (c + 1) * n_e1]
            if sum(ew) != sw:
                status |= NOT_CONSERVED
            for e in range(n_e1):
                out[e0 + c * n_e1 + e] = to_float(ew[e], quanta["weight"])
        for i, x in enumerate(pix):
            out[p0 + c * n_img + i] = to_float(x, quanta["weight"])
        out[c * ROW + CHAN_SW] = to_float(sw, quanta["weight"])
        out[c * ROW + CHAN_SQ] = to_float(sq, quanta["weight_sq"])
        out[c * ROW + CHAN_N] = to_float(v[CHAN_N], 1.0)
        out[c * ROW + CHAN_OUT] = to_float(outside, quanta["weight"])
    return out, status


def row_sums_exact_mask(raw, n_rows, pairs):
    """Exactness of the two-limb sums in the first n_rows rows of a shell or channel block; every other slot is a single slot."""
    raw_i = ints(raw)
    m = np.ones(len(raw_i), dtype=bool)
    for r in range(n_rows):
        for lo, hi in pairs:
            m[r * ROW + lo] = 0 <= raw_i[r * ROW + lo] <= (1 << 53) and _part_exact(raw_i[r * ROW + hi])
    return m


SHELL_PAIRS = ((SHELL_SW, SHELL_SW_HI), (SHELL_SQ, SHELL_SQ_HI))
CHAN_PAIRS = ((CHAN_SW, CHAN_SW_HI), (CHAN_SQ, CHAN_SQ_HI), (CHAN_OUT, CHAN_OUT_HI))
# SART_ORIGIN_* / SART_APERTURE_* (the aperture block has the origin block's head and cells): HEAD slots, then cells of CELL slots
HEAD, CELL = 8, 4
HEAD_NP, HEAD_SW, HEAD_SQ, HEAD_SW_HI, HEAD_SQ_HI = 0, 1, 2, 4, 5
CELL_N, CELL_SW, CELL_SQ = 0, 1, 2
HEAD_PAIRS = ((HEAD_SW, HEAD_SW_HI), (HEAD_SQ, HEAD_SQ_HI))
# SART_MSPEC_*: cells of MSPEC_CELL slots; the counts block behind the masses' blocks keeps N_ON_DETECTOR in slot MSPEC_N
MSPEC_CELL = 4
MSPEC_SW, MSPEC_SQ, MSPEC_SW_HI, MSPEC_SQ_HI = 0, 1, 2, 3
MSPEC_N = 0
MSPEC_PAIRS = ((MSPEC_SW, MSPEC_SW_HI), (MSPEC_SQ, MSPEC_SQ_HI))


# ---- builders: raw buffers that satisfy every law ---------------------------------------------------------------------------------
def draw(rng, cap):
    """An integer in [0, cap] from a mixture that straddles 2^40, 2^53 and the cap itself (2^62 - 1 by default)."""
    cap = int(cap)
    kind = int(rng.integers(0, 8))
    if kind == 0:
        v = int(rng.integers(0, 1 << 20))
    elif kind == 1:
        v = TWO40 + int(rng.integers(-3, 4))
    elif kind == 2:
        v = (1 << 53) + int(rng.integers(-3, 4))
    elif kind == 3:
        v = cap - int(rng.integers(0, 3))
    elif kind == 4:
        v = 0
    else:
        bits = int(rng.integers(1, max(cap.bit_length(), 1) + 1))
        v = int.from_bytes(rng.bytes(16), "little") >> max(128 - bits, 0)
    return min(max(v, 0), cap)


def fill(rng, total, n, cap=LIMIT - 1):
    """n integers in [0, cap] with a sum <= total, and what is left of total: every draw is bounded by twice the share that is
    still to be given out, so that the values spread over all n slots."""
    out = [0] * n
    left = total
    order = [int(i) for i in rng.permutation(n)]
    for todo, i in zip(range(n, 0, -1), order):
        out[i] = min(draw(rng, min(cap, 2 * (left // todo) + 3)), left)
        left -= out[i]
    return out, left, order


def partition(rng, total, n, cap=LIMIT - 1):
    """n integers in [0, cap] that add up to total (total <= n cap)."""
    assert 0 <= total <= n * cap
    out, left, order = fill(rng, total, n, cap)
    for i in order:
        if left == 0:
            break
        add = min(cap - out[i], left)
        out[i] += add
        left -= add
    assert left == 0 and sum(out) == total
    return out


def _sum_and_squares(rng, cap_total, slot_cap, hi_cap):
    """(SUM_WEIGHTS, N_PASSED, SUM_WEIGHTS_SQ) quanta, resolved: SUM_WEIGHTS >= 4096 N_PASSED, squares >= 64 N_PASSED."""
    sw = draw(rng, cap_total)
    n_passed = draw(rng, min(sw >> 12, slot_cap))
    sq = 64 * n_passed + draw(rng, hi_cap * TWO40 - 64 * n_passed)
    return sw, n_passed, sq


def consistent_accumulator(rng, shape, unnormalised=False, slot_cap=LIMIT - 1, hi_cap=None):
    """A raw accumulator (numpy int64, shape.total slots) that satisfies every law.  slot_cap bounds every single slot and every low
    limb of a normalised pair, hi_cap every high limb (default: slot_cap) - so that R of them can be added slot by slot.
    unnormalised: the low limbs keep some multiples of 2^40, as after a limb-wise reduce over ranks."""
    hi_cap = slot_cap if hi_cap is None else hi_cap
    two_cap = min(hi_cap, 1 << 50) * TWO40          # keeps limb sums of many buffers far from 2^62
    cap_total = two_cap
    if shape.spectra:
        cap_total = min(cap_total, slot_cap * min(shape.n_radial, shape.n_e1))
    a = [0] * shape.total
    s0 = shape.s0
    sw, n_passed, sq = _sum_and_squares(rng, cap_total, slot_cap, min(hi_cap, 1 << 50))
    pix, left, _ = fill(rng, sw, shape.n_img, slot_cap)
    a[:shape.n_img] = pix
    two = {0: sw, 17: left, 7: sq, 4: draw(rng, two_cap), 5: draw(rng, two_cap), 6: draw(rng, two_cap)}
    for k, kh in ACC_TWO_LIMB.items():
        carry = int(rng.integers(0, 1 << 21)) if unnormalised else 0
        lo, hi = split_limbs(two[k], carry)
        if lo > slot_cap:                              # (only with a small slot_cap and a carry)
            lo, hi = split_limbs(two[k])
        a[s0 + k], a[s0 + kh] = lo, hi
    a[s0 + ACC["N_PASSED"]] = n_passed
    for k in ACC_COUNTERS:
        if k != ACC["N_PASSED"]:
            a[s0 + k] = draw(rng, slot_cap)
    if shape.spectra:
        a[shape.rc0:shape.rw0] = partition(rng, n_passed, shape.n_radial, slot_cap)
        a[shape.rw0:shape.ec0] = partition(rng, sw, shape.n_radial, slot_cap)
        a[shape.ec0:shape.ew0] = partition(rng, n_passed, shape.n_e1, slot_cap)
        a[shape.ew0:shape.er0] = partition(rng, sw, shape.n_e1, slot_cap)
        a[shape.er0:shape.total] = [draw(rng, slot_cap) for _ in range(shape.n_e1)]
    return np.array(a, dtype=np.int64)


def consistent_scan(rng, n, counters, unnormalised=False, slot_cap=LIMIT - 1):
    """Raw scan accumulator: n resolved rows and the counter row (its first five slots)."""
    rows = np.zeros((n + 1, ROW), dtype=np.int64)
    for k in range(n):
        sw, n_passed, sq = _sum_and_squares(rng, min(slot_cap, 1 << 50) * TWO40, slot_cap, min(slot_cap, 1 << 50))
        carry = int(rng.integers(0, 1 << 21)) if unnormalised else 0
        rows[k, SCAN_SW], rows[k, SCAN_SW_HI] = split_limbs(sw, carry)
        rows[k, SCAN_SQ], rows[k, SCAN_SQ_HI] = split_limbs(sq, carry)
        for j in counters:
            rows[k, j] = draw(rng, slot_cap)
        rows[k, SCAN_NP] = n_passed
    rows[n, :5] = [draw(rng, slot_cap) for _ in range(5)]
    return rows.reshape(-1)


def consistent_shells(rng, n_shells, n_e1, spectra, unnormalised=False, slot_cap=LIMIT - 1):
    a = [0] * shell_block_len(n_shells, n_e1, spectra)
    c0 = n_shells * ROW
    w0 = c0 + n_shells * n_e1
    for s in range(n_shells):
        cap_total = min(slot_cap, 1 << 50) * TWO40
        if spectra:
            cap_total = min(cap_total, slot_cap * n_e1)
        sw, n_passed, sq = _sum_and_squares(rng, cap_total, slot_cap, min(slot_cap, 1 << 50))
        carry = int(rng.integers(0, 1 << 21)) if unnormalised else 0
        r = s * ROW
        a[r + SHELL_SW], a[r + SHELL_SW_HI] = split_limbs(sw, carry)
        a[r + SHELL_SQ], a[r + SHELL_SQ_HI] = split_limbs(sq, carry)
        for j in SHELL_COUNTERS:
            a[r + j] = draw(rng, slot_cap)
        a[r + SHELL_NP] = n_passed
        if spectra:
            a[c0 + s * n_e1:c0 + (s + 1) * n_e1] = partition(rng, n_passed, n_e1, slot_cap)
            a[w0 + s * n_e1:w0 + (s + 1) * n_e1] = partition(rng, sw, n_e1, slot_cap)
    return np.array(a, dtype=np.int64)


def consistent_channels(rng, t, n_e1, spectra, n_img, unnormalised=False, slot_cap=LIMIT - 1):
    a = [0] * channel_block_len(t, n_e1, spectra, n_img)
    e0 = t * ROW
    p0 = e0 + (t * n_e1 if spectra else 0)
    for c in range(t):
        cap_total = min(slot_cap, 1 << 50) * TWO40
        if spectra:
            cap_total = min(cap_total, slot_cap * n_e1)
        sw = draw(rng, cap_total)
        pix, left, _ = fill(rng, sw, n_img, slot_cap)
        a[p0 + c * n_img:p0 + (c + 1) * n_img] = pix
        carry = int(rng.integers(0, 1 << 21)) if unnormalised else 0
        r = c * ROW
        a[r + CHAN_SW], a[r + CHAN_SW_HI] = split_limbs(sw, carry)
        a[r + CHAN_OUT], a[r + CHAN_OUT_HI] = split_limbs(left, carry)
        a[r + CHAN_SQ], a[r + CHAN_SQ_HI] = split_limbs(draw(rng, min(slot_cap, 1 << 50) * TWO40), carry)
        a[r + CHAN_N] = draw(rng, slot_cap)
        if spectra:
            a[e0 + c * n_e1:e0 + (c + 1) * n_e1] = partition(rng, sw, n_e1, slot_cap)
    return np.array(a, dtype=np.int64)
