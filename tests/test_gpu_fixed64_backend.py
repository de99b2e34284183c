"""The SART_ACCUM_FIXED64 back end - finalize, roll-over, conservation checks and the limb-carrying folds - on crafted int64
buffers, held to the plain-integer model of tests/fixed64_model.py.

Every entry point here takes caller-owned device memory, so the values a real trace never produces (slots that straddle 2^40, 2^53
and 2^62 - 1, low limbs left unnormalised by a reduce, one stray quantum in one bin, a full 2^64 wrap) are written into the buffers
directly.  Every buffer is exactly as long as the entry point documents, followed by 64 sentinel slots that must come back untouched.
Errors are read from the code and message of ``synchronize`` alone."""
import ctypes as C
import re

import numpy as np
import pytest

import solaraxionraytracing_amd as sa
from solaraxionraytracing_amd import _lib as L
from solaraxionraytracing_amd import tables

from tests import fixed64_model as M
from tests.conftest import SMALL, make_setup

pytestmark = pytest.mark.gpu

N_E1 = SMALL["n_energies"] + 1          # 301 energy bins: crosses the 256-thread stride of the block kernels
SENT, SENTINEL = 64, 0x5A5A5A5A5A5A5A5A
TWO40, MASK40, LIMIT = M.TWO40, M.MASK40, M.LIMIT
N_FOLD = 100_000


def _torch():
    import torch
    return torch


# ---- device buffers -----------------------------------------------------------------------------------------------------------------
def upload(arr):
    """Device copy of an int64 array with SENT sentinel slots behind it; the copy has finished when this returns (the library
    works on the context's own stream)."""
    torch = _torch()
    arr = np.asarray(arr, dtype=np.int64).reshape(-1)
    buf = np.full(arr.size + SENT, SENTINEL, dtype=np.int64)
    buf[:arr.size] = arr
    d = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    return d


def blank(n):
    return upload(np.full(n, SENTINEL, dtype=np.int64))


def fetch(d, n):
    h = d.cpu().numpy()
    assert h.size == n + SENT and (h[n:] == SENTINEL).all(), "the slots behind the buffer were written"
    return h[:n].copy()


def sync(rt):
    try:
        rt.synchronize()
        return None
    except L.SartError as e:
        return e


def status_of(err):
    """The model's status bits, read from the code and message of a failed synchronize."""
    if err is None:
        return 0
    assert err.code == L.SART_ERR_ACCUMULATOR, str(err)
    msg = str(err)
    st = (M.WRAPPED if "negative or >= 2^62" in msg else 0) | (M.NOT_CONSERVED if "do not add up" in msg else 0) | \
         (M.UNRESOLVED if "average below 2^12 quanta" in msg else 0)
    assert st, msg
    return st


def message_sums(msg):
    """The `[quanta as lo + hi x 2^40: name lo + hi, ...]` record of a failed conservation check, as exact integers."""
    m = re.search(r"\[quanta as lo \+ hi x 2\^40:(.*?)\]", msg)
    assert m, msg
    out = {}
    for item in m.group(1).split(","):
        name, lo, hi = re.fullmatch(r"\s*(.+?) (-?\d+) \+ (-?\d+)", item).groups()
        assert 0 <= int(lo) < TWO40
        out[name] = int(lo) + int(hi) * TWO40
    return out


def assert_matches(out, exp, exact):
    """Bit for bit where `exact`, within 1 ulp elsewhere; NaN exactly where the model has NaN."""
    out, exp = np.ascontiguousarray(out), np.ascontiguousarray(exp)
    assert np.array_equal(np.isnan(out), np.isnan(exp)), (np.flatnonzero(np.isnan(out)), np.flatnonzero(np.isnan(exp)))
    ok = ~np.isnan(exp)
    d = np.abs(out.view(np.int64) - exp.view(np.int64))
    bad = np.flatnonzero(ok & exact & (d != 0))
    assert bad.size == 0, [(int(i), float(out[i]), float(exp[i])) for i in bad[:5]]
    bad = np.flatnonzero(ok & (d > 1))
    assert bad.size == 0, [(int(i), float(out[i]), float(exp[i])) for i in bad[:5]]


# ---- contexts ---------------------------------------------------------------------------------------------------------------------------
def open_fixed(name):
    """A context on the SMALL tables in FIXED64 mode whose quanta a flux-only launch of 1000 rays has frozen."""
    rt = sa.RayTracer(make_setup(name))
    rt.set_accumulation_mode("fixed64")
    freeze(rt)
    return rt


def freeze(rt):
    acc = upload(np.zeros(M.ACC_COUNT, dtype=np.int64))
    rt.trace_histogram_device(rt.trace_params(1000, seed=3, image_n=0), acc.data_ptr())
    rt.synchronize()
    fetch(acc, M.ACC_COUNT)
    return rt.fixed_quanta()


@pytest.fixture(scope="module")
def ctx():
    rt = open_fixed("babyiaxo_xmm")
    yield rt
    rt.close()


@pytest.fixture(scope="module")
def gas():
    rt = open_fixed("babyiaxo_xmm_gas")
    yield rt
    rt.close()


@pytest.fixture(scope="module")
def xray():
    rt = open_fixed("babyiaxo_xmm_xray")
    yield rt
    rt.close()


N_CHANNELS = 3


@pytest.fixture(scope="module")
def chan():
    rt = open_fixed("babyiaxo_xmm")
    total = tables.primakoff_emission_table(SMALL["n_radii"], SMALL["n_energies"])
    f = np.random.default_rng(77).random((N_CHANNELS,) + total.shape)
    rt.set_source_channels(f * total, total)
    yield rt
    rt.close()


def acc_params(rt, sh, n_rays=1, seed=11, accumulate=False):
    p = rt.trace_params(n_rays, seed=seed, image_n=0, accumulate=accumulate)
    p.image_nx, p.image_ny = sh.nx, sh.ny
    if sh.spectra:
        p.spectra, p.n_radial_bins, p.radial_max = 1, sh.n_radial, 10.0
    return p


def shape(nx, ny, n_radial=0):
    return M.Shape(nx, ny, n_radial, N_E1)


# ---- accumulator finalize ---------------------------------------------------------------------------------------------------------------
def run_finalize(rt, sh, raw, limbs=None, in_place=False):
    """(f64 output, error of the next synchronize) of sart_finalize_accumulator[_limbs]_device on a crafted buffer."""
    raw = np.asarray(raw, dtype=np.int64)
    assert raw.size == sh.total
    p = acc_params(rt, sh)
    d_raw = upload(raw)
    d_limbs = upload(limbs) if limbs is not None else None
    d_out = d_raw if in_place else blank(sh.total)
    if limbs is None:
        rt.finalize_accumulator_device(p, d_raw.data_ptr(), None if in_place else d_out.data_ptr())
    else:
        rt.finalize_accumulator_limbs_device(p, d_raw.data_ptr(), d_limbs.data_ptr(), None if in_place else d_out.data_ptr())
    err = sync(rt)
    out = fetch(d_out, sh.total).view(np.float64)
    if not in_place:
        assert np.array_equal(fetch(d_raw, sh.total), raw)
    if limbs is not None:
        assert np.array_equal(fetch(d_limbs, sh.total), limbs)
    return out, err


def check_against_model(rt, sh, raw, limbs=None, in_place_too=True):
    """Finalizes on the GPU and holds status and values to the model; returns the model's status."""
    q = rt.fixed_quanta()
    exp, st = M.finalize_accumulator(raw, limbs, sh, q)
    out, err = run_finalize(rt, sh, raw, limbs)
    assert status_of(err) == st, (st, str(err))
    if not st & M.WRAPPED:
        assert_matches(out, exp, M.accumulator_exact_mask(raw, limbs, sh))
    if in_place_too:
        out2, err2 = run_finalize(rt, sh, raw, limbs, in_place=True)
        assert status_of(err2) == st
        assert np.array_equal(out.view(np.int64), out2.view(np.int64))
    return st


IMAGES = [(0, 0), (1, 1), (15, 17), (16, 16), (19, 27)]
RADIAL = [0, 1, 7, 64]


@pytest.mark.parametrize("n_radial", RADIAL)
@pytest.mark.parametrize("image", IMAGES, ids=lambda im: "%dx%d" % im)
def test_consistent_accumulators_finalize_clean_and_equal_the_model(ctx, image, n_radial):
    sh = shape(image[0], image[1], n_radial)
    rng = np.random.default_rng(1000 * image[0] + 10 * image[1] + n_radial)
    for i in range(24):
        a = M.consistent_accumulator(rng, sh, unnormalised=(i % 3 == 2))
        assert check_against_model(ctx, sh, a) == 0


@pytest.mark.parametrize("ranks", [2, 8, 1000])
def test_slot_wise_sums_over_ranks_finalize_like_the_model_of_the_sum(ctx, ranks):
    """include/sart.h: "limb-wise int64 sums over up to 2^22 ranks stay exact" - the low limbs of the sum are no longer below 2^40."""
    sh = shape(15, 17, 7)
    rng = np.random.default_rng(ranks)
    cap = LIMIT // ranks - 1
    distinct = min(ranks, 40)
    parts = [M.consistent_accumulator(rng, sh, slot_cap=cap) for _ in range(distinct)]
    mult = np.ones(distinct, dtype=np.int64) if distinct == ranks else rng.multinomial(ranks - distinct, [1.0 / distinct] * distinct) + 1
    assert mult.sum() == ranks
    total = sum(int(m) * p for m, p in zip(mult, parts))
    assert total.dtype == np.int64 and total.min() >= 0 and total.max() < LIMIT
    if ranks == 1000:
        assert total[sh.s0 + M.ACC["SUM_WEIGHTS"]] >= TWO40 and total[sh.s0 + M.ACC["SUM_X"]] >= TWO40
    assert check_against_model(ctx, sh, total) == 0


_BASE = {}


def planted_base():
    """A consistent 19 x 27 accumulator with spectra whose planted slots all hold at least one quantum and stay below 2^61."""
    if "b" not in _BASE:
        sh = shape(19, 27, 7)
        slots = {"pixel_first": 0, "pixel_last": sh.n_img - 1, "pixel_255": 255, "pixel_256": 256, "radial_first": sh.rw0,
                 "radial_last": sh.rw0 + sh.n_radial - 1, "energy_0": sh.ew0, "energy_255": sh.ew0 + 255, "energy_256": sh.ew0 + 256,
                 "energy_300": sh.ew0 + 300, "outside": sh.s0 + M.ACC["SUM_WEIGHTS_OUTSIDE"]}
        for seed in range(400):
            a = M.consistent_accumulator(np.random.default_rng(seed), sh, slot_cap=1 << 61)
            if all(a[i] >= 1 for i in slots.values()):
                break
        else:
            raise AssertionError("no seed gives a base with every planted slot occupied")
        a.setflags(write=False)
        _BASE["b"] = (sh, a, slots)
    return _BASE["b"]


PLANT_SLOTS = ["pixel_first", "pixel_last", "pixel_255", "pixel_256", "radial_first", "radial_last", "energy_0", "energy_255",
               "energy_256", "energy_300", "outside"]


def refused_with_the_models_sums(rt, sh, bad, good):
    """`bad` must be refused for its conservation sums alone, with the model's sums in the message; `good` must then finalize cleanly
    on the same context (status cleared, no stale record)."""
    q = rt.fixed_quanta()
    exp_st = M.finalize_accumulator(bad, None, sh, q)[1]
    assert exp_st == M.NOT_CONSERVED
    out, err = run_finalize(rt, sh, bad)
    assert err is not None and err.code == L.SART_ERR_ACCUMULATOR and "do not add up" in str(err)
    assert status_of(err) == M.NOT_CONSERVED, str(err)
    sums = M.accumulator_sums(bad, None, sh)[0]
    assert message_sums(str(err)) == sums, (message_sums(str(err)), sums)
    assert sync(rt) is None                                   # reported once
    assert check_against_model(rt, sh, good, in_place_too=False) == 0


@pytest.mark.parametrize("delta", [1, -1, TWO40], ids=["plus1", "minus1", "plus2^40"])
@pytest.mark.parametrize("where", PLANT_SLOTS)
def test_one_stray_quantum_in_one_slot_is_refused(ctx, where, delta):
    sh, base, slots = planted_base()
    bad = base.copy()
    bad[slots[where]] += delta
    refused_with_the_models_sums(ctx, sh, bad, base)


@pytest.mark.parametrize("n_radial", [0, 7])
def test_a_full_2_64_wrap_that_lands_inside_the_range_is_refused(ctx, n_radial):
    """SUM_WEIGHTS stands 2^64 quanta above the pixels (+ outside): every slot is inside [0, 2^62), only the conservation sums see it."""
    sh = shape(19, 27, n_radial)
    base = M.consistent_accumulator(np.random.default_rng(64), sh, slot_cap=1 << 60)
    bad = base.copy()
    bad[sh.s0 + M.ACC["SUM_WEIGHTS_HI"]] += 1 << 24
    sums = M.accumulator_sums(bad, None, sh)[0]
    assert sums["SUM_WEIGHTS - outside"] - sums["pixels"] == 1 << 64
    refused_with_the_models_sums(ctx, sh, bad, base)


# -- thresholds: one slot at 2^62 - 1, 2^62 and -1, the rest rebalanced so that every law still holds
def _two_add(a, lo, hi, delta):
    t = a[hi] * TWO40 + a[lo] + delta
    if t < 0 or (t >> 40) >= LIMIT:
        return False
    a[lo], a[hi] = M.split_limbs(t)
    return True


def _spread(a, idxs, delta):
    for i in idxs:
        step = min(delta, LIMIT - 1 - a[i]) if delta > 0 else -min(-delta, a[i])
        a[i] += step
        delta -= step
    return delta == 0


def with_slot(base, sh, slot, value):
    """base with `slot` set to `value` and the other sides of its laws moved along; (buffer, whether every law could be kept)."""
    a = M.ints(base)
    s0 = sh.s0
    sw, out, sq = (s0 + 0, s0 + 12), (s0 + 17, s0 + 18), (s0 + 7, s0 + 16)
    rw, ew = list(range(sh.rw0, sh.ec0)), list(range(sh.ew0, sh.er0))
    d = value - a[slot]
    a[slot] = value
    spectra_ok = lambda dd, groups: all(_spread(a, [i for i in g if i != slot], dd) for g in groups) if sh.spectra else True
    if slot < sh.n_img or slot in out:
        dd = d * (TWO40 if slot == out[1] else 1)
        ok = _two_add(a, *sw, dd) and spectra_ok(dd, (rw, ew))
    elif slot in sw:
        dd = d * (TWO40 if slot == sw[1] else 1)
        ok = _two_add(a, *out, dd) and spectra_ok(dd, (rw, ew))
    elif slot in rw or slot in ew:
        ok = _two_add(a, *sw, d) and _two_add(a, *out, d) and spectra_ok(d, (ew if slot in rw else rw,))
    elif slot == s0 + M.ACC["N_PASSED"] and value > 0 and not sh.spectra:
        ok = _two_add(a, *sw, 4096 * value) and _two_add(a, *out, 4096 * value) and _two_add(a, *sq, 64 * value)
    else:
        ok = True
    if not ok:
        a = M.ints(base)
        a[slot] = value
    return np.array([v if -(1 << 63) <= v < (1 << 63) else 0 for v in a], dtype=np.int64), ok


def threshold_sweep(rt, sh, base, slots, must_stay_clean):
    seen = set()
    for slot in slots:
        for value in (LIMIT - 1, LIMIT, -1):
            a, kept = with_slot(base, sh, slot, value)
            st = check_against_model(rt, sh, a, in_place_too=False)
            assert bool(st & M.WRAPPED) == (value != LIMIT - 1), (slot, value, st)
            if kept:
                assert st == (0 if value == LIMIT - 1 else M.WRAPPED), (slot, value, st)
            seen.add((value, st))
            if value == LIMIT - 1 and slot in must_stay_clean:
                assert kept and st == 0, (slot, st)
    assert (LIMIT - 1, 0) in seen and (LIMIT, M.WRAPPED) in seen and (-1, M.WRAPPED) in seen


def test_slot_thresholds_in_the_image_and_the_spectra(ctx):
    sh = shape(19, 27, 7)
    base = M.consistent_accumulator(np.random.default_rng(5), sh, slot_cap=1 << 50)
    e = (0, 255, 256, 300)
    slots = [0, 255, 256, sh.n_img - 1, sh.rc0, sh.rw0 - 1, sh.rw0, sh.ec0 - 1] + [sh.ec0 + i for i in e] + [sh.ew0 + i for i in e] + \
            [sh.er0 + i for i in e]
    threshold_sweep(ctx, sh, base, slots, must_stay_clean=set(slots))


def test_slot_thresholds_in_every_scalar(ctx):
    sh = shape(19, 27)
    base = M.consistent_accumulator(np.random.default_rng(6), sh, slot_cap=1 << 50)
    assert base[sh.s0 + 12] >= 2 and base[sh.s0 + 18] >= 2     # room to take a limb away and stay consistent
    slots = [sh.s0 + k for k in range(19)]                      # (19 .. 23 are reserved: 0 in every accumulator)
    # 2^62 - 1 in SUM_WEIGHTS_OUTSIDE_HI alone would need SUM_WEIGHTS_HI beyond 2^62: every other scalar keeps every law
    threshold_sweep(ctx, sh, base, slots, must_stay_clean=set(slots) - {sh.s0 + 18})


def test_a_negative_roll_over_limb_is_a_wrapped_slot(ctx):
    """The value is kept (limb -1, slot + 2^40): nothing but the sign of the limb is wrong."""
    sh = shape(19, 27, 7)
    base = M.consistent_accumulator(np.random.default_rng(8), sh, slot_cap=1 << 50)
    zero = np.zeros(sh.total, dtype=np.int64)
    assert check_against_model(ctx, sh, base, zero) == 0
    for k in range(19):
        a, limbs = base.copy(), zero.copy()
        a[sh.s0 + k] += TWO40
        limbs[sh.s0 + k] = -1
        assert check_against_model(ctx, sh, a, limbs, in_place_too=False) == M.WRAPPED, k
    # under a pixel or a weight bin the limb's sign is not looked at by itself: its 2^40 quanta are missing from the sums
    for slot in (0, 256, sh.n_img - 1, sh.rw0, sh.ew0 + 300):
        limbs = zero.copy()
        limbs[slot] = -1
        assert check_against_model(ctx, sh, base, limbs, in_place_too=False) == M.NOT_CONSERVED, slot


@pytest.mark.parametrize("image", [(0, 0), (16, 16)], ids=["flux_only", "16x16"])
def test_the_means_are_judged_from_256_rays_on_and_from_both_sides(ctx, image):
    sh = shape(image[0], image[1], 7)
    s = sh.s0

    def faint(n, w, w2):
        a = np.zeros(sh.total, dtype=np.int64)
        a[s + M.ACC["N_PASSED"]], a[s + M.ACC["SUM_WEIGHTS"]], a[s + M.ACC["SUM_WEIGHTS_SQ"]] = n, w, w2
        a[0 if sh.n_img else s + M.ACC["SUM_WEIGHTS_OUTSIDE"]] = w
        a[sh.rw0 + 6], a[sh.ew0 + 300], a[sh.rc0], a[sh.ec0 + 256] = w, w, n, n
        return a

    q = ctx.fixed_quanta()
    edge = 4096 * 256
    assert check_against_model(ctx, sh, faint(256, edge, 64 * 256)) == 0
    assert check_against_model(ctx, sh, faint(256, edge - 1, 64 * 256)) == M.UNRESOLVED
    assert check_against_model(ctx, sh, faint(255, edge - 1, 64 * 256)) == 0
    assert check_against_model(ctx, sh, faint(255, edge, 64 * 256)) == 0
    assert check_against_model(ctx, sh, faint(255, 1, 0)) == 0
    out, err = run_finalize(ctx, sh, faint(256, edge, 64 * 256 - 1))
    assert err is None and np.isnan(out[s + M.ACC["SUM_WEIGHTS_SQ"]]) and np.isnan(out).sum() == 1
    out, err = run_finalize(ctx, sh, faint(256, edge, 64 * 256))
    assert err is None and out[s + M.ACC["SUM_WEIGHTS_SQ"]] == 64 * 256 * q["weight_sq"]
    out, err = run_finalize(ctx, sh, faint(255, edge, 64 * 256 - 1))
    assert err is None and out[s + M.ACC["SUM_WEIGHTS_SQ"]] == (64 * 256 - 1) * q["weight_sq"]
    _, err = run_finalize(ctx, sh, faint(256, edge - 1, 64 * 256))
    assert "average below 2^12 quanta" in str(err)


# ---- roll-over --------------------------------------------------------------------------------------------------------------------------
def run_rollover(rt, sh, raw, limbs):
    d_raw, d_limbs = upload(raw), upload(limbs)
    rt.rollover_accumulator_device(acc_params(rt, sh), d_raw.data_ptr(), d_limbs.data_ptr())
    err = sync(rt)
    return fetch(d_raw, sh.total), fetch(d_limbs, sh.total), err


@pytest.mark.parametrize("sh", [shape(0, 0), shape(15, 17, 7)], ids=["24_slots", "1196_slots"])
def test_rollover_moves_the_bits_above_2_40_into_the_limbs(ctx, sh):
    rng = np.random.default_rng(sh.total)
    for _ in range(6):
        raw = np.array([M.draw(rng, LIMIT - 1) for _ in range(sh.total)], dtype=np.int64)
        raw[:4] = [LIMIT - 1, TWO40 - 1, TWO40, 0]
        limbs = rng.integers(1, 1 << 30, size=sh.total, dtype=np.int64)
        r, h, err = run_rollover(ctx, sh, raw, limbs)
        er, eh, st = M.rollover(raw, limbs)
        assert st == 0 and err is None, str(err)
        assert np.array_equal(r, er) and np.array_equal(h, eh)
    for slot, value, limb in ((0, -1, 5), (sh.total - 1, LIMIT, 0), (7, 2 * TWO40, -3), (sh.total - 1, LIMIT - 1, -(1 << 22))):
        raw = np.array([M.draw(rng, LIMIT - 1) for _ in range(sh.total)], dtype=np.int64)
        limbs = rng.integers(0, 1 << 30, size=sh.total, dtype=np.int64)
        raw[slot], limbs[slot] = value, limb
        r, h, err = run_rollover(ctx, sh, raw, limbs)
        er, eh, st = M.rollover(raw, limbs)
        assert st == M.WRAPPED and status_of(err) == M.WRAPPED, (slot, value, limb, str(err))
        assert np.array_equal(r, er) and np.array_equal(h, eh)
    raw = np.full(sh.total, 3 * TWO40 + 1, dtype=np.int64)            # a limb that comes back to exactly 0 is fine
    limbs = np.full(sh.total, -3, dtype=np.int64)
    r, h, err = run_rollover(ctx, sh, raw, limbs)
    assert err is None and (r == 1).all() and (h == 0).all()


@pytest.mark.parametrize("n_radial", [0, 7])
def test_finalize_of_a_rolled_accumulator_equals_the_unrolled_one(ctx, n_radial):
    sh = shape(15, 17, n_radial)
    rng = np.random.default_rng(40 + n_radial)
    q = ctx.fixed_quanta()
    two_limb = np.zeros(sh.total, dtype=bool)
    two_limb[[sh.s0 + k for k in M.ACC_TWO_LIMB]] = True
    for i in range(8):
        a = M.consistent_accumulator(rng, sh, unnormalised=bool(i & 1))
        r, h, err = run_rollover(ctx, sh, a, np.zeros(sh.total, dtype=np.int64))
        assert err is None and ((0 <= r) & (r < TWO40)).all()
        exp, st = M.finalize_accumulator(a, None, sh, q)
        assert st == 0 and M.finalize_accumulator(r, h, sh, q)[1] == 0
        out, err = run_finalize(ctx, sh, r, h)
        assert err is None, str(err)
        assert_matches(out, exp, M.accumulator_exact_mask(r, h, sh))
        assert M.accumulator_exact_mask(r, h, sh)[~two_limb].all()    # every pixel, bin and counter: bit for bit
        plain, err = run_finalize(ctx, sh, a)
        assert err is None
        assert np.array_equal(out.view(np.int64)[~two_limb], plain.view(np.int64)[~two_limb])
        in_place, err = run_finalize(ctx, sh, r, h, in_place=True)
        assert err is None and np.array_equal(out.view(np.int64), in_place.view(np.int64))


# ---- scan finalize ------------------------------------------------------------------------------------------------------------------------
MASSES = [0.0, 0.008235, 0.005, 0.02, 0.05]
ENERGIES = [0.5, 1.5, 3.0, 6.0, 9.0]
ANGLES = [0.0, 0.05, -0.1, 0.2, 0.5]
SCAN_COUNTERS = {"mass": M.MASS_COUNTERS, "energy": M.ENERGY_COUNTERS, "angular": M.ANGULAR_COUNTERS}
_QUANTA = {}


def scan_points(kind, n):
    src = {"mass": MASSES, "energy": ENERGIES, "angular": ANGLES}[kind]
    return np.array([src[(3 * k) % 5] for k in range(n)])


def set_test_energy(rt, e):
    s = L.Setup()
    L.check(rt.lib.sart_get_setup(rt.handle, C.byref(s)))
    e0 = s.test_energy
    s.test_energy = float(e)
    L.check(rt.lib.sart_set_setup(rt.handle, C.byref(s)))
    return e0


def point_quanta(rt, kind, x):
    """The quanta a single-point FIXED64 launch of the same context freezes at that mass / energy - from the host, never from the
    output under test."""
    key = (kind, float(x))
    if key not in _QUANTA:
        if kind == "mass":
            rt.set_axion_mass(float(x))
            try:
                _QUANTA[key] = freeze(rt)
            finally:
                rt.set_axion_mass(rt.full.setup.m_axion)
        elif kind == "energy":
            e0 = set_test_energy(rt, x)
            try:
                _QUANTA[key] = freeze(rt)
            finally:
                set_test_energy(rt, e0)
        else:
            _QUANTA[key] = rt.fixed_quanta()
    return _QUANTA[key]


def run_scan_finalize(rt, kind, xs, raw, in_place=False):
    n = len(xs)
    p = rt.trace_params(1, seed=11, image_n=0)
    d_raw = upload(raw)
    d_out = d_raw if in_place else blank(raw.size)
    out_ptr = None if in_place else d_out.data_ptr()
    if kind == "mass":
        rt.finalize_mass_scan_device(p, xs, d_raw.data_ptr(), out_ptr)
    elif kind == "energy":
        rt.finalize_energy_scan_device(p, xs, d_raw.data_ptr(), out_ptr)
    else:
        rt.finalize_angular_scan_device(p, n, d_raw.data_ptr(), out_ptr)
    err = sync(rt)
    out = fetch(d_out, raw.size).view(np.float64)
    if not in_place:
        assert np.array_equal(fetch(d_raw, raw.size), raw)
    return out, err


def check_scan(rt, kind, xs, raw, qs, in_place_too=False):
    n = len(xs)
    exp, st = M.finalize_scan(raw, n, [q["weight"] for q in qs], [q["weight_sq"] for q in qs], SCAN_COUNTERS[kind], kind == "angular")
    out, err = run_scan_finalize(rt, kind, xs, raw)
    assert status_of(err) == st, (st, str(err))
    if not st & M.WRAPPED:
        assert_matches(out, exp, M.scan_exact_mask(raw, n))
    if in_place_too:
        out2, err2 = run_scan_finalize(rt, kind, xs, raw, in_place=True)
        assert status_of(err2) == st and np.array_equal(out.view(np.int64), out2.view(np.int64))
    return st, out


@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 65])
@pytest.mark.parametrize("kind", ["mass", "energy", "angular"])
def test_scan_finalize_on_crafted_rows(request, kind, n):
    rt = request.getfixturevalue({"mass": "gas", "energy": "xray", "angular": "ctx"}[kind])
    xs = scan_points(kind, n)
    qs = [point_quanta(rt, kind, x) for x in xs]
    counters = SCAN_COUNTERS[kind]
    rng = np.random.default_rng(100 * n + len(kind))
    for unnormalised in (False, True):
        rows = M.consistent_scan(rng, n, counters, unnormalised)
        st, out = check_scan(rt, kind, xs, rows, qs, in_place_too=True)
        assert st == 0 and not np.isnan(out).any()
        # the counter row behind the last group: verbatim
        assert np.array_equal(out.reshape(n + 1, 8)[n], rows.reshape(n + 1, 8)[n].astype(np.float64))
    # one slot at 2^62 - 1, 2^62, -1: first row, last row, counter row (sums far above every resolution limit)
    base = M.consistent_scan(rng, n, counters, slot_cap=1 << 50).reshape(n + 1, 8)
    base[:n, M.SCAN_SW_HI] = base[:n, M.SCAN_SQ_HI] = TWO40
    seen = set()
    for r in sorted({0, n - 1, n}):
        for j in range(8):
            for value in (LIMIT - 1, LIMIT, -1):
                a = base.copy()
                a[r, j] = value
                st, _ = check_scan(rt, kind, xs, a.reshape(-1), qs)
                assert bool(st & M.WRAPPED) == (value != LIMIT - 1), (r, j, value, st)
                seen.add((value == LIMIT - 1, st))
    assert (True, 0) in seen and (False, M.WRAPPED) in seen
    # an unresolved row, from both sides
    r = n // 2
    a = base.copy()
    a[r, :] = 0
    a[r, M.SCAN_NP], a[r, M.SCAN_SW], a[r, M.SCAN_SQ] = 256, 4096 * 256, 64 * 256
    st, out = check_scan(rt, kind, xs, a.reshape(-1), qs)
    assert st == 0 and not np.isnan(out).any()
    a[r, M.SCAN_SW] -= 1
    st, out = check_scan(rt, kind, xs, a.reshape(-1), qs)
    out = out.reshape(n + 1, 8)
    if kind == "angular":
        assert st == 0 and np.isnan(out[r, M.SCAN_SW]) and np.isnan(out).sum() == 1 and out[r, M.SCAN_NP] == 256.0
    else:
        assert st == M.UNRESOLVED
    a[r, M.SCAN_NP] = 255
    st, out = check_scan(rt, kind, xs, a.reshape(-1), qs)
    assert st == 0 and not np.isnan(out).any()


# ---- shell and channel blocks ---------------------------------------------------------------------------------------------------------
def run_block_finalize(rt, which, p, raw, in_place=False):
    d_raw = upload(raw)
    d_out = d_raw if in_place else blank(raw.size)
    fin = rt.finalize_shells_device if which == "shells" else rt.finalize_channels_device
    fin(p, d_raw.data_ptr(), None if in_place else d_out.data_ptr())
    err = sync(rt)
    out = fetch(d_out, raw.size).view(np.float64)
    if not in_place:
        assert np.array_equal(fetch(d_raw, raw.size), raw)
    return out, err


def check_block(rt, which, p, raw, model, pairs, n_rows, in_place_too=False):
    exp, st = model(raw)
    out, err = run_block_finalize(rt, which, p, raw)
    assert status_of(err) == st, (st, str(err))
    if not st & M.WRAPPED:
        assert_matches(out, exp, M.row_sums_exact_mask(raw, n_rows, pairs))
    if in_place_too:
        out2, err2 = run_block_finalize(rt, which, p, raw, in_place=True)
        assert status_of(err2) == st and np.array_equal(out.view(np.int64), out2.view(np.int64))
    return st, out


@pytest.mark.parametrize("spectra", [False, True], ids=["rows", "spectra"])
def test_shell_block_finalize_on_crafted_blocks(ctx, spectra):
    n_s = ctx.full.setup.n_shells
    p = ctx.shells_params(1, image_n=0, spectra=spectra, n_radial_bins=7)
    q = ctx.fixed_quanta()
    assert ctx.shell_block_len(spectra) == M.shell_block_len(n_s, N_E1, spectra)
    model = lambda raw: M.finalize_shells(raw, n_s, N_E1, spectra, q)
    check = lambda raw, **kw: check_block(ctx, "shells", p, raw, model, M.SHELL_PAIRS, n_s, **kw)
    rng = np.random.default_rng(31 + spectra)
    for i in range(6):
        st, out = check(M.consistent_shells(rng, n_s, N_E1, spectra, unnormalised=bool(i & 1)), in_place_too=True)
        assert st == 0 and not np.isnan(out).any()
    c0 = n_s * 8
    w0 = c0 + n_s * N_E1
    bins = [g + s * N_E1 + e for g in (c0, w0) for s in (0, n_s - 1) for e in (0, 255, 256, 300)] if spectra else []
    base = M.consistent_shells(rng, n_s, N_E1, spectra, slot_cap=1 << 50)
    if spectra:                                             # every planted bin occupied: a quantum can be taken away as well
        for s in (0, n_s - 1):
            for e in (0, 255, 256, 300):                    # one more ray of 8192 quanta (64 squared) in each of these bins
                base[c0 + s * N_E1 + e] += 1
                base[w0 + s * N_E1 + e] += 8192
                base[s * 8 + M.SHELL_NP] += 1
                base[s * 8 + M.SHELL_SW] += 8192
                base[s * 8 + M.SHELL_SQ] += 64
    assert all(base[i] >= 1 for i in bins) and model(base)[1] == 0
    slots = [s * 8 + j for s in (0, n_s - 1) for j in range(8)]
    if spectra:
        slots += [g + s * N_E1 + e for g in (c0, w0) for s in (0, n_s - 1) for e in (0, 255, 256, 300)]
    seen = set()
    for slot in slots:
        for value in (LIMIT - 1, LIMIT, -1):
            a = base.copy()
            a[slot] = value
            st, _ = check(a)
            assert bool(st & M.WRAPPED) == (value != LIMIT - 1), (slot, value, st)
            seen.add((value == LIMIT - 1, st))
    assert (True, 0) in seen
    if spectra:
        # one stray count or quantum in one bin of the first or last shell
        for g in (c0, w0):
            for s in (0, n_s - 1):
                for e in (0, 255, 256, 300):
                    for d in (1, -1):
                        a = base.copy()
                        a[g + s * N_E1 + e] += d
                        if a[g + s * N_E1 + e] < 0:
                            continue
                        st, _ = check(a)
                        assert st & M.NOT_CONSERVED and not st & M.WRAPPED, (g, s, e, d, st)
        for s in (0, n_s - 1):
            for j in (M.SHELL_NP, M.SHELL_SW, M.SHELL_SW_HI):
                a = base.copy()
                a[s * 8 + j] += 1
                st, _ = check(a)
                assert st & M.NOT_CONSERVED, (s, j, st)
        assert check(base)[0] == 0
    # squared weights that are not resolved read NaN in that shell alone
    a = base.copy()
    s = n_s // 2
    a[s * 8:(s + 1) * 8] = 0
    a[s * 8 + M.SHELL_NP], a[s * 8 + M.SHELL_SW], a[s * 8 + M.SHELL_SQ] = 256, 4096 * 256, 64 * 256 - 1
    if spectra:
        a[c0 + s * N_E1:c0 + (s + 1) * N_E1] = 0
        a[w0 + s * N_E1:w0 + (s + 1) * N_E1] = 0
        a[c0 + s * N_E1 + 256], a[w0 + s * N_E1 + 300] = 256, 4096 * 256
    st, out = check(a)
    assert st == 0 and np.isnan(out[s * 8 + M.SHELL_SQ]) and np.isnan(out).sum() == 1
    a[s * 8 + M.SHELL_SQ] += 1
    st, out = check(a)
    assert st == 0 and out[s * 8 + M.SHELL_SQ] == 64 * 256 * q["weight_sq"]
    a[s * 8 + M.SHELL_SW] -= 1
    if spectra:
        a[w0 + s * N_E1 + 300] -= 1
    assert check(a)[0] == M.UNRESOLVED


@pytest.mark.parametrize("image_n", [0, 16])
@pytest.mark.parametrize("spectra", [False, True], ids=["rows", "spectra"])
def test_channel_block_finalize_on_crafted_blocks(chan, spectra, image_n):
    t, n_img = N_CHANNELS, image_n * image_n
    p = chan.channels_params(1, image_n=image_n, spectra=spectra, n_radial_bins=7)
    q = chan.fixed_quanta()
    assert chan.channel_block_len(spectra, image_n) == M.channel_block_len(t, N_E1, spectra, n_img)
    model = lambda raw: M.finalize_channels(raw, t, N_E1, spectra, n_img, q)
    check = lambda raw, **kw: check_block(chan, "channels", p, raw, model, M.CHAN_PAIRS, t, **kw)
    rng = np.random.default_rng(53 + 2 * spectra + image_n)
    for i in range(6):
        st, out = check(M.consistent_channels(rng, t, N_E1, spectra, n_img, unnormalised=bool(i & 1)), in_place_too=True)
        assert st == 0 and not np.isnan(out).any()
    e0 = t * 8
    p0 = e0 + (t * N_E1 if spectra else 0)
    law = [c * 8 + j for c in (0, t - 1) for j in (M.CHAN_SW, M.CHAN_OUT)]
    if spectra:
        law += [e0 + c * N_E1 + e for c in (0, t - 1) for e in (0, 255, 256, 300)]
    if n_img:
        law += [p0 + c * n_img + i for c in (0, t - 1) for i in (0, n_img - 1)]
    for seed in range(400):
        base = M.consistent_channels(np.random.default_rng(seed), t, N_E1, spectra, n_img, slot_cap=1 << 50)
        if all(base[i] >= 1 for i in law):
            break
    assert all(base[i] >= 1 for i in law)
    assert check(base)[0] == 0
    for slot in law:
        for d in (1, -1):
            a = base.copy()
            a[slot] += d
            assert check(a)[0] == M.NOT_CONSERVED, (slot, d)
    assert check(base)[0] == 0
    others = [c * 8 + j for c in (0, t - 1) for j in (M.CHAN_SQ, M.CHAN_N, M.CHAN_SW_HI, M.CHAN_SQ_HI, M.CHAN_OUT_HI)]
    seen = set()
    for slot in law + others:
        for value in (LIMIT - 1, LIMIT, -1):
            a = base.copy()
            a[slot] = value
            st, _ = check(a)
            assert bool(st & M.WRAPPED) == (value != LIMIT - 1), (slot, value, st)
            seen.add((value == LIMIT - 1, st))
    assert (True, 0) in seen
    # a faint channel is no error and its squares never read NaN
    a = base.copy()
    a[0:8] = 0
    a[M.CHAN_SW], a[M.CHAN_OUT], a[M.CHAN_N] = 300, 300, 300
    if spectra:
        a[e0:e0 + N_E1] = 0
        a[e0 + 256] = 300
    a[p0:p0 + n_img] = 0
    st, out = check(a)
    assert st == 0 and out[M.CHAN_SQ] == 0.0 and not np.isnan(out).any()


# ---- the folds: accumulate = 1 launches onto crafted buffers ----------------------------------------------------------------------------
def top_pair(a, lo, hi, carry):
    """The pair's low limb at 2^40 - 1 (+ carry x 2^40: unnormalised); returns the quanta added to the pair's value."""
    d = MASK40 - (a[lo] & MASK40)
    t = a[hi] * TWO40 + a[lo] + d
    a[lo], a[hi] = M.split_limbs(t, carry)
    assert a[lo] & MASK40 == MASK40
    return d


def crafted_accumulator(sh, seed, carry):
    a = M.ints(M.consistent_accumulator(np.random.default_rng(seed), sh, slot_cap=1 << 60))
    s0 = sh.s0
    big = 1 << 61                                             # high limbs of at least 2^21: room for the carry
    for lo, hi in ((s0 + 17, s0 + 18), (s0 + 0, s0 + 12)):
        a[lo], a[hi] = M.split_limbs(a[hi] * TWO40 + a[lo] + big)
    if sh.spectra:
        a[sh.rw0 + 1] += big
        a[sh.ew0 + 1] += big
    for k in (4, 5, 6, 7):
        a[s0 + M.ACC_TWO_LIMB[k]] += 1 << 21
    d = top_pair(a, s0 + 17, s0 + 18, carry)                  # OUTSIDE, and SUM_WEIGHTS with it
    t = a[s0 + 12] * TWO40 + a[s0 + 0] + d
    a[s0 + 0], a[s0 + 12] = M.split_limbs(t)
    d2 = top_pair(a, s0 + 0, s0 + 12, carry)
    if sh.n_img:
        a[0] += d2
    else:
        assert d2 == 0
    if sh.spectra:
        a[sh.rw0] += d + d2
        a[sh.ew0] += d + d2
    for k in (4, 5, 6, 7):
        top_pair(a, s0 + k, s0 + M.ACC_TWO_LIMB[k], carry)
    return np.array(a, dtype=np.int64)


def assert_folded(before, traced, after, pairs):
    """after == before + traced as integers: slot for slot, and as hi 2^40 + lo for the (lo, hi) pairs, whose lo is normalised."""
    b, a, c = M.ints(before), M.ints(traced), M.ints(after)
    in_pair = set()
    for lo, hi in pairs:
        in_pair.update((lo, hi))
        assert 0 <= c[lo] < TWO40, (lo, c[lo])
        assert 0 <= a[lo] < TWO40
        assert c[hi] * TWO40 + c[lo] == b[hi] * TWO40 + b[lo] + a[hi] * TWO40 + a[lo], (lo, hi)
    bad = [i for i in range(len(b)) if i not in in_pair and c[i] != b[i] + a[i]]
    assert not bad, [(i, b[i], a[i], c[i]) for i in bad[:5]]


def fold_through(rt, launch, lens, befores):
    """Traces N_FOLD rays into zeroed buffers (A) and, with accumulate = 1, onto copies of `befores` (C); returns (A list, C list)."""
    zero = [upload(np.zeros(n, dtype=np.int64)) for n in lens]
    launch(False, [d.data_ptr() for d in zero])
    assert sync(rt) is None
    onto = [upload(b) for b in befores]
    launch(True, [d.data_ptr() for d in onto])
    assert sync(rt) is None
    return [fetch(d, n) for d, n in zip(zero, lens)], [fetch(d, n) for d, n in zip(onto, lens)]


def acc_pairs(sh):
    return [(sh.s0 + lo, sh.s0 + hi) for lo, hi in M.ACC_TWO_LIMB.items()]


@pytest.mark.parametrize("carry", [0, 1 << 20], ids=["normalised", "unnormalised"])
@pytest.mark.parametrize("sh", [shape(0, 0), shape(16, 16), shape(19, 27, 7)], ids=["flux_only", "16x16", "19x27_spectra"])
def test_histogram_launch_folds_onto_a_crafted_accumulator(ctx, sh, carry):
    b = crafted_accumulator(sh, 3, carry)
    q = ctx.fixed_quanta()
    assert M.finalize_accumulator(b, None, sh, q)[1] == 0
    launch = lambda acc, ptrs: ctx.trace_histogram_device(acc_params(ctx, sh, N_FOLD, seed=21, accumulate=acc), ptrs[0])
    (a,), (c,) = fold_through(ctx, launch, [sh.total], [b])
    assert a[sh.s0 + M.ACC["N_RAYS"]] == N_FOLD and a[sh.s0 + M.ACC["N_PASSED"]] > 1000
    assert_folded(b, a, c, acc_pairs(sh))
    assert c[sh.s0 + M.ACC["N_RAYS"]] == b[sh.s0 + M.ACC["N_RAYS"]] + N_FOLD
    assert check_against_model(ctx, sh, c, in_place_too=False) == 0


def crafted_rows(n, counters, seed, carry):
    rows = M.ints(M.consistent_scan(np.random.default_rng(seed), n, counters, slot_cap=1 << 60))
    for k in range(n):
        rows[k * 8 + M.SCAN_SW_HI] += 1 << 21                 # room for the carry
        rows[k * 8 + M.SCAN_SQ_HI] += 1 << 21
        top_pair(rows, k * 8 + M.SCAN_SW, k * 8 + M.SCAN_SW_HI, carry)
        top_pair(rows, k * 8 + M.SCAN_SQ, k * 8 + M.SCAN_SQ_HI, carry)
    return np.array(rows, dtype=np.int64)


@pytest.mark.parametrize("carry", [0, 1 << 20], ids=["normalised", "unnormalised"])
@pytest.mark.parametrize("kind,n", [("mass", 33), ("energy", 5), ("angular", 5)])
def test_scan_launch_folds_onto_crafted_rows(request, kind, n, carry):
    rt = request.getfixturevalue({"mass": "gas", "energy": "xray", "angular": "ctx"}[kind])
    xs = scan_points(kind, n) if kind != "mass" else np.linspace(0.002, 0.03, n)
    b = crafted_rows(n, SCAN_COUNTERS[kind], 17, carry)
    trace = {"mass": rt.trace_mass_scan_device, "energy": rt.trace_energy_scan_device, "angular": rt.trace_angular_scan_device}[kind]
    launch = lambda acc, ptrs: trace(rt.trace_params(N_FOLD, seed=22, accumulate=acc), xs, ptrs[0])
    (a,), (c,) = fold_through(rt, launch, [(n + 1) * 8], [b])
    assert a[n * 8] == N_FOLD and a.reshape(n + 1, 8)[:n, M.SCAN_NP].max() > 100
    assert_folded(b, a, c, [(k * 8 + lo, k * 8 + hi) for k in range(n) for lo, hi in ((M.SCAN_SW, M.SCAN_SW_HI), (M.SCAN_SQ, M.SCAN_SQ_HI))])
    assert c[n * 8] == b[n * 8] + N_FOLD


@pytest.mark.parametrize("carry", [0, 1 << 20], ids=["normalised", "unnormalised"])
def test_shell_launch_folds_onto_a_crafted_block(ctx, carry):
    sh = shape(16, 16, 7)
    n_s = ctx.full.setup.n_shells
    b_acc = crafted_accumulator(sh, 4, carry)
    blk = M.ints(M.consistent_shells(np.random.default_rng(18), n_s, N_E1, True, slot_cap=1 << 60))
    w0 = n_s * 8 + n_s * N_E1
    for s in range(n_s):
        blk[s * 8 + M.SHELL_SW_HI] += 1 << 21                 # room for the carry, with its 2^61 quanta in an energy bin
        blk[s * 8 + M.SHELL_SQ_HI] += 1 << 21
        blk[w0 + s * N_E1 + 1] += 1 << 61
        blk[w0 + s * N_E1] += top_pair(blk, s * 8 + M.SHELL_SW, s * 8 + M.SHELL_SW_HI, carry)
        top_pair(blk, s * 8 + M.SHELL_SQ, s * 8 + M.SHELL_SQ_HI, carry)
    b_blk = np.array(blk, dtype=np.int64)
    q = ctx.fixed_quanta()
    assert M.finalize_shells(b_blk, n_s, N_E1, True, q)[1] == 0
    params = lambda acc: ctx.shells_params(N_FOLD, seed=23, image_n=16, spectra=True, n_radial_bins=7, accumulate=acc)
    launch = lambda acc, ptrs: ctx.trace_shells_device(params(acc), ptrs[0], ptrs[1])
    (a_acc, a_blk), (c_acc, c_blk) = fold_through(ctx, launch, [sh.total, b_blk.size], [b_acc, b_blk])
    assert a_blk.reshape(-1)[:n_s * 8].reshape(n_s, 8)[:, M.SHELL_NP].sum() == a_acc[sh.s0 + M.ACC["N_PASSED"]] > 1000
    assert_folded(b_acc, a_acc, c_acc, acc_pairs(sh))
    assert_folded(b_blk, a_blk, c_blk, [(s * 8 + lo, s * 8 + hi) for s in range(n_s) for lo, hi in M.SHELL_PAIRS])
    st, _ = check_block(ctx, "shells", params(False), c_blk, lambda raw: M.finalize_shells(raw, n_s, N_E1, True, q), M.SHELL_PAIRS, n_s)
    assert st == 0


@pytest.mark.parametrize("carry", [0, 1 << 20], ids=["normalised", "unnormalised"])
def test_channel_launch_folds_onto_a_crafted_block(chan, carry):
    sh = shape(16, 16, 7)
    t, n_img = N_CHANNELS, 256
    b_acc = crafted_accumulator(sh, 5, carry)
    blk = M.ints(M.consistent_channels(np.random.default_rng(19), t, N_E1, True, n_img, slot_cap=1 << 60))
    e0, p0 = t * 8, t * 8 + t * N_E1
    for c in range(t):
        for j in (M.CHAN_OUT_HI, M.CHAN_SW_HI, M.CHAN_SQ_HI):   # room for the carry: 2^61 quanta more outside, hence in the sum
            blk[c * 8 + j] += 1 << 21
        blk[e0 + c * N_E1 + 1] += 1 << 61
        d = top_pair(blk, c * 8 + M.CHAN_OUT, c * 8 + M.CHAN_OUT_HI, carry)
        total = blk[c * 8 + M.CHAN_SW_HI] * TWO40 + blk[c * 8 + M.CHAN_SW] + d
        blk[c * 8 + M.CHAN_SW], blk[c * 8 + M.CHAN_SW_HI] = M.split_limbs(total)
        d2 = top_pair(blk, c * 8 + M.CHAN_SW, c * 8 + M.CHAN_SW_HI, carry)
        blk[p0 + c * n_img] += d2
        blk[e0 + c * N_E1] += d + d2
        top_pair(blk, c * 8 + M.CHAN_SQ, c * 8 + M.CHAN_SQ_HI, carry)
    b_blk = np.array(blk, dtype=np.int64)
    q = chan.fixed_quanta()
    model = lambda raw: M.finalize_channels(raw, t, N_E1, True, n_img, q)
    assert model(b_blk)[1] == 0
    params = lambda acc: chan.channels_params(N_FOLD, seed=24, image_n=16, spectra=True, n_radial_bins=7, accumulate=acc)
    launch = lambda acc, ptrs: chan.trace_channels_device(params(acc), ptrs[0], ptrs[1])
    (a_acc, a_blk), (c_acc, c_blk) = fold_through(chan, launch, [sh.total, b_blk.size], [b_acc, b_blk])
    assert a_acc[sh.s0 + M.ACC["N_PASSED"]] > 1000 and a_blk[M.CHAN_N] > 1000
    assert_folded(b_acc, a_acc, c_acc, acc_pairs(sh))
    assert_folded(b_blk, a_blk, c_blk, [(c * 8 + lo, c * 8 + hi) for c in range(t) for lo, hi in M.CHAN_PAIRS])
    assert check_block(chan, "channels", params(False), c_blk, model, M.CHAN_PAIRS, t)[0] == 0


TINY = (2, 4)                                                 # the smallest solar tables that build (tests/test_gpu_origin.py)


@pytest.fixture(scope="module")
def tiny():
    rt = sa.RayTracer(make_setup("babyiaxo_xmm", n_radii=TINY[0], n_energies=TINY[1]))
    rt.set_accumulation_mode("fixed64")
    freeze(rt)
    yield rt
    rt.close()


def crafted_head_block(n_cells, seed, carry):
    """An origin / aperture block whose cells add up to its head, the head's two low limbs at 2^40 - 1."""
    rng = np.random.default_rng(seed)
    blk = [0] * (M.HEAD + n_cells * M.CELL)
    at = lambda i, j: M.HEAD + i * M.CELL + j
    for i in range(n_cells):
        blk[at(i, M.CELL_N)] = M.draw(rng, 1 << 40)
        blk[at(i, M.CELL_SW)] = M.draw(rng, 1 << 60)
        blk[at(i, M.CELL_SQ)] = M.draw(rng, 1 << 60)
    blk[M.HEAD_NP] = sum(blk[at(i, M.CELL_N)] for i in range(n_cells))
    for (lo, hi), j in zip(M.HEAD_PAIRS, (M.CELL_SW, M.CELL_SQ)):
        blk[at(1, j)] += 1 << 61                              # high limbs of at least 2^21: room for the carry
        blk[lo], blk[hi] = M.split_limbs(sum(blk[at(i, j)] for i in range(n_cells)))
        blk[at(0, j)] += top_pair(blk, lo, hi, carry)
    assert max(blk) < LIMIT
    return np.array(blk, dtype=np.int64)


@pytest.mark.parametrize("carry", [0, 1 << 20], ids=["normalised", "unnormalised"])
@pytest.mark.parametrize("which", ["origin", "aperture"])
def test_head_launch_folds_onto_a_crafted_block(request, which, carry):
    """The head fold of the origin block, which the aperture block shares; every cell takes the trace's atomics directly."""
    if which == "origin":
        rt = request.getfixturevalue("tiny")
        n_cells = TINY[0] * TINY[1]
        n_slots, trace, finalize = rt.origin_block_len(), rt.trace_origin_device, rt.finalize_origin_device
    else:
        rt = request.getfixturevalue("ctx")
        rt.set_aperture_grid(3, 2, 0.0, 352.0, -100.0, 250.0)   # a window that leaves rays for the outside cell
        n_cells = 3 * 2 + 1
        n_slots, trace, finalize = rt.aperture_block_len(), rt.trace_aperture_device, rt.finalize_aperture_device
    sh = M.Shape(0, 0)
    b_acc = crafted_accumulator(sh, 6, carry)
    b_blk = crafted_head_block(n_cells, 20, carry)
    assert b_blk.size == n_slots
    params = lambda acc: rt.shells_params(N_FOLD, seed=25, image_n=0, spectra=False, accumulate=acc)
    launch = lambda acc, ptrs: trace(params(acc), ptrs[0], ptrs[1])
    (a_acc, a_blk), (c_acc, c_blk) = fold_through(rt, launch, [sh.total, n_slots], [b_acc, b_blk])
    cells = a_blk[M.HEAD:].reshape(n_cells, M.CELL)
    assert cells[:, M.CELL_N].sum() == a_blk[M.HEAD_NP] == a_acc[sh.s0 + M.ACC["N_PASSED"]] > 1000
    assert (cells[:, M.CELL_N] > 0).sum() >= 4               # (the origin table's first energy has no rays: tests/test_gpu_origin.py)
    assert_folded(b_acc, a_acc, c_acc, acc_pairs(sh))
    assert_folded(b_blk, a_blk, c_blk, M.HEAD_PAIRS)
    d = upload(c_blk)                                         # the finalize's own conservation checks: cells against the head
    finalize(params(False), d.data_ptr())
    err = sync(rt)
    assert err is None, str(err)


@pytest.mark.parametrize("carry", [0, 1 << 20], ids=["normalised", "unnormalised"])
@pytest.mark.parametrize("n_bands", [1, 31])
def test_banded_scan_launch_folds_onto_crafted_cells(gas, n_bands, carry):
    """33 masses: a full group of 32 and a group of one; only the first group's launch carries the counts block."""
    n, n_cells = 33, n_bands + 1
    xs = np.linspace(0.002, 0.03, n)
    bands = (30, 240 // n_bands, n_bands)
    b_rows = crafted_rows(n, M.MASS_COUNTERS, 17, carry)
    rng = np.random.default_rng(26 + n_bands)
    spec = [0] * ((n + 1) * n_cells * M.MSPEC_CELL)
    assert len(spec) == L.mass_scan_spectra_len(n, n_bands)
    cell = lambda k, c: (k * n_cells + c) * M.MSPEC_CELL
    pairs = [(cell(k, c) + lo, cell(k, c) + hi) for k in range(n) for c in range(n_cells) for lo, hi in M.MSPEC_PAIRS]
    for lo, hi in pairs:
        spec[lo], spec[hi] = M.split_limbs(M.draw(rng, 1 << 60) + (1 << 61))   # high limbs of at least 2^21: room for the carry
    for k in (0, 31, 32):
        for c in range(n_cells):
            for lo, hi in M.MSPEC_PAIRS:
                top_pair(spec, cell(k, c) + lo, cell(k, c) + hi, carry)
    for c in range(n_cells):
        spec[cell(n, c) + M.MSPEC_N] = M.draw(rng, 1 << 60)
    b_spec = np.array(spec, dtype=np.int64)
    launch = lambda acc, ptrs: gas.trace_mass_scan_spectra_device(gas.trace_params(N_FOLD, seed=27, accumulate=acc), xs, bands,
                                                                  ptrs[0], ptrs[1])
    (a_rows, a_spec), (c_rows, c_spec) = fold_through(gas, launch, [(n + 1) * 8, b_spec.size], [b_rows, b_spec])
    assert a_rows[n * 8] == N_FOLD and a_rows.reshape(n + 1, 8)[:n, M.SCAN_NP].max() > 100
    assert_folded(b_rows, a_rows, c_rows, [(k * 8 + lo, k * 8 + hi) for k in range(n) for lo, hi in ((M.SCAN_SW, M.SCAN_SW_HI), (M.SCAN_SQ, M.SCAN_SQ_HI))])
    assert c_rows[n * 8] == b_rows[n * 8] + N_FOLD
    # what was traced is a banded scan: the cells of a mass add up to its row, the band counts to N_ON_DETECTOR (slot 4)
    a = M.ints(a_spec)
    for k in (0, 31, 32):
        for (lo, hi), (rlo, rhi) in zip(M.MSPEC_PAIRS, ((M.SCAN_SW, M.SCAN_SW_HI), (M.SCAN_SQ, M.SCAN_SQ_HI))):
            total = sum(a[cell(k, c) + hi] * TWO40 + a[cell(k, c) + lo] for c in range(n_cells))
            assert total == int(a_rows[k * 8 + rhi]) * TWO40 + int(a_rows[k * 8 + rlo]), (k, lo)
    assert sum(a[cell(n, c) + M.MSPEC_N] for c in range(n_cells)) == a_rows[n * 8 + 4] > 100
    assert_folded(b_spec, a_spec, c_spec, pairs)               # (the counts block: plain sums)


@pytest.mark.parametrize("carry", [0, 1 << 20], ids=["normalised", "unnormalised"])
def test_angular_scan_images_launch_folds_onto_crafted_blocks(ctx, carry):
    """The scalars of every angle's block go through the scalars fold, once per angle."""
    sh = shape(8, 8)
    k_angles = 3
    angles = np.array(ANGLES[:k_angles])
    b_rows = crafted_rows(k_angles, M.ANGULAR_COUNTERS, 28, carry)
    b_blocks = np.concatenate([crafted_accumulator(sh, 30 + k, carry) for k in range(k_angles)])
    params = lambda acc: ctx.angular_scan_images_params(N_FOLD, seed=29, image_n=8, accumulate=acc)
    launch = lambda acc, ptrs: ctx.trace_angular_scan_images_device(params(acc), angles, ptrs[0], ptrs[1])
    (a_rows, a_blocks), (c_rows, c_blocks) = fold_through(ctx, launch, [(k_angles + 1) * 8, k_angles * sh.total], [b_rows, b_blocks])
    assert a_rows.reshape(k_angles + 1, 8)[:k_angles, M.SCAN_NP].max() > 1000
    assert_folded(b_rows, a_rows, c_rows, [(k * 8 + lo, k * 8 + hi) for k in range(k_angles) for lo, hi in ((M.SCAN_SW, M.SCAN_SW_HI), (M.SCAN_SQ, M.SCAN_SQ_HI))])
    for k in range(k_angles):
        blk = slice(k * sh.total, (k + 1) * sh.total)
        a = a_blocks[blk]
        assert a[sh.s0 + M.ACC["N_RAYS"]] == N_FOLD and a[sh.s0 + M.ACC["N_PASSED"]] == a_rows[k * 8 + M.SCAN_NP]
        assert_folded(b_blocks[blk], a, c_blocks[blk], acc_pairs(sh))
        assert c_blocks[blk][sh.s0 + M.ACC["N_RAYS"]] == b_blocks[blk][sh.s0 + M.ACC["N_RAYS"]] + N_FOLD
        assert check_against_model(ctx, sh, c_blocks[blk], in_place_too=False) == 0
