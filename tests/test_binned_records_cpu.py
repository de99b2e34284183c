"""The host binning reference (tests/binned_records.py) itself, without a GPU.

  * Its formulas are pinned to an independent implementation: the f64 oracle's records, binned by the helper, equal the f64 oracle's
    own trace_histogram / trace_spectra of the same rays (counts exactly, weights to the order of the additions).
  * Mutation checks on the binary128 oracle's records alone, in both accumulation modes (f64, and a FIXED64 stand-in that adds
    rint(v / quantum) per ray with quanta of the size fixed_quanta() gives): check_histogram must FAIL for one ray moved by a pixel
    in x or in y, moved to the next radial bin or energy index, x and y swapped on a window with unequal steps, one weight doubled,
    one ray dropped from `passed`, one ray's x wrong in SUM_X alone, a NaN in a resolved SUM_WEIGHTS_SQ; and must PASS when a ray
    0.5e-9 mm from an edge is put on either side of it.
  * The two conditions of every case of tests/test_gpu_binned_records.py (at most 2 ambiguous rays, detectable share >= 0.90) hold
    for the binary128 oracle's records: six setups x ids [0, 40 000) and [777, 40 780) x (256 x 256 over the chip; 2000 and
    10 000 radial bins over 10 mm; 64 bins up to the median pointdataR), six windows on two setups.  Measured, seed 9: 0 ambiguous
    rays in every case.  Detectable shares at eps = 2e-8, f64 / FIXED64 stand-in (weight bound = 16 x the heaviest ray, headroom
    27), chip-wide: babyiaxo_xmm 0.988 / 0.942, babyiaxo_xmm_gas 0.988 / 0.934, cast_llnl 0.942 / 0.923, cast_abrixas 0.994 / 0.990,
    babyiaxo_xmm_rot 1.0 / 1.0, babyiaxo_xmm_xray 1.0 / 1.0; windows (FIXED64 stand-in, rays inside the image) >= 0.914."""
import functools

import numpy as np
import pytest

from tests import binned_records as B
from tests.conftest import make_setup

N, SEED = B.RANGES[0][0], B.SEED
MODES = ["f64", "fixed64"]


@functools.lru_cache(maxsize=None)
def _setup(name):
    return make_setup(name)


@functools.lru_cache(maxsize=None)
def _case(name, variant, n=N, offset=0):
    from oracle.oracle import Oracle
    full = _setup(name)
    rec = Oracle(full, variant).trace_records(n, seed=SEED, ray_id_offset=offset)
    rec.setflags(write=False)
    return full, rec


def _quanta(rec, mode, bound_factor=16.0):
    """None in f64 mode; else quanta of the size a context has whose weight bound is `bound_factor` x the heaviest ray."""
    return None if mode == "f64" else B.stand_in_quanta(bound_factor * rec["weights"][rec["passed"] != 0].max())


def plain_bin(rec, nx, ny, x_range, y_range, n_bins, radial_max, energies, test_active, quanta=None):
    """A stand-in for the kernel: the statement of the accumulation block (np.add.at adds ray by ray), no envelopes.  f64 sums, or
    with `quanta` what SART_ACCUM_FIXED64 does: every ray adds rint(v / quantum) to an int64, and the sums are converted to f64 once."""
    r = rec[rec["passed"] != 0]
    x, y, rad = r["pointdataX"], r["pointdataY"], r["pointdataR"]
    fixed = (lambda v, q: np.rint(v / q).astype(np.int64)) if quanta is not None else (lambda v, q: v)
    acc = np.int64 if quanta is not None else np.float64
    q = quanta or {"weight": 1.0, "weight_sq": 1.0, "position": 1.0, "reflect": 1.0}
    w, w2, refl = fixed(r["weights"], q["weight"]), fixed(r["weights"] * r["weights"], q["weight_sq"]), fixed(r["reflect"], q["reflect"])
    summ = {"N_PASSED": float(r.size), "SUM_WEIGHTS": w.sum() * q["weight"], "SUM_WEIGHTS_SQ": w2.sum() * q["weight_sq"]}
    for k, v in (("SUM_X", x), ("SUM_Y", y), ("SUM_R", rad)):
        summ[k] = fixed(v, q["position"]).sum() * q["position"]
    fx = (x - x_range[0]) * (1.0 / ((x_range[1] - x_range[0]) / nx))
    fy = (y - y_range[0]) * (1.0 / ((y_range[1] - y_range[0]) / ny))
    inside = (fx >= 0.0) & (fx < nx) & (fy >= 0.0) & (fy < ny)
    summ["N_OUTSIDE_IMAGE"] = float((~inside).sum())
    img = np.zeros((ny, nx), dtype=acc)
    np.add.at(img, (fy[inside].astype(np.int64), fx[inside].astype(np.int64)), w[inside])
    rb = np.minimum((rad * (n_bins / radial_max)).astype(np.int64), n_bins - 1)
    ne = len(energies)
    e = np.full(r.size, ne) if test_active else np.abs(energies[None, :] - r["energiesAx"][:, None]).argmin(axis=1)
    sp = {k: np.zeros(n_bins if k.startswith("radial") else ne + 1, dtype=acc if "counts" not in k else np.float64)
          for k in ("radial_counts", "radial_weights", "energy_counts", "energy_weights", "energy_reflect")}
    np.add.at(sp["radial_counts"], rb, 1.0)
    np.add.at(sp["radial_weights"], rb, w)
    np.add.at(sp["energy_counts"], e, 1.0)
    np.add.at(sp["energy_weights"], e, w)
    np.add.at(sp["energy_reflect"], e, refl)
    for k, key in (("radial_weights", "weight"), ("energy_weights", "weight"), ("energy_reflect", "reflect")):
        sp[k] = sp[k] * q[key]
    return img * q["weight"], summ, sp


@pytest.mark.parametrize("name", ["babyiaxo_xmm", "cast_llnl", "babyiaxo_xmm_rot", "babyiaxo_xmm_xray"])
def test_binned_f64_oracle_records_equal_the_f64_oracles_histogram(name):
    from oracle.oracle import Oracle
    full, rec = _case(name, "f64")
    n_bins, radial_max = 2000, 10.0
    img, summ, sp = Oracle(full).trace_spectra(N, seed=SEED, n_radial_bins=n_bins, radial_max=radial_max)
    b = B.bin_records(rec, *B.chip(full), n_bins, radial_max, full.energies, full.setup.test_active, delta=0.0)
    (s_img, a_img), (s_r, a_r), (s_e, a_e) = b.image, b.radial, b.energy
    assert b.n_passed > 1000 and b.n_ambiguous_image == 0 and b.n_ambiguous_radial == 0    # delta = 0: the f64 records are the rays
    assert summ["N_PASSED"] == b.n_passed and summ["N_OUTSIDE_IMAGE"] == b.outside[0].count[0]
    np.testing.assert_array_equal(sp["radial_counts"], s_r.count)
    np.testing.assert_array_equal(sp["energy_counts"], s_e.count)
    np.testing.assert_array_equal(img != 0, (s_img.count > 0).reshape(256, 256))
    # the oracle adds per thread and then across threads: to the order of the additions (2^-53 per addition)
    for got, want, cnt in ((img.ravel(), s_img.w, s_img.count), (sp["radial_weights"], s_r.w, s_r.count),
                           (sp["energy_weights"], s_e.w, s_e.count), (sp["energy_reflect"], s_e.reflect, s_e.count)):
        assert np.all(np.abs(got - want.astype(np.float64)) <= (cnt + 1) * B.U * np.abs(want.astype(np.float64)))
    assert np.abs(img.ravel() - s_img.w.astype(np.float64)).max() <= 1e-15 * img.max()
    assert summ["SUM_WEIGHTS"] == pytest.approx(float(b.passed[0].w[0]), rel=N * B.U)
    for k in ("SUM_X", "SUM_Y", "SUM_R"):
        assert summ[k] == pytest.approx(float(b.sums[k][0]), rel=N * B.U)
    # and the whole output passes the envelope check with the tightest settings an f64 sum allows
    B.check_histogram(b, img, summ, sp, 0.0, None, name)


def _conditions(b, rec, what, radial=True):
    assert b.n_ambiguous_image <= B.MAX_AMBIGUOUS, what
    assert not radial or b.n_ambiguous_radial <= B.MAX_AMBIGUOUS, what
    for mode in MODES:
        share, share_passed = b.detectable_shares(B.EPS_ORACLE, _quanta(rec, mode))
        print("%s %s: passed %d, ambiguous image %d radial %d, detectable share %.4f (of all passed rays %.4f)"
              % (what, mode, b.n_passed, b.n_ambiguous_image, b.n_ambiguous_radial, share, share_passed))
        assert share >= B.MIN_DETECTABLE, (what, mode, share)


@pytest.mark.parametrize("name", B.SETUPS)
def test_conditions_hold_for_every_case_of_the_gpu_tests(name):
    for n, offset in B.RANGES:
        full, rec = _case(name, "q", n, offset)
        for n_bins, radial_max in B.radial_cases(rec):
            b = B.bin_records(rec, *B.chip(full), n_bins, radial_max, full.energies, full.setup.test_active)
            _conditions(b, rec, "%s ids from %d, %d bins over %g mm" % (name, offset, n_bins, radial_max))
            if radial_max < 10.0:
                assert 0.4 * b.n_passed < b.radial[0].count[-1] < 0.6 * b.n_passed
        assert b.outside[0].count[0] == 0          # the chip-wide image holds every passed ray
        assert b.energy[0].count.sum() == b.n_passed
        if full.setup.test_active:
            assert b.energy[0].count[-1] == b.n_passed
    if name in B.WINDOW_SETUPS:
        full, rec = _case(name, "q")
        for what, nx, ny, xr, yr in B.windows(full, *B.centroid(rec)):
            b = B.bin_records(rec, nx, ny, xr, yr, 2000, 10.0, full.energies, full.setup.test_active)
            _conditions(b, rec, "%s window %s" % (name, what), radial=False)


# ---- mutation checks ------------------------------------------------------------------------------------------------------------
WINDOW = (40, 30)      # unequal steps in x and y, nx != ny
N_BINS, RADIAL_MAX = 2000, 10.0


@functools.lru_cache(maxsize=None)
def _reference(name="cast_llnl"):
    full, rec = _case(name, "q")
    args = (*B.chip(full, *WINDOW), N_BINS, RADIAL_MAX, full.energies, full.setup.test_active)
    return full, rec, args, B.bin_records(rec, *args)


def _median_ray(rec, b, quanta):
    """Index (into rec) of the passed ray of median weight; it is one of the detectable rays."""
    idx = np.flatnonzero(rec["passed"] != 0)
    j = idx[np.argsort(rec["weights"][idx])[idx.size // 2]]
    lo, hi = B.bounds(*b.image, B.EPS_ORACLE, B.half_quantum(quanta, *b.image))
    assert rec["weights"][j] > 2 * (hi - lo)[b.pixel_of_ray[np.searchsorted(idx, j)]]
    return j


def _check(b, out, what, quanta):
    B.check_histogram(b, *out, B.EPS_ORACLE, quanta, str(what))


@functools.lru_cache(maxsize=None)
def _good_sums(mode):
    full, rec, args, b = _reference()
    return plain_bin(rec, *args, _quanta(rec, mode))[1]


def _bin_with_the_true_position_sums(bad, args, mode, quanta):
    """The stand-in's output for mutated records; SUM_X, SUM_Y, SUM_R as of the true ones: the planted error is one of binning."""
    img, summ, sp = plain_bin(bad, *args, quanta)
    for k in ("SUM_X", "SUM_Y", "SUM_R"):
        summ[k] = _good_sums(mode)[k]
    return img, summ, sp


@pytest.mark.parametrize("mode", MODES)
def test_unchanged_records_pass(mode):
    full, rec, args, b = _reference()
    q = _quanta(rec, mode)
    _check(b, plain_bin(rec, *args, q), "unchanged", q)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("mutation", ["pixel_x", "pixel_y", "radial_bin", "energy_index", "swap_xy", "weight_doubled", "dropped",
                                      "sum_x_alone"])
def test_a_planted_error_fails(mutation, mode):
    full, rec, args, b = _reference()
    q = _quanta(rec, mode)
    nx, ny, xr, yr = args[:4]
    j = _median_ray(rec, b, q)
    bad = rec.copy()
    if mutation == "pixel_x":
        bad["pointdataX"][j] += (xr[1] - xr[0]) / nx
    elif mutation == "pixel_y":
        bad["pointdataY"][j] += (yr[1] - yr[0]) / ny
    elif mutation == "radial_bin":
        bad["pointdataR"][j] += RADIAL_MAX / N_BINS
    elif mutation == "energy_index":
        e = int(np.searchsorted(full.energies, rec["energiesAx"][j]))
        bad["energiesAx"][j] = full.energies[e + 1 if e + 1 < full.energies.size else e - 1]
    elif mutation == "swap_xy":
        bad["pointdataX"], bad["pointdataY"] = rec["pointdataY"].copy(), rec["pointdataX"].copy()
    elif mutation == "weight_doubled":
        bad["weights"][j] *= 2.0
    elif mutation == "dropped":
        bad["passed"][j] = 0
    out = _bin_with_the_true_position_sums(bad, args, mode, q)
    if mutation == "sum_x_alone":      # one ray's x a pixel off in the scalar, the image left alone: check_position_sum's to reject
        out[1]["SUM_X"] += (xr[1] - xr[0]) / nx
    with pytest.raises(AssertionError) as e:
        _check(b, out, mutation, q)
    want = {"pixel_x": "image", "pixel_y": "image", "radial_bin": "radial_counts", "energy_index": "energy_counts", "swap_xy": "image",
            "weight_doubled": "image", "dropped": "N_PASSED", "sum_x_alone": "SUM_X"}[mutation]
    assert want in str(e.value), str(e.value)[:300]        # caught at the first slot kind that sees it


@pytest.mark.parametrize("mode", MODES)
def test_position_sums_are_held_to_a_delta_per_ray(mode):
    """SUM_X off by twice its tolerance N_PASSED (delta + 2^-33 mm) fails, by a quarter of it passes."""
    full, rec, args, b = _reference()
    q = _quanta(rec, mode)
    tol = b.n_passed * (B.DELTA_MM + 0.5 * B.POSITION_QUANTUM)
    for key in ("SUM_X", "SUM_Y", "SUM_R"):
        img, summ, sp = plain_bin(rec, *args, q)
        summ[key] += 0.25 * tol
        _check(b, (img, summ, sp), key, q)
        summ[key] += 2 * tol
        with pytest.raises(AssertionError, match=key):
            _check(b, (img, summ, sp), key, q)


def test_fixed64_sum_of_squares_may_read_nan_only_where_unresolved():
    full, rec, args, b = _reference()
    q = _quanta(rec, "fixed64")
    img, summ, sp = plain_bin(rec, *args, q)
    summ["SUM_WEIGHTS_SQ"] = float("nan")
    with pytest.raises(AssertionError, match="SUM_WEIGHTS_SQ"):
        _check(b, (img, summ, sp), "nan", q)
    coarse = dict(q, weight_sq=float(b.sum_w_sq) / b.n_passed)     # squared weights average ONE quantum: unresolved, NaN by design
    _check(b, (img, summ, sp), "nan, unresolved", coarse)
    img, summ, sp = plain_bin(rec, *args)
    summ["SUM_WEIGHTS_SQ"] = float("nan")
    with pytest.raises(AssertionError, match="SUM_WEIGHTS_SQ"):     # f64 mode knows no NaN
        _check(b, (img, summ, sp), "nan, f64", None)


def test_fixed64_reflect_is_held_to_its_own_quantum():
    """energy_reflect of the FIXED64 stand-in, one bin off by one ray's quantum 2^-40 more than its count allows."""
    full, rec, args, b = _reference()
    q = _quanta(rec, "fixed64")
    img, summ, sp = plain_bin(rec, *args, q)
    k = int(np.argmax(b.energy[0].count))
    sp["energy_reflect"][k] += (0.5 * b.energy[0].count[k] + 1) * B.REFLECT_QUANTUM + 2 * B.EPS_ORACLE * float(b.energy[0].reflect[k])
    with pytest.raises(AssertionError, match="energy_reflect"):
        _check(b, (img, summ, sp), "reflect", q)


@pytest.mark.parametrize("mode", MODES)
def test_a_faint_ray_moved_is_caught_by_the_counts(mode):
    """The lightest passed ray weighs nothing beside its radial bin's envelope: the count slots hold it."""
    full, rec, args, b = _reference()
    q = _quanta(rec, mode)
    idx = np.flatnonzero(rec["passed"] != 0)
    j = idx[np.argmin(rec["weights"][idx])]
    bad = rec.copy()
    bad["pointdataR"][j] += RADIAL_MAX / N_BINS
    with pytest.raises(AssertionError, match="radial_counts"):
        _check(b, _bin_with_the_true_position_sums(bad, args, mode, q), "faint", q)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("axis", ["x", "y", "r"])
def test_a_ray_half_a_delta_from_an_edge_passes_on_either_side(axis, mode):
    full, rec, args, b0 = _reference()
    q = _quanta(rec, mode)
    nx, ny, xr, yr = args[:4]
    ref = rec.copy()
    j = _median_ray(rec, b0, q)
    field, edge = {"x": ("pointdataX", xr[0] + 17 * (xr[1] - xr[0]) / nx), "y": ("pointdataY", yr[0] + 11 * (yr[1] - yr[0]) / ny),
                   "r": ("pointdataR", 321 * RADIAL_MAX / N_BINS)}[axis]
    ref[field][j] = edge + 0.5e-9
    b = B.bin_records(ref, *args)
    assert (b.n_ambiguous_radial if axis == "r" else b.n_ambiguous_image) == 1
    for side in (+0.5e-9, -0.5e-9, +0.9e-9, -0.9e-9):
        got = ref.copy()
        got[field][j] = edge + side
        _check(b, plain_bin(got, *args, q), (axis, side), q)


@pytest.mark.parametrize("mode", MODES)
def test_an_empty_slot_must_read_exactly_zero(mode):
    full, rec, args, b = _reference()
    q = _quanta(rec, mode)
    img, summ, sp = plain_bin(rec, *args, q)
    empty = np.flatnonzero((b.image[0].count == 0) & (b.image[1].count == 0))
    assert empty.size
    img.ravel()[empty[0]] = 1e-300
    with pytest.raises(AssertionError, match="image"):
        _check(b, (img, summ, sp), "empty pixel", q)
