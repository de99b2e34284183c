"""Host binning reference of the fused histogram: the Axion records of a set of rays, binned on the host as prepareHeatmap
(raytracer.nim:818-842) and generateResultPlots define and as the accumulation block of trace_histogram_kernel restates.  Pure numpy,
no GPU, not a conftest.

The records come from another computation than the histogram under test (the binary128 oracle, or the record kernel), so a ray's
position and weight need not have the same last bits on both sides.  Equality is therefore replaced by an envelope:

  * a ray farther than DELTA_MM from every edge of its slot is SURE to be in that slot;
  * a ray within DELTA_MM of an edge is AMBIGUOUS: it may be in its own slot or in the one across the edge, and counts for both;
  * weights agree to a relative `eps`, plus what the accumulation itself rounds: half a quantum per ray in SART_ACCUM_FIXED64, the
    summation term n 2^-53 sum|w| in f64.

The constants are bounds the project asserts elsewhere (tests/test_gpu_parity.py): positions of the record kernel against the
binary128 oracle below 1e-10 mm (DELTA_MM is ten times that, for the specialised instantiations whose contraction differs from the
record kernel's), weights and reflect to rtol 2e-8 (EPS_ORACLE); instantiations of one source against each other to 1e-12
(EPS_DEVICE).  They are far smaller than one ray's contribution: see Binned.detectable_shares.

Slot kinds: image pixel [int(fy)][int(fx)] plus one slot "outside the image" (index nx * ny), radial bin, energy index."""
from __future__ import annotations

import numpy as np

DELTA_MM = 1e-9
EPS_ORACLE = 2e-8
EPS_DEVICE = 1e-12
POSITION_QUANTUM = 2.0 ** -32      # kFixedPositionScale of the kernels: SUM_X, SUM_Y, SUM_R count in 2^-32 mm
REFLECT_QUANTUM = 2.0 ** -40       # kFixedReflectScale: energy_reflect counts in 2^-40
MAX_AMBIGUOUS = 2                  # a case with more ambiguous rays is a bad choice of inputs, not a pass
MIN_DETECTABLE = 0.90              # share of passed rays heavier than twice the envelope of their own pixel
U = 2.0 ** -53                     # unit roundoff of f64
# the sums of this module are taken in long double (x87: 2^-64); their own summation term is part of every bound
HOST_U = float(np.finfo(np.longdouble).eps) / 2


class SlotSets:
    """Per slot of one kind: number of rays, sum of w, sum of |w| and sum of reflect of one set (sure or ambiguous)."""

    def __init__(self, n_slots):
        self.count = np.zeros(n_slots, dtype=np.int64)
        self.w = np.zeros(n_slots, dtype=np.longdouble)
        self.abs_w = np.zeros(n_slots, dtype=np.longdouble)
        self.reflect = np.zeros(n_slots, dtype=np.longdouble)

    def add(self, slot, w, reflect):
        """Adds rays (arrays) to their slots; long-double sums, rays of a slot in ray order."""
        slot = np.asarray(slot, dtype=np.int64)
        if slot.size == 0:
            return
        order = np.argsort(slot, kind="stable")
        s = slot[order]
        starts = np.flatnonzero(np.r_[True, s[1:] != s[:-1]])
        at = s[starts]
        self.count[at] += np.diff(np.r_[starts, s.size])
        wl = np.asarray(w, dtype=np.longdouble)[order]
        self.w[at] += np.add.reduceat(wl, starts)
        self.abs_w[at] += np.add.reduceat(np.abs(wl), starts)
        self.reflect[at] += np.add.reduceat(np.asarray(reflect, dtype=np.longdouble)[order], starts)

    def part(self, sl):
        """The slots of the slice `sl` as a SlotSets of their own."""
        out = SlotSets(0)
        out.count, out.w, out.abs_w, out.reflect = self.count[sl], self.w[sl], self.abs_w[sl], self.reflect[sl]
        return out


def _axis_candidates(v, v_min, v_max, n, delta):
    """Per ray: index floor(f) with f = (v - v_min) n / (v_max - v_min), and whether the ray lies within delta (in mm) of the
    lower / the upper edge of that index."""
    step = (v_max - v_min) / n
    f = (v - v_min) * n / (v_max - v_min)
    k = np.floor(f)
    near_lo = (f - k) * step <= delta
    near_hi = (k + 1.0 - f) * step <= delta
    return np.clip(k, -2.0, n + 1.0).astype(np.int64), near_lo, near_hi      # beyond -1 / n every index means "outside"


def _neighbours(k, near_lo, near_hi):
    """Candidate indices of one ray on one axis: its own, and the one across every edge it is near."""
    return [int(k)] + ([int(k) - 1] if near_lo else []) + ([int(k) + 1] if near_hi else [])


def _split(n_slots, own, candidates, w, refl):
    """(sure, ambiguous) SlotSets and the number of ambiguous rays.  `candidates`: {ray: set of slots} of the rays near an edge; a
    ray whose candidates are one slot (two sides of an edge that both mean "outside", or the clamp into the last radial bin) is sure."""
    amb_rays = sorted(j for j, c in candidates.items() if len(c) > 1)
    is_amb = np.zeros(own.size, dtype=bool)
    is_amb[amb_rays] = True
    sure, amb = SlotSets(n_slots), SlotSets(n_slots)
    sure.add(own[~is_amb], w[~is_amb], refl[~is_amb])
    for j in amb_rays:
        c = sorted(candidates[j])
        amb.add(c, np.full(len(c), w[j]), np.full(len(c), refl[j]))
    return (sure, amb), len(amb_rays)


class Binned:
    """The passed records binned.  `image` (nx * ny pixels), `outside` (one slot), `radial`, `energy`, `passed` (every passed ray as
    one slot): pairs (sure, ambiguous) of SlotSets; `sums`: SUM_X, SUM_Y, SUM_R with their sums of magnitudes; `n_ambiguous_image`,
    `n_ambiguous_radial`: rays (not slots); `pixel_of_ray`: pixel index of every passed ray, nx * ny for a ray outside."""

    def __init__(self, rec, nx, ny, x_range, y_range, n_radial_bins, radial_max, energies, test_active, delta=DELTA_MM):
        p = rec["passed"] != 0
        x, y, r = (rec[f][p].astype(np.float64) for f in ("pointdataX", "pointdataY", "pointdataR"))
        w, refl, e_ax = rec["weights"][p].astype(np.float64), rec["reflect"][p].astype(np.float64), rec["energiesAx"][p]
        assert np.all(w >= 0.0) and np.all(np.isfinite(w)) and np.all(r >= 0.0)
        self.nx, self.ny, self.n_radial_bins, self.delta = int(nx), int(ny), int(n_radial_bins), delta
        self.n_passed = int(p.sum())
        self.w = w
        ld = np.longdouble
        self.sums = {k: (v.astype(ld).sum(), np.abs(v).astype(ld).sum()) for k, v in (("SUM_X", x), ("SUM_Y", y), ("SUM_R", r))}
        self.sum_w_sq = (w.astype(ld) ** 2).sum()

        # ---- image: pixel iy * nx + ix, or slot nx * ny for a ray outside --------------------------------------------------
        n_img = self.nx * self.ny
        ix, xlo, xhi = _axis_candidates(x, x_range[0], x_range[1], self.nx, delta)
        iy, ylo, yhi = _axis_candidates(y, y_range[0], y_range[1], self.ny, delta)

        def slot_of(jx, jy):
            inside = (jx >= 0) & (jx < self.nx) & (jy >= 0) & (jy < self.ny)
            return np.where(inside, jy * self.nx + jx, n_img)

        self.pixel_of_ray = slot_of(ix, iy)
        cand = {int(j): {int(slot_of(np.int64(a), np.int64(b))) for a in _neighbours(ix[j], xlo[j], xhi[j])
                         for b in _neighbours(iy[j], ylo[j], yhi[j])} for j in np.flatnonzero(xlo | xhi | ylo | yhi)}
        (sure, amb), self.n_ambiguous_image = _split(n_img + 1, self.pixel_of_ray, cand, w, refl)
        self.image = (sure.part(slice(0, n_img)), amb.part(slice(0, n_img)))
        self.outside = (sure.part(slice(n_img, None)), amb.part(slice(n_img, None)))

        # ---- radial: min(int(R n / radial_max), n - 1); the last bin has no upper edge ------------------------------------
        nb = self.n_radial_bins
        kr, rlo, rhi = _axis_candidates(r, 0.0, radial_max, nb, delta)
        cand_r = {int(j): {min(max(k, 0), nb - 1) for k in _neighbours(kr[j], rlo[j], rhi[j])} for j in np.flatnonzero(rlo | rhi)}
        self.radial, self.n_ambiguous_radial = _split(nb, np.clip(kr, 0, nb - 1), cand_r, w, refl)

        # ---- energy index: n_energies for the X-ray test source, else where the table holds the ray's energy exactly --------
        energies = np.asarray(energies, dtype=np.float64)
        ne = energies.size
        if test_active:
            e_idx = np.full(w.size, ne, dtype=np.int64)
        else:
            e_idx = np.minimum(np.searchsorted(energies, e_ax), ne - 1)
            assert np.array_equal(energies[e_idx], e_ax), "a passed ray's energiesAx is no entry of full.energies"
        self.energy, _ = _split(ne + 1, e_idx, {}, w, refl)     # no edges: every ray is sure
        self.passed, _ = _split(1, np.zeros(w.size, dtype=np.int64), {}, w, refl)

    def detectable_shares(self, eps, quanta):
        """(inside, passed): the share of the rays that are heavier than twice the envelope (upper minus lower bound) of their own
        weight slot - moving such a ray to another slot must fail check_slots - among the rays inside the image, against their pixel,
        and among all passed rays, the rays outside the image against the slot "outside" (1.0 where there is no such ray).
        `quanta` as in check_histogram.  The first is the condition (>= MIN_DETECTABLE): a ray outside the image has no pixel, the
        slot "outside" of a window that cuts the spot holds thousands of rays and hides the fainter half of them, and what holds a
        ray outside - as it holds the faint tail of the fifty decades of weights everywhere - is a count without slack
        (N_OUTSIDE_IMAGE; radial_counts, energy_counts).  An image that no ray reaches has share 1.0 and is held by these counts and
        by "an empty slot reads exactly 0" alone.  The second share is reported beside it."""
        width = np.zeros(self.nx * self.ny + 1, dtype=np.longdouble)
        for sets, sl in ((self.image, slice(0, -1)), (self.outside, slice(-1, None))):
            lo, hi = bounds(*sets, eps, half_quantum(quanta, *sets))
            width[sl] = hi - lo
        seen = self.w.astype(np.longdouble) > 2 * width[self.pixel_of_ray]
        inside = self.pixel_of_ray < self.nx * self.ny
        return (float(seen[inside].mean()) if inside.any() else 1.0), (float(seen.mean()) if seen.size else 1.0)


def bin_records(rec, nx, ny, x_range, y_range, n_radial_bins, radial_max, energies, test_active, delta=DELTA_MM):
    return Binned(rec, nx, ny, x_range, y_range, n_radial_bins, radial_max, energies, test_active, delta)


def half_quantum(quanta, sure, ambiguous, quantity="w", key="weight"):
    """h of bounds().  SART_ACCUM_FIXED64 (`quanta` = fixed_quanta() of the context): half the quantum, every ray adds
    rint(v / quantum); SART_ACCUM_F64 (`quanta` None): the per-ray share of the summation term n 2^-53 sum|v| of a slot's n rays
    (any order of the additions)."""
    if quanta is not None:
        return 0.5 * (REFLECT_QUANTUM if quantity == "reflect" else quanta[key])
    return U * ((sure.abs_w + ambiguous.abs_w) if quantity == "w" else (sure.reflect + ambiguous.reflect))


def bounds(sure, ambiguous, eps, half_quantum, quantity="w"):
    """[lower, upper] of every slot's sum of `quantity` ("w" or "reflect"; both are >= 0):
       sum_sure v (1 - eps) - h |sure|  <=  got  <=  sum_(sure + amb) v (1 + eps) + h (|sure| + |amb|),
    widened by the summation term of this module's own long-double sums."""
    if quantity == "w":
        v_s, m_s, v_a, m_a = sure.w, sure.abs_w, ambiguous.w, ambiguous.abs_w
    else:
        v_s, m_s, v_a, m_a = sure.reflect, sure.reflect, ambiguous.reflect, ambiguous.reflect
    n_s, n_a = sure.count.astype(np.longdouble), ambiguous.count.astype(np.longdouble)
    h = np.asarray(half_quantum, dtype=np.longdouble)
    host = HOST_U * (n_s + n_a) * (m_s + m_a)
    return v_s - eps * m_s - h * n_s - host, v_s + v_a + eps * (m_s + m_a) + h * (n_s + n_a) + host


def check_slots(got, sure, ambiguous, eps, half_quantum, quantity="w", what=""):
    """The one rule every test applies.  quantity "count": |sure| <= got <= |sure| + |ambiguous|, integers, no other slack;
    "w" / "reflect": bounds().  A slot whose two sets are both empty must read exactly 0 (both rules give [0, 0] there)."""
    g = np.asarray(got).ravel()
    assert g.size == sure.count.size, (what, g.size, sure.count.size)
    if quantity == "count":
        assert np.all(g == np.rint(g)), (what, "a count is no integer")
        g = g.astype(np.int64)
        lo, hi = sure.count, sure.count + ambiguous.count
    else:
        g = g.astype(np.longdouble)
        lo, hi = bounds(sure, ambiguous, eps, half_quantum, quantity)
    bad = np.flatnonzero(~((g >= lo) & (g <= hi)))        # (a NaN is bad)
    if bad.size:
        rows = ["slot %d: got %r, want [%r, %r] (sure %d, ambiguous %d)" % (j, g[j], lo[j], hi[j], sure.count[j], ambiguous.count[j])
                for j in bad[:8]]
        raise AssertionError("%s %s: %d of %d slots outside the envelope\n  %s" % (what, quantity, bad.size, g.size, "\n  ".join(rows)))


def check_position_sum(got, binned, key, what=""):
    """SUM_X, SUM_Y, SUM_R: |got - sum_passed v| <= N_PASSED (delta + 0.5 * 2^-32) mm, and the f64 summation term."""
    want, mag = binned.sums[key]
    n = binned.n_passed
    tol = n * (binned.delta + 0.5 * POSITION_QUANTUM) + n * (U + HOST_U) * mag
    assert abs(np.longdouble(got) - want) <= tol, (what, key, got, float(want), float(tol))


def check_histogram(binned, image, summary, spectra, eps, quanta, what=""):
    """Every output of one histogram launch (or of an accumulation of several) against the binned records of the same rays.
    `quanta`: fixed_quanta() of the context in SART_ACCUM_FIXED64, None in f64 mode.  `spectra`: None for a launch without."""
    b = binned

    def weights(got, sets, name, quantity="w", key="weight", factor=1):
        check_slots(got, *sets, factor * eps, half_quantum(quanta, *sets, quantity, key), quantity, what + " " + name)

    def counts(got, sets, name):
        check_slots(got, *sets, 0.0, 0.0, "count", what + " " + name)

    counts([summary["N_PASSED"]], b.passed, "N_PASSED")
    counts([summary["N_OUTSIDE_IMAGE"]], b.outside, "N_OUTSIDE_IMAGE")
    image = np.asarray(image, dtype=np.float64)
    assert image.shape == (b.ny, b.nx), (what, image.shape)
    weights(image, b.image, "image")
    weights([summary["SUM_WEIGHTS"]], b.passed, "SUM_WEIGHTS")
    sq = SlotSets(1)
    sq.count[0], sq.w[0], sq.abs_w[0] = b.n_passed, b.sum_w_sq, b.sum_w_sq
    if quanta is not None and np.isnan(summary["SUM_WEIGHTS_SQ"]):
        # include/sart.h, "unresolved": squared weights that average below 2^6 of their quanta read NaN, by design
        assert b.sum_w_sq < (2.0 ** 6 + 0.5) * quanta["weight_sq"] * b.n_passed, (what, "SUM_WEIGHTS_SQ is NaN though resolved")
    else:
        weights([summary["SUM_WEIGHTS_SQ"]], (sq, SlotSets(1)), "SUM_WEIGHTS_SQ", key="weight_sq", factor=2)
    for key in ("SUM_X", "SUM_Y", "SUM_R"):
        check_position_sum(summary[key], b, key, what)
    # weight outside the image = SUM_WEIGHTS - image.sum(): a difference of two rounded numbers, so this one derived slot carries
    # their rounding besides its own envelope.  FIXED64: both are sums of the same integers, each rounded once to f64 when it is
    # finalized (2^-53 of SUM_WEIGHTS each); f64: each side is a sum of up to N_PASSED terms (N_PASSED 2^-53 sum|w| each).  The
    # pixel sum is taken here in long double.  The slot's "exactly 0" is N_OUTSIDE_IMAGE's, above.
    total = np.longdouble(summary["SUM_WEIGHTS"])
    outside = total - image.astype(np.longdouble).sum()
    lo, hi = bounds(*b.outside, eps, half_quantum(quanta, *b.outside))
    slack = (2 * U + HOST_U * image.size) * total + (0.0 if quanta is not None else 2 * U * b.n_passed * b.passed[0].abs_w[0])
    assert lo[0] - slack <= outside <= hi[0] + slack, (what, "weight outside the image", float(outside), float(lo[0]), float(hi[0]))
    if spectra is None:
        return
    counts(spectra["radial_counts"], b.radial, "radial_counts")
    weights(spectra["radial_weights"], b.radial, "radial_weights")
    counts(spectra["energy_counts"], b.energy, "energy_counts")
    weights(spectra["energy_weights"], b.energy, "energy_weights")
    weights(spectra["energy_reflect"], b.energy, "energy_reflect", quantity="reflect")


def stand_in_quanta(w_max, headroom_bits=27):
    """Quanta of the size fixed_quanta() gives for a context whose weight bound is `w_max` (include/sart.h, "quanta": weights in
    2^(e - 63 + headroom) with bound < 2^e, squared weights in 2^(2 e - 39)), for CPU stand-ins of the FIXED64 accumulation."""
    e = int(np.frexp(w_max)[1])
    return {"weight": 2.0 ** (e - 63 + headroom_bits), "weight_sq": 2.0 ** (2 * e - 39), "position": POSITION_QUANTUM,
            "reflect": REFLECT_QUANTUM}


# ---- the cases of tests/test_gpu_binned_records.py; tests/test_binned_records_cpu.py holds each to the two conditions first ----
SEED = 9
RANGES = ((40_000, 0), (40_003, 777))      # (n, ray_id_offset); the second: neither a multiple of 256 nor of 64, and not aligned
SETUPS = ["babyiaxo_xmm",        # constant-path variant, LDS tile in ring 1's column
          "babyiaxo_xmm_gas",    # path carried
          "cast_llnl",           # no stage A0
          "cast_abrixas", "babyiaxo_xmm_rot", "babyiaxo_xmm_xray"]
WINDOW_SETUPS = ["babyiaxo_xmm", "cast_llnl"]
SPECTRA_SETUPS = ["babyiaxo_xmm", "cast_llnl", "babyiaxo_xmm_xray"]


def chip(full, nx=256, ny=256):
    s = full.setup
    return nx, ny, (0.0, s.chip_x_max), (0.0, s.chip_y_max)


def centroid(rec):
    p = rec["passed"] != 0
    return float(np.round(rec["pointdataX"][p].mean(), 6)), float(np.round(rec["pointdataY"][p].mean(), 6))


def windows(full, cx, cy):
    """(name, nx, ny, x range, y range): the three of tests/test_gpu_tile64.py around the spot's centroid (cx, cy), then a window
    with unequal steps and nx != ny, a one-column y slice through the spot and an image of one pixel."""
    s = full.setup
    px = s.chip_x_max / 256.0
    far_x = 0.0 if cx > 0.5 * s.chip_x_max else s.chip_x_max - 64 * px
    far_y = 0.0 if cy > 0.5 * s.chip_y_max else s.chip_y_max - 64 * px
    return [("straddling", 128, 128, (cx, cx + 128 * px), (cy - 10 * px, cy + 118 * px)),
            ("outside", 64, 64, (far_x, far_x + 64 * px), (far_y, far_y + 64 * px)),
            ("small", 40, 48, (cx - 20 * px, cx + 20 * px), (cy - 24 * px, cy + 24 * px)),
            ("unequal steps", 120, 90, (0.0, s.chip_x_max), (0.0, s.chip_y_max)),
            ("y slice", 1, 280, (cx - 0.05, cx + 0.05), (0.0, s.chip_y_max)),
            ("one pixel", 1, 1, (cx - 0.03, cx + 0.04), (cy - 0.02, cy + 0.03))]


def radial_cases(rec):
    """(n_radial_bins, radial_max): 2000 and 10 000 bins over 10 mm (the reference's 0.001 mm), and a radial_max at the median
    pointdataR - about half of the passed rays clamp into the last bin.  (64 bins there: the 2000 edges of a 2.4 mm range lie
    1.2e-6 mm apart, and several of 1e4 rays fall within 1e-9 mm of one.)"""
    med = float(np.round(np.median(rec["pointdataR"][rec["passed"] != 0]), 4))
    return [(2000, 10.0), (10_000, 10.0), (64, med)]
