"""Host binning reference of the aperture map (include/sart.h: sart_trace_histogram_aperture_device): the entrance points of a set of
passed rays (the record's pointdataXBefore / pointdataYBefore) binned on the host into the cells of a grid over the entrance plane
plus the one slot "outside the window" (index nx * ny), as ApertureArgs and breakdown_histogram_body restate prepareHeatmap's rule.
Pure numpy, no GPU, not a conftest.

The rules are those of tests/binned_records.py, whose pieces do the work here: a ray within DELTA_MM of a cell edge is AMBIGUOUS and
counts for the slots on both sides, every other ray is SURE of its slot; more than MAX_AMBIGUOUS ambiguous rays make a case a bad
input, not a pass.  A slot's N must lie in [sure, sure + ambiguous] (exact where nothing is ambiguous, and every slot no ray reaches
reads 0), its sums within

    FIXED64:  EPS_DEVICE relative plus half a quantum per ray
    f64:      (EPS_DEVICE + 2 k 2^-53) sum w      (k rays in the slot: the summation term, any order of the additions)

of the rays' own sums; for the squared weights the relative term is twice that (the square of a weight that is off by eps is off by
2 eps) and f64 has one more rounding per ray, the product's."""
from __future__ import annotations

import numpy as np

from tests.binned_records import DELTA_MM, EPS_DEVICE, MAX_AMBIGUOUS, U, SlotSets, _axis_candidates, _neighbours, _split, check_slots


class ApertureBinned:
    """`cells`: the pair (sure, ambiguous) of SlotSets over nx * ny + 1 slots, the last one "outside the window" - their `w` holds
    the weights, their `reflect` the squared weights; `slot_of_ray`; `n_ambiguous` (rays); `n_passed`."""

    def __init__(self, x, y, w, nx, ny, x_range, y_range, delta=DELTA_MM):
        x, y, w = (np.asarray(v, dtype=np.float64) for v in (x, y, w))
        assert x.shape == y.shape == w.shape and x.ndim == 1
        assert np.all(np.isfinite(x)) and np.all(np.isfinite(y)) and np.all(np.isfinite(w)) and np.all(w >= 0.0)
        self.nx, self.ny, self.n_passed = int(nx), int(ny), int(w.size)
        n_cells = self.nx * self.ny
        ix, xlo, xhi = _axis_candidates(x, x_range[0], x_range[1], self.nx, delta)
        iy, ylo, yhi = _axis_candidates(y, y_range[0], y_range[1], self.ny, delta)

        def slot_of(jx, jy):
            inside = (jx >= 0) & (jx < self.nx) & (jy >= 0) & (jy < self.ny)
            return np.where(inside, jy * self.nx + jx, n_cells)

        self.slot_of_ray = slot_of(ix, iy)
        cand = {int(j): {int(slot_of(np.int64(a), np.int64(b))) for a in _neighbours(ix[j], xlo[j], xhi[j])
                         for b in _neighbours(iy[j], ylo[j], yhi[j])} for j in np.flatnonzero(xlo | xhi | ylo | yhi)}
        self.cells, self.n_ambiguous = _split(n_cells + 1, self.slot_of_ray, cand, w, w * w)


def bin_entrance(x, y, w, nx, ny, x_range, y_range, delta=DELTA_MM) -> ApertureBinned:
    b = ApertureBinned(x, y, w, nx, ny, x_range, y_range, delta)
    assert b.n_ambiguous <= MAX_AMBIGUOUS, "%d rays within %g mm of a cell edge: choose another grid" % (b.n_ambiguous, delta)
    return b


def check_map(binned, counts, weights, weights_sq, quanta, what=""):
    """The nx * ny + 1 slots of a map (the grid's cells row-major, then the outside cell) against the binned rays.  `quanta`:
    fixed_quanta() of the context for a finalized (or scaled raw) FIXED64 map, None for an f64 map.  No ray is left out: the
    counts add up to the number of rays."""
    sure, amb = binned.cells
    counts = np.asarray(counts).ravel()
    check_slots(counts, sure, amb, 0.0, 0.0, "count", what + " N")
    assert int(np.asarray(counts, dtype=np.float64).sum()) == binned.n_passed, (what, "rays left out or counted twice")
    if quanta is not None:
        h_w, h_w2 = 0.5 * quanta["weight"], 0.5 * quanta["weight_sq"]
        eps_w2 = 2 * EPS_DEVICE
    else:
        h_w, h_w2 = 2 * U * (sure.abs_w + amb.abs_w), 2 * U * (sure.reflect + amb.reflect)
        eps_w2 = 2 * EPS_DEVICE + 2 * U
    check_slots(weights, sure, amb, EPS_DEVICE, h_w, "w", what + " SUM_WEIGHTS")
    check_slots(weights_sq, sure, amb, eps_w2, h_w2, "reflect", what + " SUM_WEIGHTS_SQ")


def naive_bins(x, y, w, nx, ny, x_range, y_range):
    """The same binning by the rule's own words, one ray at a time: (N, sum w, sum w^2) [nx * ny + 1] with math.fsum."""
    import math
    n_cells = nx * ny
    rays = [[] for _ in range(n_cells + 1)]
    for xi, yi, wi in zip(x, y, w):
        fx = (float(xi) - x_range[0]) * nx / (x_range[1] - x_range[0])
        fy = (float(yi) - y_range[0]) * ny / (y_range[1] - y_range[0])
        inside = fx >= 0.0 and fx < nx and fy >= 0.0 and fy < ny
        rays[int(fy) * nx + int(fx) if inside else n_cells].append(float(wi))
    return (np.array([len(r) for r in rays]), np.array([math.fsum(r) for r in rays]), np.array([math.fsum(v * v for v in r) for r in rays]))
