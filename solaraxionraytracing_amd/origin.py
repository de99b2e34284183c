"""What the solar-origin map of a trace answers (include/sart.h "solar-origin map of the histogram trace"; RayTracer.trace_origin).

Every solar ray is drawn in one cell (radius index r, energy index e) of the emission table, with the probability mass of that cell:
rates[r][e] E_e^2 r_r^2, normalised (raytracer.nim:2670-2705, draws :425-471).  Past its cell a ray's weight depends on geometry and
energy alone.  The map ``m`` holds, per cell, the passed rays drawn there: ``counts`` N, ``weights`` D = sum of w, ``weights_sq``
Q = sum of w^2, all [n_radii][n_energies] (a dict: the last element of trace_origin's result, or the arrays of origin_map_*.npz).

Pure numpy: nothing here needs a GPU or the native libraries."""
from __future__ import annotations

import numpy as np


class UncoveredError(ValueError):
    """reweight: the new model has more of its cell mass in cells the traced model never sampled than the caller allows."""


def _maps(m):
    d = np.asarray(m["weights"], dtype=np.float64)
    q = np.asarray(m["weights_sq"], dtype=np.float64)
    if d.ndim != 2 or q.shape != d.shape:
        raise ValueError("the map's weights and weights_sq must be [n_radii][n_energies]")
    return d, q


def radial_profile(m) -> np.ndarray:
    """The detected flux per solar radius index: sum over the energies of D[r][e]."""
    return _maps(m)[0].sum(axis=1)


def cell_mass(flux_radius_cdf, diff_flux_cdfs) -> np.ndarray:
    """The probability that a ray is drawn in cell (r, e): the step of fluxRadiusCDF at r times the step of r's energy CDF at e (a
    draw is the lower bound of its uniform in the CDF)."""
    rcdf = np.asarray(flux_radius_cdf, dtype=np.float64)
    ecdf = np.asarray(diff_flux_cdfs, dtype=np.float64)
    if ecdf.ndim != 2 or rcdf.shape != (ecdf.shape[0],):
        raise ValueError("flux_radius_cdf must be [n_radii] and diff_flux_cdfs [n_radii][n_energies]")
    return np.diff(rcdf, prepend=0.0)[:, None] * np.diff(ecdf, axis=1, prepend=0.0)


def acceptance(m, flux_radius_cdf, diff_flux_cdfs, n_rays) -> np.ndarray:
    """The mean weight of the rays DRAWN in a cell, passed or not: D / (n_rays x cell mass).  NaN where the cell has no mass (no ray
    is ever drawn there)."""
    d, _ = _maps(m)
    mass = cell_mass(flux_radius_cdf, diff_flux_cdfs)
    if mass.shape != d.shape:
        raise ValueError("the CDFs are %r, the map is %r" % (mass.shape, d.shape))
    out = np.full(d.shape, np.nan)
    np.divide(d, float(n_rays) * mass, out=out, where=mass > 0.0)
    return out


def model_mass(rates, radii, energies) -> np.ndarray:
    """rates[r][e] E_e^2 r_r^2: the unnormalised cell mass of an emission table (raytracer.nim:2686)."""
    rates = np.asarray(rates, dtype=np.float64)
    radii, energies = np.asarray(radii, dtype=np.float64), np.asarray(energies, dtype=np.float64)
    if rates.shape != (radii.size, energies.size):
        raise ValueError("rates must be [n_radii][n_energies] of the radii and energies given: %r against (%d, %d)"
                         % (rates.shape, radii.size, energies.size))
    return rates * (energies * energies)[None, :] * (radii * radii)[:, None]


def reweight(m, rates_old, rates_new, max_uncovered: float = 0.0, radii=None, energies=None) -> dict:
    """The trace's result for another emission table on the same grid, by importance reweighting: a ray drawn in cell c stands for
    rates_new[c] / rates_old[c] rays of the new model (the E^2 r^2 factors cancel), in the units of the TRACED model's table - a direct
    trace of the new table is normalised to its own total mass S' = sum of model_mass(rates_new), so it reads S / S' times this.

    Returns ``flux`` = sum D rho, ``flux_error`` = sqrt(sum Q rho^2) (one standard deviation of the Monte Carlo), ``spectrum`` [n_energies],
    ``radial_profile`` [n_radii], ``rho`` and ``uncovered``: the share of the new model's cell mass that sits in cells with
    rates_old == 0, where nothing was sampled and no ratio is formed.  Raises UncoveredError when that share exceeds ``max_uncovered``.
    ``radii`` / ``energies`` default to the map's own (origin_map_*.npz carries them)."""
    d, q = _maps(m)
    old = np.asarray(rates_old, dtype=np.float64)
    new = np.asarray(rates_new, dtype=np.float64)
    if old.shape != d.shape or new.shape != d.shape:
        raise ValueError("rates_old %r and rates_new %r must have the map's shape %r" % (old.shape, new.shape, d.shape))
    if not (np.all(np.isfinite(old)) and np.all(np.isfinite(new)) and np.all(old >= 0.0) and np.all(new >= 0.0)):
        raise ValueError("emission rates must be finite and >= 0")
    covered = old > 0.0
    if np.any((d != 0.0) & ~covered):
        raise ValueError("the map has weight in cells where rates_old is 0: these are not the rates the map was traced with")
    uncovered = 0.0
    if np.any(~covered & (new > 0.0)):
        radii = m.get("radii") if radii is None and hasattr(m, "get") else radii
        energies = m.get("energies") if energies is None and hasattr(m, "get") else energies
        if radii is None or energies is None:
            raise ValueError("rates_new has mass where rates_old is 0: radii and energies are needed to say how much")
        mass = model_mass(new, radii, energies)
        uncovered = float(mass[~covered].sum() / mass.sum())
    if uncovered > max_uncovered:
        raise UncoveredError("%.6g of the new model's cell mass sits in cells the traced model never sampled (rates_old == 0), more "
                             "than max_uncovered = %.6g: it cannot be reweighted to" % (uncovered, max_uncovered))
    rho = np.zeros(d.shape)
    np.divide(new, old, out=rho, where=covered)
    dr = d * rho
    return dict(flux=float(dr.sum()), flux_error=float(np.sqrt((q * rho * rho).sum())), spectrum=dr.sum(axis=0),
                radial_profile=dr.sum(axis=1), rho=rho, uncovered=uncovered)


def load_map(path: str) -> dict:
    """The arrays of an origin_map_*.npz (written by --originMap) as a dict."""
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def write_radial_csv(path: str, m, radii) -> str:
    """flux_by_solar_radius_*.csv: per solar radius the passed rays, the detected flux, its Monte-Carlo error and its share."""
    d, q = _maps(m)
    n = np.asarray(m["counts"]).sum(axis=1)
    prof, err = d.sum(axis=1), np.sqrt(q.sum(axis=1))
    total = prof.sum()
    with open(path, "w") as f:
        f.write("radius index,radius [R_sun],rays,flux,flux error,flux fraction\n")
        for i, r in enumerate(np.asarray(radii, dtype=np.float64)):
            f.write("%d,%.17g,%d,%.17g,%.17g,%.17g\n" % (i, r, int(n[i]), prof[i], err[i], prof[i] / total if total > 0 else 0.0))
    return path
