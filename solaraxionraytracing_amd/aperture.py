"""What the aperture map of a trace answers (include/sart.h "aperture map of the histogram trace"; RayTracer.trace_aperture).

Every ray crosses the telescope's entrance plane at pointEntranceXRT (the record's pointdataXBefore / pointdataYBefore, mm in the
telescope frame).  The map ``m`` holds, per cell of a grid over that plane, the passed rays that entered there: ``counts`` N,
``weights`` D = sum of w, ``weights_sq`` D2 = sum of w^2, all [ny][nx] and row-major as the image is; ``outside`` (N, SUM_WEIGHTS,
SUM_WEIGHTS_SQ) the passed rays that entered outside the window; ``x_edges`` [nx + 1] / ``y_edges`` [ny + 1] the grid (a dict: the
last element of trace_aperture's result, or what load_map reads from aperture_map_*.npz).

Pure numpy: nothing here needs a GPU or the native libraries."""
from __future__ import annotations

import numpy as np

OUTSIDE_KEYS = ("N", "SUM_WEIGHTS", "SUM_WEIGHTS_SQ")


def _maps(m):
    d = np.asarray(m["weights"], dtype=np.float64)
    q = np.asarray(m["weights_sq"], dtype=np.float64)
    if d.ndim != 2 or q.shape != d.shape:
        raise ValueError("the map's weights and weights_sq must be [ny][nx]")
    return d, q


def _outside(m):
    o = m.get("outside") if hasattr(m, "get") else None
    if o is None:
        return 0.0, 0.0, 0.0
    if hasattr(o, "keys"):
        return tuple(float(o[k]) for k in OUTSIDE_KEYS)
    o = np.asarray(o, dtype=np.float64)
    if o.shape != (3,):
        raise ValueError("the map's outside cell must be (N, SUM_WEIGHTS, SUM_WEIGHTS_SQ)")
    return float(o[0]), float(o[1]), float(o[2])


def cell_centres(m):
    """(x [nx], y [ny]) of the cell centres, from the map's edges."""
    xe, ye = np.asarray(m["x_edges"], dtype=np.float64), np.asarray(m["y_edges"], dtype=np.float64)
    d, _ = _maps(m)
    if xe.shape != (d.shape[1] + 1,) or ye.shape != (d.shape[0] + 1,):
        raise ValueError("x_edges / y_edges must be [nx + 1] / [ny + 1] of a [ny][nx] map: %r, %r against %r" % (xe.shape, ye.shape, d.shape))
    return 0.5 * (xe[:-1] + xe[1:]), 0.5 * (ye[:-1] + ye[1:])


def save_map(path: str, m, n_rays) -> str:
    """aperture_map_*.npz: counts, weights, weights_sq [ny][nx], outside (N, sum of w, sum of w^2), x_edges, y_edges, n_rays and the
    head (N_PASSED, SUM_WEIGHTS, SUM_WEIGHTS_SQ of the whole run)."""
    d, q = _maps(m)
    cell_centres(m)   # (the edges fit the map)
    head = m.get("head") or {}
    o = _outside(m)
    np.savez_compressed(path, counts=np.asarray(m["counts"]), weights=d, weights_sq=q, outside=np.array(o),
                        x_edges=np.asarray(m["x_edges"], dtype=np.float64), y_edges=np.asarray(m["y_edges"], dtype=np.float64),
                        n_rays=np.float64(n_rays),
                        head=np.array([head.get("N_PASSED", np.asarray(m["counts"]).sum() + o[0]), head.get("SUM_WEIGHTS", d.sum() + o[1]),
                                       head.get("SUM_WEIGHTS_SQ", q.sum() + o[2])], dtype=np.float64))
    return path


def load_map(path: str) -> dict:
    """The arrays of an aperture_map_*.npz as the dict the functions here take (``outside`` and ``head`` as dicts again)."""
    with np.load(path) as z:
        m = {k: z[k] for k in z.files}
    m["outside"] = dict(zip(OUTSIDE_KEYS, (float(v) for v in m["outside"])))
    m["head"] = dict(zip(("N_PASSED", "SUM_WEIGHTS", "SUM_WEIGHTS_SQ"), (float(v) for v in m["head"])))
    m["n_rays"] = float(m["n_rays"])
    return m


def radial_profile(m, n_bins: int) -> dict:
    """The detected flux per annulus of the entrance plane about the optical axis (the frame's origin): the cells' D, D2 and N summed
    by the radius of the cell CENTRE into ``n_bins`` equal annuli from 0 to the largest centre radius (that cell in the last bin).
    Returns ``r_edges`` [n_bins + 1], ``flux``, ``sigma`` (sqrt of the summed D2) and ``counts`` [n_bins].  The outside cell has no
    place and is left out."""
    n_bins = int(n_bins)
    if n_bins < 1:
        raise ValueError("n_bins must be >= 1")
    d, q = _maps(m)
    xc, yc = cell_centres(m)
    r = np.hypot(xc[None, :], yc[:, None])
    r_max = float(r.max())
    edges = np.linspace(0.0, r_max if r_max > 0.0 else 1.0, n_bins + 1)
    idx = np.minimum(np.searchsorted(edges, r.ravel(), side="right") - 1, n_bins - 1)
    flux = np.bincount(idx, weights=d.ravel(), minlength=n_bins)
    var = np.bincount(idx, weights=q.ravel(), minlength=n_bins)
    cnt = np.bincount(idx, weights=np.asarray(m["counts"], dtype=np.float64).ravel(), minlength=n_bins)
    return dict(r_edges=edges, flux=flux, sigma=np.sqrt(var), counts=cnt)


def reweight(m, factor, outside_factor: float = 0.0) -> dict:
    """The trace's flux for anything that multiplies a ray's weight by a function of its entrance point, ``factor`` [ny][nx] per cell
    (an aperture stop or a masked sector exactly, where the function is constant per cell; a smooth profile to first order in the cell
    size).  ``flux`` = sum D f (+ the outside cell's D x ``outside_factor``), ``sigma`` = sqrt(sum D2 f^2) likewise (one standard
    deviation of the Monte Carlo), ``uncovered`` = the outside cell's share of the traced flux: what the map cannot place."""
    d, q = _maps(m)
    f = np.asarray(factor, dtype=np.float64)
    if f.shape != d.shape:
        raise ValueError("factor %r must have the map's shape %r ([ny][nx])" % (f.shape, d.shape))
    if not np.all(np.isfinite(f)) or not np.isfinite(outside_factor):
        raise ValueError("factors must be finite")
    _, d_out, q_out = _outside(m)
    total = float(d.sum()) + d_out
    return dict(flux=float((d * f).sum()) + d_out * float(outside_factor),
                sigma=float(np.sqrt((q * f * f).sum() + q_out * float(outside_factor) ** 2)),
                uncovered=d_out / total if total > 0.0 else 0.0)


def write_csv(path: str, m) -> str:
    """aperture_image_*.csv: per cell its centre (x, y in mm), the passed rays N, the detected flux and its Monte-Carlo error, rows in
    the map's order (y outer, x inner)."""
    d, q = _maps(m)
    xc, yc = cell_centres(m)
    n = np.asarray(m["counts"])
    with open(path, "w") as f:
        f.write("x,y,N,flux,sigma\n")
        for iy in range(d.shape[0]):
            for ix in range(d.shape[1]):
                f.write("%.17g,%.17g,%d,%.17g,%.17g\n" % (xc[ix], yc[iy], int(n[iy, ix]), d[iy, ix], np.sqrt(q[iy, ix])))
    return path
