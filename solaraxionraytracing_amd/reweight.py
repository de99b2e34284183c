"""The flux of a traced run for another solar model, from its origin map and without a new trace (CPU only).

    python -m solaraxionraytracing_amd.reweight origin_map_IAXO.npz --solarModel solar_model_dataframe.csv [--maxUncovered X]

MAP.npz is what `python -m solaraxionraytracing_amd --originMap` wrote: the detected weight per (solar radius, energy) cell, the grid
and the emission rates the run was traced with.  FILE.csv is an emission table in the reference's layout (Radius, Energy [keV],
emRates) on the same grid.  Prints the reweighted flux, in the units of the traced run, with its Monte-Carlo error, the flux a direct
trace of the new model would print (normalised to the new table's own mass) and `uncovered`: the share of the new model's cell mass
in cells the traced model never sampled.  Exit 1 when that share exceeds --maxUncovered (default 0), 2 for a file that does not fit."""
from __future__ import annotations

import argparse
import sys

import numpy as np

from . import origin, tables


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m solaraxionraytracing_amd.reweight", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("map", metavar="MAP.npz")
    ap.add_argument("--solarModel", required=True, metavar="FILE.csv")
    ap.add_argument("--maxUncovered", type=float, default=0.0)
    args = ap.parse_args(argv)
    m = origin.load_map(args.map)
    missing = [k for k in ("counts", "weights", "weights_sq", "radii", "energies", "n_rays", "rates") if k not in m]
    if missing:
        ap.error("%s holds no %s: not an origin map of --originMap" % (args.map, ", ".join(missing)))
    radii, energies, new = tables.read_solar_model_csv(args.solarModel)
    if radii.shape != m["radii"].shape or energies.shape != m["energies"].shape or not (
            np.allclose(radii, m["radii"], rtol=1e-12, atol=0.0) and np.allclose(energies, m["energies"], rtol=1e-12, atol=0.0)):
        ap.error("%s is not on the grid of the map (%d radii x %d energies)" % (args.solarModel, m["radii"].size, m["energies"].size))
    try:
        res = origin.reweight(m, m["rates"], new, max_uncovered=args.maxUncovered)
    except origin.UncoveredError as e:
        print("reweight:", e, file=sys.stderr)
        return 1
    s_old = origin.model_mass(m["rates"], m["radii"], m["energies"]).sum()
    s_new = origin.model_mass(new, m["radii"], m["energies"]).sum()
    print("traced flux %.17g +- %.6g (%d rays, %d passed)" % (m["weights"].sum(), np.sqrt(m["weights_sq"].sum()), int(m["n_rays"]),
                                                           int(m["counts"].sum())))
    print("reweighted flux %.17g +- %.6g" % (res["flux"], res["flux_error"]))
    print("as a direct trace of the new model prints it %.17g +- %.6g" % (res["flux"] * s_old / s_new, res["flux_error"] * s_old / s_new))
    print("uncovered %.6g" % res["uncovered"])
    return 0


if __name__ == "__main__":
    sys.exit(main())
