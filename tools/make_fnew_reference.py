#!/usr/bin/env python3
"""Writes tests/golden/fnew_reference.json: fNew(w, y) by mpmath quadrature at 50 digits (tests/emission_reference.py,
`fnew_exact`) for every (w, y) and (w, sqrt(2) y) pair of the emission tests' lattice case - 17 AGSS09 zones by 32 energies.
Numbers only: w and y as hex floats, the value to 40 digits.  CPU only; a few minutes on a handful of cores.

    python tools/make_fnew_reference.py [--jobs N] [--out PATH]
"""
import argparse
import json
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import emission_reference as ER   # noqa: E402


def _one(pair):
    w, y = pair
    return [w.hex(), y.hex(), ER.M.nstr(ER.fnew_exact(w, y), 40, min_fixed=0, max_fixed=0)]


def lattice_pairs():
    from solaraxionraytracing_amd import emission as em
    all_zones = em.solar_zones()
    zones = [all_zones[i] for i in ER.select_zones(all_zones)]
    case = ER.lattice_case(zones)
    pairs = []
    for R, z in enumerate(zones):
        c = ER.zone_constants(z, R)
        for E in case.per_zone[R]:
            w = float(E) / c["temp_table"]
            pairs += [(w, c["y"]), (w, c["y_sqrt2"])]
    return sorted(set(pairs))


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--jobs", type=int, default=min(16, len(os.sched_getaffinity(0))))
    ap.add_argument("--out", default=ER.GOLDEN_FNEW)
    a = ap.parse_args()
    pairs = lattice_pairs()
    with multiprocessing.Pool(a.jobs) as pool:
        entries = pool.map(_one, pairs, chunksize=4)
    with open(a.out, "w") as f:
        json.dump({"what": "fNew(w, y), readOpacityFile.nim:296-326, mpmath tanh-sinh at 50 digits; [w.hex(), y.hex(), value]",
                   "entries": entries}, f, indent=0)
        f.write("\n")
    print("%d entries -> %s" % (len(entries), a.out))


if __name__ == "__main__":
    main()
